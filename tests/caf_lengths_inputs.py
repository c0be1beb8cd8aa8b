"""Inputs and yardstick of the cross-ambiguity search's length and shift-edge tests (tests/test_caf_lengths_host.py on the
CPU, tests/caf_lengths/test_round6_gpu.py on the GPU).  Not a test module.

The yardstick is ``sweep_bins``: the definition of include/gpsjam.h (gj_xcorr_caf_dev) in float64 for an ARBITRARY list
of bins, with one forward transform per antenna -- caf_restatement.sweep takes a contiguous range only, and the bins that
matter here (+-1, around L1 = L / 4096, +-(L/2 - 1)) lie far apart.  It uses the same identity as ``sweep``
(FFT_L(x_j^(b))[k] = Z_j[(k + b) mod L], exact because the slice is zero-padded to L) and knows nothing of the kernels'
row / column layout; the host test holds it to ``sweep`` and to the literal ``direct_bin``.

Tolerances are the existing ones: k5_check.PEAK_RTOL and MARGIN_ATOL (1e-4 each) on peaks and margins, lags exact in
every cell whose float64 lag margin is at least caf_restatement.LAG_NEAR_TIE -- and the inputs are built so that this is
EVERY cell (asserted on the reference before anything is compared)."""
from typing import NamedTuple

import numpy as np

import caf_restatement as caf
import k5_check as k5

PEAK_RTOL, MARGIN_ATOL, GAP = k5.PEAK_RTOL, k5.MARGIN_ATOL, k5.GAP
LAG_NEAR_TIE = caf.LAG_NEAR_TIE
ROW = 4096                                   # the contiguous row of K5's four-step transform: L = L1 x 4096


# ------------------------------------------------------------------ the yardstick
def unpack(raw, offset: float = 127.5) -> np.ndarray:
    """x = (I - offset) + j(Q - offset) in complex128 (un-normalised: the search honours gj_set_unpack's offset only)."""
    raw = np.asarray(raw, np.uint8)
    return (raw[0::2].astype(np.float64) - offset) + 1j * (raw[1::2].astype(np.float64) - offset)


def spectrum(raw, offset: float = 127.5) -> np.ndarray:
    x = unpack(raw, offset)
    return np.fft.fft(x, caf.fft_len(x.size))


def bin_of_spectra(Zj: np.ndarray, Zi: np.ndarray, b: int, n: int) -> caf.BinPeak:
    """|c_b| over the 'full' lag range from the two spectra: c_b[lag mod L] = sum_t x_j^(b)[t + lag] conj(x_i[t])."""
    L = Zj.size
    c = np.fft.ifft(np.roll(Zj, -int(b)) * np.conj(Zi))
    return caf._pick(np.abs(np.concatenate([c[L - (n - 1):], c[:n]])), n)


def sweep_bins(raw_j, raw_i, bins, offset: float = 127.5):
    """The bins of the list ``bins`` (any order, any spacing), float64: a list of caf.BinPeak in the list's order."""
    n = np.asarray(raw_i).size // 2
    Zj, Zi = spectrum(raw_j, offset), spectrum(raw_i, offset)
    return [bin_of_spectra(Zj, Zi, b, n) for b in bins]


def winner_of(bins, recs) -> caf.Surface:
    """The pair's answer over the increasing list ``bins``: the larger peak, then the earlier bin (caf.winner for a list)."""
    assert list(bins) == sorted(set(bins))
    s = caf.winner(recs, 0)
    return s._replace(bin=int(bins[s.bin]))


def search_bins(raw_j, raw_i, bins, offset: float = 127.5) -> caf.Surface:
    return winner_of(bins, sweep_bins(raw_j, raw_i, bins, offset))


class Worst(NamedTuple):
    peak: float          # largest relative error of a peak
    margin: float        # largest absolute error of a margin
    lag_margin: float    # smallest float64 lag margin of a compared cell
    cells: int


def assert_no_near_tie(want: caf.Surface, what=""):
    """The precondition of an exact lag comparison in EVERY cell (and of a meaningful margin_bin)."""
    low = min(r.margin for r in want.bins)
    assert low >= LAG_NEAR_TIE, f"{what}: a cell's lag margin {low} is under {LAG_NEAR_TIE}: not a usable case"
    return low


def hold(rec, ridge_lags, ridge_peaks, want: caf.Surface, what="") -> Worst:
    """One pair's record (lag, bin, peak, margin_lag, margin_bin attributes) and its ridge over the bins of
    ``want.bins`` against the float64 surface; no cell is left out."""
    low = assert_no_near_tie(want, what)
    assert (int(rec.lag), int(rec.bin)) == (want.lag, want.bin), f"{what}: got {(rec.lag, rec.bin)}, want {(want.lag, want.bin)}"
    want_peaks = np.array([r.peak for r in want.bins])
    got_peaks = np.asarray(ridge_peaks, np.float64)
    assert got_peaks.shape == want_peaks.shape and np.asarray(ridge_lags).shape == want_peaks.shape
    e_peak = max(abs(float(rec.peak) - want.peak) / want.peak, float(np.max(np.abs(got_peaks - want_peaks) / want_peaks)))
    e_margin = max(abs(float(rec.margin_lag) - want.margin_lag), abs(float(rec.margin_bin) - want.margin_bin))
    print(f"{what}: lag {rec.lag} bin {rec.bin} peak err {e_peak:.2e} (tol {PEAK_RTOL:g}) margin err {e_margin:.2e} "
          f"(tol {MARGIN_ATOL:g}); reference margins lag {want.margin_lag:.4f} bin {want.margin_bin:.4f}, smallest cell {low:.4f}")
    assert e_peak <= PEAK_RTOL, f"{what}: peak error {e_peak}"
    assert e_margin <= MARGIN_ATOL, f"{what}: margin error {e_margin}: got {rec.margin_lag}, {rec.margin_bin}"
    assert [int(x) for x in ridge_lags] == [r.lag for r in want.bins], f"{what}: ridge lags {list(ridge_lags)}"
    return Worst(e_peak, e_margin, low, len(want.bins))


# ------------------------------------------------------------------ 1: every FFT length, both bucket edges, edge bins
LENGTHS = [1 << p for p in range(16, 25)]
FULL_MAX_L = 1 << 21                         # up to here all nine edge bins at both n; above, thinned (the float64 reference)
#: the delay planted with the k-th edge bin: small, non-zero, of both signs, different from bin to bin
DELAYS = (3, -5, 7, -9, 11, -13, 15, -17, 19)


def edge_bins(L: int):
    """+-1 (bin -1: b mod L1 = L1 - 1, b div L1 = 4095 -- every row but the first carries and the rotation wraps to 0),
    the bins around one whole row of the shift, L1 - 1, L1, L1 + 1, -L1, -(L1 + 1), and the largest bins accepted."""
    L1 = L // ROW
    bins = [1, -1, L1 - 1, L1, L1 + 1, -L1, -(L1 + 1), L // 2 - 1, -(L // 2 - 1)]
    assert len(set(bins)) == 9
    return bins


class LengthCase(NamedTuple):
    L: int
    n: int
    bin: int         # the bin the offset is planted in
    delay: int
    thin: str        # "" or how the case's length is thinned

    @property
    def id(self):
        return f"L1={self.L // ROW}-n={self.n}{'-' + self.thin if self.thin else ''}-bin={self.bin}"

    @property
    def searched(self):
        """b - 1 .. b + 1, or b alone where a neighbour would leave (-L/2, L/2)."""
        b, half = self.bin, self.L // 2
        return [b - 1, b, b + 1] if -half < b - 1 and b + 1 < half else [b]


def length_cases():
    out = []
    for L in LENGTHS:
        L1, bins = L // ROW, edge_bins(L)
        delay = dict(zip(bins, DELAYS))
        if L <= FULL_MAX_L:
            out += [LengthCase(L, n, b, delay[b], "") for n in (L // 4 + 1, L // 2) for b in bins]
        else:
            # the float64 reference costs seconds per bin here: n = L/2 with three edge bins, and one bin at the lower
            # edge of the bucket so that both edges of every column kernel's lag mapping run
            out += [LengthCase(L, L // 2, b, delay[b], "thin3of9") for b in (L1 + 1, -1, L // 2 - 1)]
            out += [LengthCase(L, L // 4 + 1, -1, delay[-1], "thin1of9")]
    return out


LENGTH_CASES = length_cases()


def length_seed(L: int) -> int:
    return 1000 + L.bit_length() - 1


def length_capture(case: LengthCase):
    assert caf.fft_len(case.n) == case.L
    return caf.make_antennas(case.n, [(0, 0.0), (case.delay, float(case.bin))], length_seed(case.L))


def length_reference(case: LengthCase, raws) -> caf.Surface:
    """The float64 surface over the searched bins, with the case's preconditions asserted: the record is the planted
    (delay, bin), no cell is a near tie, and the runner-up bin stands at least GAP under the winner."""
    want = search_bins(raws[1], raws[0], case.searched)
    assert (want.lag, want.bin) == (case.delay, case.bin), (case.id, want[:5])
    assert all(r.lag == case.delay for r in want.bins), (case.id, [r.lag for r in want.bins])
    assert_no_near_tie(want, case.id)
    assert want.margin_bin >= GAP, (case.id, want.margin_bin)
    return want


# ------------------------------------------------------------------ 2: planted peaks under a bin
PLANT_N = [32768, (1 << 22) - 3]             # k5_check.K5_PLANT_N: L1 = 16 (L = 2n: a one-point padding band), L1 = 2048


def plant_bins(n: int):
    L1 = caf.fft_len(n) // ROW
    return [L1 + 1, -1]


# ------------------------------------------------------------------ 3: the bin clip
CLIP_N, CLIP_BINS = 1000, (-64, 129)
CLIP_WORDS = 688                             # include/gpsjam.h: a request is clipped to 688 / n_pairs


def clip_capture():
    return caf.make_antennas(CLIP_N, [(0, 0.0), (3, 20.0), (-4, -30.0)], seed=41)


# ------------------------------------------------------------------ 4: the largest call
BIG_N, BIG_FIRST, BIG_BINS = 1000, -2048, 4096           # n_bins = GJ_CAF_MAX_BINS
BIG_LAG, BIG_BIN = 3, 2040                                 # planted in the last batch of bins
#: the default batch at this shape: 128 MiB / (L x 8 bytes x 1 pair) = 256 bins, under the counters' 688 (k_xcorr.hip
#: caf_bins_per_launch) -- sixteen launches, and sixteen passes of the final pick's 256 threads over the 4096 records
BIG_BATCH = 256
BIG_TILE = 129                                             # bins per call of the calls that tile the range


def big_capture():
    """Low receiver noise: at n / L = 1000 / 65536 a neighbouring bin keeps 1 - 3.8e-4 of the peak, and the planted bin
    has to stay the winner in float64 and in float32 alike (asserted on the reference by the host test)."""
    return caf.make_antennas(BIG_N, [(0, 0.0), (BIG_LAG, float(BIG_BIN))], seed=43, sigma=1.0)


def big_subset():
    """At most 64 bins: both ends of the range, both sides of every batch seam, the winner's neighbourhood."""
    last = BIG_FIRST + BIG_BINS - 1
    s = {BIG_FIRST, last}
    for seam in range(BIG_FIRST + BIG_BATCH, last + 1, BIG_BATCH):
        s |= {seam - 1, seam}
    s |= {b for b in range(BIG_BIN - 3, BIG_BIN + 4) if b <= last}
    out = sorted(s)
    assert len(out) <= 64 and out[0] == BIG_FIRST and out[-1] == last
    return out


# ------------------------------------------------------------------ 5: slots and conventions at L1 = 64
SLOT_N = 100_000                                           # L = 2^18, L1 = 64: no slot test reaches it
SLOT_SPECS = [(0, 0.0), (4, 65.0), (-6, 1.0)]              # pairwise offsets 65 (L1 + 1), 1 and -64 (-L1)
SLOT_PAIRS = [(0, 1), (0, 2), (1, 2)]
SLOT_FIRST, SLOT_BINS = -66, 134                           # bins -66 .. 67
GNSSDEC = (128.0, 1.0 / 128.0)                             # gj_set_unpack's second documented convention


def slot_capture():
    return caf.make_antennas(SLOT_N, SLOT_SPECS, seed=47)


def slot_truth(pair):
    i, j = pair
    return SLOT_SPECS[j][0] - SLOT_SPECS[i][0], int(SLOT_SPECS[j][1] - SLOT_SPECS[i][1])


def slot_subset(pair):
    """The bins of a pair that the float64 reference evaluates (the GPU searches all 134): the ends of the range, the
    bins around 0 and around +-L1, and the neighbourhood of the pair's true bin, which holds the runner-up bin (at
    n / L = 0.38 a neighbouring bin keeps 0.78 of the peak, a bin three away 0.12)."""
    last = SLOT_FIRST + SLOT_BINS - 1
    tb = slot_truth(pair)[1]
    s = {SLOT_FIRST, last, -65, -64, -63, -1, 0, 1, 63, 64, 65} | set(range(tb - 2, tb + 3))
    return sorted(b for b in s if SLOT_FIRST <= b <= last)


def slot_reference(raws, pair, offset: float = 127.5) -> caf.Surface:
    i, j = pair
    bins = slot_subset(pair)
    want = search_bins(raws[j], raws[i], bins, offset)
    assert (want.lag, want.bin) == slot_truth(pair), (pair, want[:5])
    assert_no_near_tie(want, f"pair {pair}")
    return want
