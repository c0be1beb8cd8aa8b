"""The chirp-rate search (gj_chirp_dev, include/gpsjam.h) restated in float64 numpy, and the inputs of the chirp tests.
Not a test module: tests/test_chirp_host.py and tests/chirp/test_round6_gpu.py import it.

    x[t], w[n]  the ridge's (tests/ridge_restatement.py)
    m_r[n]  = (q_r n^2) mod 2 N^2          in integers
    c_r[n]  = exp(-i pi m_r[n] / N^2)
    Y_fr    = np.fft.fft(w * x[s_f : s_f + N] * c_r),   s_f = first_sample + f * hop,   q_r = first + r * step
    P_fr[k] = |Y_fr[k]|^2;  the record of frame f is the ridge's record of the r with the largest max_k P_fr[k]
              (equal values: the smallest r)

Every input is made here in numpy from a seed, quantised as tests/ridge_restatement.py does.  Nothing is derived from the
reference project.
"""
import functools
from typing import NamedTuple

import numpy as np

import ridge_restatement as rr

RECORD64 = np.dtype([("total", np.float64), ("peak", np.float64), ("second", np.float64), ("peak_bin", np.int32),
                     ("rate_index", np.int32)])

FS = rr.FS
NEAR_TIE = 1e-4             # no frame of any GPU input may beat its runner-up rate or bin by less
RTOL = 1e-5                 # the project's figure for a K2 value summed in another order (tests/test_gpu_parity.py)


class Scan(NamedTuple):
    records: np.ndarray     # RECORD64[n_frames]
    peaks: np.ndarray       # float64[n_frames][n_rates]
    rate_margin: np.ndarray  # 1 - (largest peak at any other rate) / peak; 1 with a single rate or without power
    bin_margin: np.ndarray   # at the best rate: 1 - (largest P at any other bin) / peak; 1 without power


def rate_values(rates):
    first, step, n = rates
    return [first + r * step for r in range(n)]


def dechirp(q, nfft, dtype=np.complex128):
    """c_r[n] with the phase reduced in integers: m / N^2 is an exact binary fraction in [0, 2)."""
    n = np.arange(nfft, dtype=np.int64)
    m = (int(q) * n * n) % (2 * nfft * nfft)          # |q| <= 2^23, n^2 < 2^24: inside int64
    return np.exp(-1j * np.pi * (m / float(nfft * nfft))).astype(dtype)


def dechirp_factors32(q, nfft):
    """c_r[n] as csrc/k_chirp.hip builds it, in complex64: with n = j + T s (T = nfft / 16, j < T, s < 16) the phase
    q n^2 = q j^2 + s (2 q j T) + s^2 (q T^2) gives (e8 d^(s-8)) * k_s; e8, d and k_s are rounded from their exact
    phases, d's powers come from up to eight complex64 products up and down from s = 8.  Returns (e8 d^(s-8), k_s) per n."""
    T, mod = nfft // 16, 2 * nfft * nfft
    unit = lambda m: np.exp(-1j * np.pi * ((m % mod) / float(nfft * nfft))).astype(np.complex64)
    j = np.arange(T, dtype=np.int64)
    pj, pd, pc = int(q) * j * j, int(q) * 2 * j * T, int(q) * T * T
    s = np.arange(16, dtype=np.int64)
    k = unit(pc * s * s)
    e = np.empty((16, T), np.complex64)
    e[8] = unit(pj + 8 * pd)
    up = unit(pd)
    down = np.conj(up)
    for i in range(9, 16):
        e[i] = e[i - 1] * up
    for i in range(7, -1, -1):
        e[i] = e[i + 1] * down
    return e.reshape(-1), np.repeat(k, T)                  # n = j + T s: slot-major


def chirp_scan_of(x, nfft, hop, rates, first_sample=0, n_frames=None, guard=2, single=False):
    """The definition on complex samples that are already unpacked.  ``single``: evaluate it in float32 / complex64
    (window, de-chirp as the kernel factors it, transform, powers and sums), the arithmetic a GPU kernel has, in numpy's
    order."""
    cplx, real = (np.complex64, np.float32) if single else (np.complex128, np.float64)
    x = np.asarray(x, np.complex128)
    if n_frames is None:
        n_frames = (x.size - first_sample - nfft) // hop + 1 if x.size - first_sample >= nfft else 0
    starts = first_sample + hop * np.arange(n_frames, dtype=np.int64)
    assert n_frames > 0 and starts[-1] + nfft <= x.size
    qs = rate_values(rates)
    assert qs and rates[1] >= 1 and all(abs(q) <= nfft * nfft // 2 for q in qs)
    k = np.arange(nfft)
    xw = (x[starts[:, None] + k[None, :]].astype(cplx) * rr.hann(nfft).astype(real)[None, :]).astype(cplx)
    rows = np.arange(n_frames)
    rec = np.zeros(n_frames, RECORD64)
    peaks = np.zeros((n_frames, len(qs)))
    bin_margin = np.ones(n_frames)
    for r, q in enumerate(qs):
        if single:
            e, kk = dechirp_factors32(q, nfft)
            y = np.fft.fft((xw * e[None, :]) * kk[None, :], axis=1)
        else:
            y = np.fft.fft(xw * dechirp(q, nfft)[None, :], axis=1)
        assert y.dtype == cplx
        p = np.abs(y) ** 2                                 # the ridge restatement's expression: rate 0 gives its bits
        pb = np.argmax(p, axis=1)                          # first maximum = smallest k
        peak = p[rows, pb]
        d = np.abs(k[None, :] - pb[:, None])
        d = np.minimum(d, nfft - d)
        second = np.where(d > guard, p, 0).max(axis=1)
        others = np.where(d > 0, p, -1).max(axis=1).astype(np.float64)
        peaks[:, r] = peak
        better = (peak > rec["peak"]) if r else np.ones(n_frames, bool)      # strictly greater: the smallest r among equals
        rec["total"][better], rec["peak"][better] = p.sum(axis=1)[better], peak[better]
        rec["second"][better], rec["peak_bin"][better], rec["rate_index"][better] = second[better], pb[better], r
        pk = peak.astype(np.float64)
        bin_margin[better] = np.where(pk > 0, 1.0 - others / np.where(pk > 0, pk, 1.0), 1.0)[better]
    rate_margin = np.ones(n_frames)
    if len(qs) > 1:
        rest = peaks.copy()
        rest[rows, rec["rate_index"]] = -1.0
        best = rec["peak"]
        rate_margin = np.where(best > 0, 1.0 - rest.max(axis=1) / np.where(best > 0, best, 1.0), 1.0)
    return Scan(rec, peaks, rate_margin, bin_margin)


def chirp_scan(raw, nfft, hop, rates, first_sample=0, n_frames=None, guard=2, offset=127.5, scale=1.0 / 127.5, single=False):
    return chirp_scan_of(rr.unpack(raw, offset, scale), nfft, hop, rates, first_sample, n_frames, guard, single)


# ---------------------------------------------------------------------------------------------------- inputs
def sawtooth(n, amp, sweep_hz_per_s, bw_hz, fs=FS, start=0.25):
    """A saw-tooth sweep -bw/2 .. +bw/2 at sweep_hz_per_s, beginning `start` of a period in."""
    t = np.arange(n) / fs
    f = -0.5 * bw_hz + bw_hz * ((t * sweep_hz_per_s / bw_hz + start) % 1.0)
    return amp * np.exp(2j * np.pi * np.cumsum(f) / fs)


PARITY_NFFT = (16, 32, 64, 1024, 2048, 4096)
PARITY_RATE = 1.3           # the sweep of parity_capture(nfft), in rate units AT THAT nfft: between two integers, off the half
# one seed per size, chosen so that no frame of any GPU case has a nearly tied rate or bin (tests/test_chirp_host.py asserts it)
PARITY_SEED = {16: 348, 32: 3, 64: 16, 256: 1, 1024: 1, 2048: 1, 4096: 2}


def parity_hop(nfft):
    return nfft // 2 + 37


def parity_frames(nfft):
    """Two full workgroup steps of 4096 / nfft frames, a part-filled third one and room for the translation test."""
    return 2 * (4096 // nfft) + 10


def parity_rate_sets(nfft):
    """The single rate 0, a grid around the sweep, and one set at each limit.  -N^2/2 and +N^2/2 are never in ONE set:
    rates N^2 apart give the same spectrum moved by N/2 bins (c differs by (-1)^n), an exact tie by construction."""
    half = nfft * nfft // 2
    return ((0, 1, 1), (-3, 2, 5), (-half, 3, 2), (half - 3, 3, 2))


@functools.lru_cache(maxsize=None)
def parity_capture(nfft):
    """parity_frames(nfft) frames at first sample 1 (at most 2^16 samples): noise, a continuous sweep of PARITY_RATE units
    (a discrete-time chirp wraps at the band edge without a seam, so every frame holds the same rate at another start
    frequency) and a short strong burst.  Read-only uint8."""
    n = 1 + (parity_frames(nfft) - 1) * parity_hop(nfft) + nfft
    assert n <= 1 << 16
    rng = np.random.default_rng(PARITY_SEED[nfft])
    t = np.arange(n, dtype=np.float64)
    z = rr._noise(rng, n, rr.NOISE_SIGMA).astype(np.complex128)
    z += 30.0 * np.exp(1j * np.pi * PARITY_RATE * (t / nfft) ** 2 + 2j * np.pi * 0.0371 * t)
    z[n // 2:n // 2 + 3 * nfft] += rr._noise(rng, 3 * nfft, 40.0)
    raw = rr.quantise(z)
    raw.setflags(write=False)
    return raw


@functools.lru_cache(maxsize=None)
def parity_reference(nfft, rates, first_sample, guard=2, offset=127.5, scale=1.0 / 127.5):
    """The restatement of parity_capture(nfft) at one rate set, every frame that fits, computed once and shared."""
    scan = chirp_scan(parity_capture(nfft), nfft, parity_hop(nfft), rates, first_sample, None, guard, offset, scale)
    for a in scan:
        a.setflags(write=False)
    return scan


# the classifier's cases: the ridge's five (tests/ridge_restatement.py) and the sweep the ridge cannot follow
CLASSIFIER_NFFT, CLASSIFIER_HOP = 256, 128
RATE_UNIT = (FS / CLASSIFIER_NFFT) ** 2                     # 64 MHz/s
FAST_SWEEP = 1.0e9                                          # Hz/s: 15.625 rate units, an eighth away from a half-integer
FAST_BW_HZ = 1.0e6                                          # a period of 1 ms = 16 frames of hop 128
FAST_SEED = 523
SWEPT_RATES = (-32, 1, 65)                                  # what tests/test_chirp_host.py scans


@functools.lru_cache(maxsize=None)
def fast_chirp_capture():
    """2^18 samples: the first half noise, the second half noise plus a saw-tooth that sweeps 1 MHz per millisecond."""
    rng = np.random.default_rng(FAST_SEED)
    n, h = rr.CLASSIFIER_SAMPLES, rr.CLASSIFIER_SAMPLES // 2
    z = rr._noise(rng, n, rr.NOISE_SIGMA).astype(np.complex128)
    z[h:] += sawtooth(h, 40.0, FAST_SWEEP, FAST_BW_HZ)
    raw = rr.quantise(z)
    raw.setflags(write=False)
    return raw


def classifier_capture(case):
    return fast_chirp_capture() if case == "fast chirp" else rr.classifier_capture(case)


WORST = {"total": 0.0, "peak": 0.0, "second": 0.0, "peaks": 0.0}   # largest error met so far, printed for the notes


def compare(got, peaks, want, what):
    rec = want.records
    assert got.size == rec.size, what
    np.testing.assert_array_equal(got["rate_index"], rec["rate_index"], err_msg=str(what))
    np.testing.assert_array_equal(got["peak_bin"], rec["peak_bin"], err_msg=str(what))
    for key in ("total", "peak"):
        err = np.max(np.abs(got[key] - rec[key]) / rec[key])
        WORST[key] = max(WORST[key], float(err))
        assert err <= RTOL, (what, key, err)
    err = np.max(np.abs(got["second"] - rec["second"]) / rec["peak"])
    WORST["second"] = max(WORST["second"], float(err))
    assert err <= RTOL, (what, "second", err)
    if peaks is not None:
        err = np.max(np.abs(peaks - want.peaks) / want.peaks)
        WORST["peaks"] = max(WORST["peaks"], float(err))
        assert err <= RTOL, (what, "peaks", err)
        rows = np.arange(got.size)
        assert np.array_equal(peaks[rows, got["rate_index"]], got["peak"]), what
