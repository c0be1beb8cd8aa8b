"""The cross-ambiguity search (gj_xcorr_caf_dev) at every FFT length and at the edges of its shift, on the GPU.

This file sits in a package of its own for the reason tests/xcorr_caf/test_round6_gpu.py gives: the suite orders GPU
files by basename (tests/conftest.py SUITE_ORDER), and under the name test_round6_gpu.py it runs in stage 2, behind the
parity tests of K5.

What tests/xcorr_caf does not reach, and these do:
  1. caf_cols_kernel<L1> for all nine L1 = 16 .. 4096, each at both edges of its bucket (n = L/4 + 1 and n = L/2), under
     the bins at which caf_rows_kernel's shifted row and rotation change: +-1, L1 - 1, L1, L1 + 1, -L1, -(L1 + 1),
     +-(L/2 - 1) -- with the neighbouring bins searched too, so that margin_bin is a number (0.098 at n = L/4 + 1);
  2. peaks at the ends of the lag range, on both sides of a row and at the column kernels' tile edges, under a bin;
  3. a bins_per_launch request above what the arrival counters hold;
  4. n_bins = GJ_CAF_MAX_BINS: sixteen launches and sixteen passes of the pair's final pick;
  5. the slot and host-buffer entries at L1 = 64, and the search under gj_set_unpack(128, 1/128);
  6. the documented tie rule, on a pair whose |c| is exactly 0 everywhere.

Yardstick: caf_lengths_inputs.sweep_bins, the definition of include/gpsjam.h in float64, at the existing tolerances
(k5_check.PEAK_RTOL / MARGIN_ATOL = 1e-4, lags exact); tests/test_caf_lengths_host.py asserts what the inputs must be for
no cell to be left out, and every reference computed here is held to the same preconditions before the GPU's answer is
looked at.  Every call writes into sentinel-filled buffers.  Where a case takes seconds it is the float64 reference."""
import numpy as np
import pytest

import caf_lengths_inputs as ci
import caf_restatement as caf
import k5_check
from gpsjam import _ffi
from gpu_lib import LAG_INVALID, SENTINEL, ResidentSlices as Resident, as_k5, make_slots
from gpu_lib import caf_records as records

pytestmark = pytest.mark.gpu

P7 = caf.P7


def ridge(bl: bytes, bp: bytes, n_pairs: int, n_bins: int):
    return np.frombuffer(bl, np.int32).reshape(n_pairs, n_bins), np.frombuffer(bp, np.float32).reshape(n_pairs, n_bins)


def search(dev, raws, n, pairs, bin_first, n_bins, bpl=0):
    """One call into sentinel-filled buffers: the records and the ridge [n_pairs][n_bins]."""
    res = Resident(dev, raws, n, len(pairs), n_bins)
    try:
        res.fill(SENTINEL)
        res.caf(pairs, bin_first, n_bins, bpl=bpl)
        out, bl, bp = res.read()
    finally:
        res.close()
    recs = records(out)
    assert all(r.reserved == 0.0 for r in recs)                          # the record was written, to its last field
    return (recs,) + ridge(bl, bp, len(pairs), n_bins)


# ------------------------------------------------------------------ 1: every FFT length, non-zero bins
@pytest.mark.parametrize("case", ci.LENGTH_CASES, ids=[c.id for c in ci.LENGTH_CASES])
def test_every_fft_length_under_edge_bins(dev, case):
    raws = ci.length_capture(case)
    want = ci.length_reference(case, raws)                               # asserts the case's preconditions
    bins = case.searched
    recs, lags, peaks = search(dev, raws, case.n, [(0, 1)], bins[0], len(bins))
    ci.hold(recs[0], lags[0], peaks[0], want, case.id)
    if len(bins) == 1:
        assert recs[0].margin_bin == 1.0


# ------------------------------------------------------------------ 2: peaks at the ends of the lag range, under a bin
@pytest.mark.parametrize("which", [0, 1], ids=["bin=L1+1", "bin=-1"])
@pytest.mark.parametrize("n", ci.PLANT_N)
def test_peak_anywhere_in_the_lag_range_under_a_bin(dev, n, which):
    """K5's planted bursts (test_gpu_k5_check.k5_planted at k5_edge_lags) through the search's own copy of the lag mapping:
    a burst of at most 16 samples is turned by a nearly constant phase, so the bin's answer is still the planted lag."""
    b = ci.plant_bins(n)[which]
    rng = np.random.default_rng(n + b)
    worst = [0.0, 0.0]
    for lag in k5_check.k5_edge_lags(n):
        s0, s1 = k5_check.k5_planted(n, lag, rng, width=1 if abs(lag) >= n - 2 else None)
        Z0, Z1 = ci.spectrum(s0), ci.spectrum(s1)
        recs, lags, peaks = search(dev, [s0, s1], n, [(0, 1), (1, 0)], b, 1)
        for k, (ref, want_lag) in enumerate(((ci.bin_of_spectra(Z1, Z0, b, n), lag), (ci.bin_of_spectra(Z0, Z1, b, n), -lag))):
            assert ref.lag == want_lag and ref.margin > ci.GAP, (n, b, lag, ref)
            w = ci.hold(recs[k], lags[k], peaks[k], ci.winner_of([b], [ref]), f"n={n} bin={b} lag={want_lag} pair {(k, 1 - k)}")
            assert recs[k].margin_bin == 1.0
            worst = [max(worst[0], w.peak), max(worst[1], w.margin)]
    print(f"n={n} bin={b}: worst peak error {worst[0]:.2e} (tol {ci.PEAK_RTOL:g}), worst margin error {worst[1]:.2e} "
          f"(tol {ci.MARGIN_ATOL:g})")


# ------------------------------------------------------------------ 3: a request above the counters' capacity
def test_a_bins_per_launch_request_above_the_counters_capacity(dev):
    n, (first, nb) = ci.CLIP_N, ci.CLIP_BINS
    # first, on the host: were the clip gone, the launches below would count arrivals behind the 4-KiB sync area
    ws = lambda bpl: dev.xcorr_caf_workspace(3, n, len(P7), nb, bpl)
    assert ci.CLIP_WORDS // len(P7) == 98
    assert ws(4096) == ws(98) > ws(97)
    raws = ci.clip_capture()
    res = Resident(dev, raws, n, len(P7), nb)
    try:
        before = res.lags(P7)
        outs = []
        for bpl in (4096, 0, 1):                                         # launches of 98 + 31 bins; of 36; of 1
            res.fill(SENTINEL)
            res.caf(P7, first, nb, bpl=bpl)
            outs.append(res.read())
            assert res.lags(P7) == before, f"bins_per_launch {bpl}: an arrival counter was not left at zero"
        assert outs[0] == outs[1] == outs[2]
    finally:
        res.close()
    recs = records(outs[0][0])
    lags, peaks = ridge(outs[0][1], outs[0][2], len(P7), nb)
    assert all(r.lag != LAG_INVALID and first <= r.bin < first + nb and r.reserved == 0.0 for r in recs)
    # bin 0 of the ridge is K5, bit for bit, in every batching; the record's peak is its row's largest
    assert lags[:, -first].tobytes() == before[0] and peaks[:, -first].tobytes() == before[1]
    assert [r.peak for r in recs] == peaks.max(axis=1).tolist()
    assert [r.bin for r in recs] == (first + peaks.argmax(axis=1)).tolist()


# ------------------------------------------------------------------ 4: the largest call
def test_the_largest_call(dev):
    n, first, nb = ci.BIG_N, ci.BIG_FIRST, ci.BIG_BINS
    assert nb == _ffi.GJ_CAF_MAX_BINS
    raws = ci.big_capture()
    recs, lags, peaks = search(dev, raws, n, [(0, 1)], first, nb)
    subset = ci.big_subset()
    want = ci.search_bins(raws[1], raws[0], subset)
    idx = [b - first for b in subset]
    ci.hold(recs[0], lags[0, idx], peaks[0, idx], want, f"{nb} bins, {len(subset)} of them against float64")
    assert (recs[0].lag, recs[0].bin) == (ci.BIG_LAG, ci.BIG_BIN)
    # the whole ridge, byte for byte, against calls of 129 bins that tile the range (the last one holds 97)
    res = Resident(dev, raws, n, 1, ci.BIG_TILE)
    try:
        for t0 in range(0, nb, ci.BIG_TILE):
            k = min(ci.BIG_TILE, nb - t0)
            res.fill(SENTINEL)
            res.caf([(0, 1)], first + t0, k)
            out, bl, bp = res.read()
            assert bl[:4 * k] == lags[0, t0:t0 + k].tobytes() and bp[:4 * k] == peaks[0, t0:t0 + k].tobytes(), f"bins from {first + t0}"
            assert bl[4 * k:] == bp[4 * k:] == bytes([SENTINEL]) * (4 * (ci.BIG_TILE - k))
            tile = records(out)[0]
            assert tile.peak == peaks[0, t0:t0 + k].max() and tile.bin == first + t0 + int(peaks[0, t0:t0 + k].argmax())
    finally:
        res.close()
    assert recs[0].peak == peaks[0].max() and recs[0].bin == first + int(peaks[0].argmax())


# ------------------------------------------------------------------ 5: slots and conventions
def test_slots_and_conventions_at_l1_64(dev):
    n, pairs, first, nb = ci.SLOT_N, ci.SLOT_PAIRS, ci.SLOT_FIRST, ci.SLOT_BINS
    raws = ci.slot_capture()
    winners = {}
    try:
        for offset, scale in ((127.5, 1.0 / 127.5), ci.GNSSDEC):
            dev.set_unpack(offset, scale)
            res = Resident(dev, raws, n, len(pairs), nb)
            d_slots, sb = make_slots(dev, raws, n)
            try:
                res.fill(SENTINEL)
                res.caf(pairs, first, nb)
                got = res.read()
                res.fill(SENTINEL)
                dev.xcorr_caf_slots_dev(d_slots, sb, len(raws), n, pairs, first, nb, *res.bufs)
                assert res.read() == got, f"offset {offset}: the slot entry differs"
            finally:
                d_slots.free()
                res.close()
            recs = records(got[0])
            lags, peaks = ridge(got[1], got[2], len(pairs), nb)
            host, host_lags, host_peaks = dev.xcorr_caf(raws, pairs, bins=(first, nb), want_ridge=True)
            assert [(h.lag, h.bin, h.peak, h.margin_lag, h.margin_bin) for h in host] == \
                   [(r.lag, r.bin, r.peak, r.margin_lag, r.margin_bin) for r in recs]
            assert host_lags.tobytes() == got[1] and host_peaks.tobytes() == got[2]
            for k, p in enumerate(pairs):
                want = ci.slot_reference(raws, p, offset)
                idx = [b - first for b in ci.slot_subset(p)]
                ci.hold(recs[k], lags[k, idx], peaks[k, idx], want, f"offset {offset} pair {p}")
                winners[(offset, p)] = (recs[k].peak, want.peak)
    finally:
        dev.set_unpack()
    assert dev.get_unpack() == (127.5, 1.0 / 127.5)
    # the two conventions' peaks lie 3e-5 apart on this zero-mean capture -- inside PEAK_RTOL, but some thirty times the
    # float32 chain's error (18 butterfly layers of 6e-8): each answer is nearer the reference of its OWN convention
    for p in pairs:
        (g0, w0), (g1, w1) = winners[(127.5, p)], winners[(128.0, p)]
        print(f"pair {p}: peak {g0:.9g} / {g1:.9g}, float64 {w0:.9g} / {w1:.9g}")
        assert abs(g0 - w0) < abs(g0 - w1) and abs(g1 - w1) < abs(g1 - w0)


# ------------------------------------------------------------------ 6: the documented tie rule
@pytest.mark.parametrize("n", [1000, 1 << 20], ids=["L1=16", "L1=512"])
def test_the_tie_rule_on_a_pair_that_is_zero_everywhere(dev, n):
    """Bytes 128 under gj_set_unpack(128, 1/128) are the sample 0: every |c_b[m]| is exactly 0.  'The larger value, then
    the earlier bin of the range, then the smaller m' (include/gpsjam.h): the first bin, lag -(n - 1), peak and margins 0
    -- and K5 answers the same pair the same way, so bin 0 stays K5 bit for bit."""
    assert caf.fft_len(n) // 4096 == (16 if n == 1000 else 512)
    z = np.full(2 * n, 128, np.uint8)
    first, nb = -3, 7
    res = Resident(dev, [z, z], n, 1, nb)
    try:
        dev.set_unpack(*ci.GNSSDEC)
        res.fill(SENTINEL)
        res.caf([(0, 1)], first, nb)
        out, bl, bp = res.read()
        k5 = res.lags([(0, 1)])
        res.fill(SENTINEL)
        res.caf([(0, 1)], 0, 1)
        zero = res.read()
    finally:
        dev.set_unpack()
        res.close()
    r = records(out)[0]
    lags, peaks = ridge(bl, bp, 1, nb)
    print(f"n={n}: record {(r.lag, r.bin, r.peak, r.margin_lag, r.margin_bin)}, ridge lags {lags[0].tolist()} peaks {peaks[0].tolist()}")
    assert (r.lag, r.bin, r.peak, r.margin_lag, r.margin_bin, r.reserved) == (-(n - 1), first, 0.0, 0.0, 0.0, 0.0)
    assert lags[0].tolist() == [-(n - 1)] * nb and peaks[0].tolist() == [0.0] * nb
    want = ci.search_bins(z, z, list(range(first, first + nb)), offset=128.0)
    assert (want.lag, want.bin, want.peak, want.margin_lag, want.margin_bin) == (r.lag, r.bin, 0.0, 0.0, 0.0)
    # K5 on the same pair
    assert (np.frombuffer(k5[0], np.int32)[0], np.frombuffer(k5[1], np.float32)[0], np.frombuffer(k5[2], np.float32)[0]) == \
           (-(n - 1), 0.0, 0.0)
    assert as_k5(zero[0]) == k5 and records(zero[0])[0].bin == 0
    assert zero[1][:4] == k5[0] and zero[2][:4] == k5[1]
