"""The cross-ambiguity search (gj_xcorr_caf_dev / _slots_dev / _u8, Device.xcorr_caf, triangulateTDOA.correlation_lag_offset)
on the GPU.

This file sits in a package of its own on purpose: the suite orders GPU files by basename (tests/conftest.py
SUITE_ORDER), and under the name test_round6_gpu.py it runs in stage 2, behind the parity tests of K5 it builds on.

Yardsticks: bin 0 must BE K5 (byte for byte); every other bin is compared with the numpy / scipy restatement of the
definition in include/gpsjam.h (tests/caf_restatement.py).  Tolerances: peaks 1e-4 relative (K5's own gate in
tests/test_gpu_parity.py), margins 1e-4 absolute, lags exact wherever the restatement's own decision margin is at
least LAG_NEAR_TIE = 2e-5 (the band inside which two complex64 FFTs may order two lags differently)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import caf_restatement as caf
import gpsjam
from gpsjam import _ffi
from gpu_lib import CAF_REC as REC
from gpu_lib import GJ_ERR_INVALID, GJ_ERR_UNSUPPORTED, LAG_INVALID as INVALID, ResidentSlices as Resident, as_k5, make_slots
from gpu_lib import caf_records as records

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SKRYPTY = os.path.join(os.path.dirname(os.path.dirname(HERE)), "gps-jamming_amd", "skrypty")
if SKRYPTY not in sys.path:
    sys.path.insert(0, SKRYPTY)

P3, P7 = caf.P3, caf.P7
FIRST, NBINS = caf.BINS_REF


# ------------------------------------------------------------------ 4: bin 0 is K5
@pytest.mark.parametrize("n", [50000, 1 << 19])
@pytest.mark.parametrize("pairs", [P3, P7], ids=["few_pairs", "many_pairs"])
def test_bin_zero_is_k5_byte_for_byte(dev, n, pairs):
    raws = caf.make_antennas(n, [(0, 0.0), (4, 0.3), (-6, -0.2)], seed=7)
    res = Resident(dev, raws, n, len(pairs), 1)
    want = res.lags(pairs)
    res.fill()
    dev.reserve(dev.xcorr_caf_workspace(3, n, len(pairs), 1))
    res.caf(pairs, 0, 1)
    out, bl, bp = res.read()
    assert as_k5(out) == want
    assert bl == want[0] and bp == want[1]                       # the ridge of a one-bin search is the answer itself
    assert all(r.bin == 0 and r.margin_bin == 1.0 and r.reserved == 0.0 for r in records(out))
    # through slots
    d_slots, sb = make_slots(dev, raws, n)
    dev.xcorr_slots_dev(d_slots, sb, 3, n, pairs, *res.k5)
    dev.synchronize()
    want_slots = tuple(b.download(np.uint8, 4 * len(pairs)).tobytes() for b in res.k5)
    assert want_slots == want
    res.fill()
    dev.xcorr_caf_slots_dev(d_slots, sb, 3, n, pairs, 0, 1, *res.bufs)
    assert as_k5(res.read()[0]) == want
    d_slots.free()
    # through the host-buffer entry point
    l, p, m = dev.xcorr_lags(raws, pairs, want_margins=True)
    got = dev.xcorr_caf(raws, pairs)
    assert (np.array([r.lag for r in got], np.int32).tobytes(), np.array([r.peak for r in got], np.float32).tobytes(),
            np.array([r.margin_lag for r in got], np.float32).tobytes()) == (l.tobytes(), p.tobytes(), m.tobytes()) == want
    res.close()


# ------------------------------------------------------------------ 5: against the restatement
@pytest.mark.parametrize("case", range(len(caf.CASES)))
def test_search_matches_the_restatement(dev, case):
    n = caf.N_REF
    specs = [(0, 0.0), caf.CASES[case], caf.THIRD[case]]
    raws = caf.make_antennas(n, specs, seed=200 + case)
    got, ridge_lags, ridge_peaks = dev.xcorr_caf(raws, P3, bins=(FIRST, NBINS), want_ridge=True)
    assert ridge_lags.shape == ridge_peaks.shape == (3, NBINS)
    cells = skipped = 0
    for k, (i, j) in enumerate(P3):
        want = caf.search(raws[j], raws[i], FIRST, NBINS)
        true_lag, true_bin = specs[j][0] - specs[i][0], int(round(specs[j][1] - specs[i][1]))
        print(f"case {case} pair {(i, j)}: got {got[k]} want {want[:5]} truth {(true_lag, true_bin)}")
        assert (want.lag, want.bin) == (true_lag, true_bin)
        assert (got[k].lag, got[k].bin) == (want.lag, want.bin)
        assert got[k].offset_hz == want.bin * 2.048e6 / caf.fft_len(n)
        np.testing.assert_allclose(got[k].peak, want.peak, rtol=1e-4)
        assert abs(got[k].margin_lag - want.margin_lag) <= 1e-4 and abs(got[k].margin_bin - want.margin_bin) <= 1e-4
        np.testing.assert_allclose(ridge_peaks[k], [r.peak for r in want.bins], rtol=1e-4)
        for b, r in enumerate(want.bins):
            cells += 1
            if r.margin >= caf.LAG_NEAR_TIE:
                assert ridge_lags[k, b] == r.lag, (case, (i, j), FIRST + b, int(ridge_lags[k, b]), r)
            else:
                skipped += 1
    assert cells == 3 * NBINS and skipped <= 0.02 * cells, (skipped, cells)


# ------------------------------------------------------------------ 6: the shift across rows and its carry
def check_single_bins(dev, n, bins, seed):
    L = caf.fft_len(n)
    for b in bins:
        raws = caf.make_antennas(n, [(0, 0.0), (5, float(b))], seed=seed)
        got = dev.xcorr_caf(raws, [(0, 1)], bins=(b, 1))[0]
        want = caf.direct_bin(raws[1], raws[0], b)
        print(f"n {n} L {L} bin {b}: got lag {got.lag} peak {got.peak:.6g}, want {want}")
        assert got.bin == b and got.lag == want.lag == 5, (b, got, want)
        np.testing.assert_allclose(got.peak, want.peak, rtol=1e-4)
        assert got.margin_bin == 1.0


def test_shift_and_carry_small_l1(dev):
    L = caf.fft_len(1000)
    assert L == 65536                                                     # L1 = 16
    check_single_bins(dev, 1000, [-17, -16, -1, 0, 1, 15, 16, 17, 4095, -28672, L // 2 - 1, -(L // 2 - 1)], seed=31)


def test_shift_and_carry_large_l1(dev):
    assert caf.fft_len(1 << 19) == 1 << 20                               # L1 = 256
    check_single_bins(dev, 1 << 19, [-257, -256, 255, 256, 257], seed=32)


# ------------------------------------------------------------------ 7: batching
def test_results_do_not_depend_on_the_batch_size(dev):
    n = caf.N_REF
    raws = caf.make_antennas(n, [(0, 0.0), caf.CASES[0], caf.THIRD[0]], seed=200)
    res = Resident(dev, raws, n, 3, NBINS)
    outs = []
    for bpl in (0, 1, 7):
        res.fill()
        res.caf(P3, FIRST, NBINS, bpl=bpl)
        outs.append(res.read())
    assert outs[0] == outs[1] == outs[2]
    assert [(r.lag, r.bin) for r in records(outs[0][0])] == [(37, 21), (-11, -14), (-48, -35)]
    res.close()


# ------------------------------------------------------------------ 8: invalid antennas
def test_invalid_antenna_invalidates_its_pairs_only(dev):
    n = caf.N_REF
    raws = caf.make_antennas(n, [(0, 0.0), caf.CASES[0], caf.THIRD[0]], seed=200)
    nb = 9
    good = Resident(dev, raws, n, 3, nb)
    good.caf(P3, -16, nb)
    want = good.read()
    good.close()
    want_rec = records(want[0])
    for starts in ([0, -1, 0], [0, 1, 0]):                                # negative start; slice runs off the end
        res = Resident(dev, raws, n, 3, nb, starts=starts)
        res.fill()
        res.caf(P3, -16, nb)
        out, bl, bp = res.read()
        rec = records(out)
        for k in (0, 2):
            assert (rec[k].lag, rec[k].bin, rec[k].peak, rec[k].margin_lag, rec[k].margin_bin) == (INVALID, 0, 0.0, 0.0, 0.0)
        assert out[REC:2 * REC] == want[0][REC:2 * REC] and want_rec[1].lag == -11
        lags = np.frombuffer(bl, np.int32).reshape(3, nb)
        peaks = np.frombuffer(bp, np.float32).reshape(3, nb)
        assert (lags[[0, 2]] == INVALID).all() and (peaks[[0, 2]] == 0).all()
        assert bl[4 * nb:8 * nb] == want[1][4 * nb:8 * nb] and bp[4 * nb:8 * nb] == want[2][4 * nb:8 * nb]
        res.close()
    # the same through slots: flag -1
    d_slots, sb = make_slots(dev, raws, n, flags=[0, -1, 0])
    bufs = [dev.alloc(REC * 3), dev.alloc(4 * 3 * nb), dev.alloc(4 * 3 * nb)]
    dev.xcorr_caf_slots_dev(d_slots, sb, 3, n, P3, -16, nb, *bufs)
    dev.synchronize()
    out = bufs[0].download(np.uint8).tobytes()
    rec = records(out)
    assert rec[0].lag == INVALID and rec[2].lag == INVALID and out[REC:2 * REC] == want[0][REC:2 * REC]
    assert bufs[1].download(np.uint8).tobytes()[4 * nb:8 * nb] == want[1][4 * nb:8 * nb]
    for x in bufs + [d_slots]:
        x.free()


# ------------------------------------------------------------------ 9: refusals
def test_refused_calls_enqueue_nothing(dev):
    n = caf.N_REF
    L = caf.fft_len(n)
    raws = caf.make_antennas(n, [(0, 0.0), caf.CASES[0], caf.THIRD[0]], seed=200)
    res = Resident(dev, raws, n, 3, 4)
    res.fill()
    sentinel = res.read()
    lib, ctx = dev._lib, dev._ctx
    ptrs = (C.c_void_p * 17)(*([c.ptr for c in res.caps] + [res.caps[0].ptr] * 14))
    sizes = (C.c_size_t * 17)(*([c.nbytes for c in res.caps] + [res.caps[0].nbytes] * 14))
    d_starts17 = dev.alloc(8 * 17).upload(np.zeros(17, np.int64))
    many = np.zeros(2 * 200, np.int32)
    flat = np.array(P3, np.int32).reshape(-1)

    def call(n_ant=3, n_samples=n, pairs=flat, n_pairs=3, bin_first=0, n_bins=1, bpl=0):
        return lib.gj_xcorr_caf_dev(ctx, ptrs, sizes, n_ant, d_starts17.ptr, n_samples, pairs.ctypes.data_as(C.POINTER(C.c_int32)),
                                    n_pairs, bin_first, n_bins, bpl, res.bufs[0].ptr, res.bufs[1].ptr, res.bufs[2].ptr)

    assert call(n_bins=0) == GJ_ERR_INVALID
    assert call(n_bins=-3) == GJ_ERR_INVALID
    assert call(bin_first=L // 2) == GJ_ERR_INVALID
    assert call(bin_first=-(L // 2)) == GJ_ERR_INVALID
    assert call(bin_first=L // 2 - 2, n_bins=3) == GJ_ERR_INVALID          # the LAST bin is out of range
    assert call(n_pairs=0) == GJ_ERR_INVALID
    assert call(pairs=many, n_pairs=137) == GJ_ERR_INVALID                  # GJ_MAX_ANTENNAS^2 / 2 + 8 = 136 is the most
    assert call(n_ant=0) == GJ_ERR_INVALID
    assert call(n_ant=17) == GJ_ERR_INVALID
    assert call(pairs=np.array([0, 3], np.int32), n_pairs=1) == GJ_ERR_INVALID
    assert call(bpl=-1) == GJ_ERR_INVALID
    assert call(n_samples=(1 << 23) + 1) == GJ_ERR_UNSUPPORTED
    assert call(bin_first=-2048, n_bins=_ffi.GJ_CAF_MAX_BINS + 1) == GJ_ERR_UNSUPPORTED
    with pytest.raises(gpsjam.GpsJamError):
        dev.xcorr_caf(raws, P3, bins=(0, 0))
    assert res.read() == sentinel
    # the context still works, and the largest bins are accepted
    assert call(bin_first=L // 2 - 1) == 0 and call(bin_first=-(L // 2 - 1)) == 0
    assert call(bin_first=-1, n_bins=4) == 0
    out = res.read()
    assert all(-1 <= r.bin <= 2 and r.lag != INVALID for r in records(out[0]))
    d_starts17.free()
    res.close()


# ------------------------------------------------------------------ 10: back to back, counters back at zero
def test_twenty_calls_back_to_back_leave_the_counters_at_zero(dev):
    n = caf.N_REF
    raws = caf.make_antennas(n, [(0, 0.0), caf.CASES[0], caf.THIRD[0]], seed=200)
    nb = 17
    res = Resident(dev, raws, n, 3, nb)
    before = res.lags(P3)
    dev.reserve(dev.xcorr_caf_workspace(3, n, 3, nb, 5))
    sets = [[dev.alloc(s) for s, _ in res.sizes] for _ in range(20)]
    for bufs in sets:
        res.caf(P3, 13, nb, bpl=5, bufs=bufs)                             # four launches of bins each, no synchronisation
    dev.synchronize()
    outs = [tuple(b.download(np.uint8).tobytes() for b in bufs) for bufs in sets]
    assert all(o == outs[0] for o in outs)
    assert [(r.lag, r.bin) for r in records(outs[0][0])][0] == (37, 21)
    assert res.lags(P3) == before
    res.caf(P3, 13, nb)
    assert res.read() == outs[0]
    for bufs in sets:
        for b in bufs:
            b.free()
    res.close()


# ------------------------------------------------------------------ 11: the drop-in
def test_dropin_finds_lag_and_offset_where_the_plain_call_fails(tmp_path, monkeypatch):
    import triangulateTDOA as tdoa
    monkeypatch.setattr(gpsjam, "_default", None)
    n = tdoa.CORRELATION_SLICE_SIZE
    assert n == caf.N_REF
    raws = caf.make_antennas(n, [(0, 0.0), (37, 21.0)], seed=100)
    caps = []
    for k, r in enumerate(raws):
        path = tmp_path / f"ant{k}.bin"
        r.tofile(path)
        caps.append(tdoa.load_iq_data(str(path)))
    lag, peak, offset_hz = tdoa.correlation_lag_offset(caps[1][0:n], caps[0][0:n], 1000.0)
    assert lag == 37 and offset_hz == 21 * tdoa.SAMPLE_RATE / gpsjam.xcorr_fft_len(n) == 328.125
    np.testing.assert_allclose(peak, caf.direct_bin(raws[1], raws[0], 21).peak, rtol=1e-4)
    plain, plain_peak = tdoa.correlation_lag(caps[1][0:n], caps[0][0:n])
    assert plain != 37 and plain == caf.plain_lag(raws[1], raws[0]) and peak > 30 * plain_peak
    assert tdoa.FREQ_SEARCH_HZ == 0.0
    gpsjam.default_device().close()
    monkeypatch.setattr(gpsjam, "_default", None)
