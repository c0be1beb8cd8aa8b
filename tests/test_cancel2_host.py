"""CPU side of the three-antenna per-bin canceller (gj_cancel2_dev) and of what is built on it (Device.cancel2,
coherence.spectral_matrix and cancel_weights2, mitigate.clean_spatial2 and its command line): the binding, the float64
restatement the GPU tests compare with (tests/cancel2_restatement.py) against a per-frame loop and its anchors, the
conditions the GPU tests rely on -- no power of any parity input near its threshold, few output values near a rounding
tie -- the weights, the call sequences of the Python layer on a host double of the library, and the end-to-end chain in
float64.  No GPU call is made."""
import ctypes as C

import numpy as np
import pytest

import cancel2_restatement as c2
import cancel_restatement as cr
import csd_restatement as cs
import excise_restatement as er
import gpsjam
import host_lib
from gpsjam import _ffi, coherence, mitigate

SIGNATURE = _ffi.SIGNATURES["gj_cancel2_dev"]        # without the binding nothing below has anything to restate

# ------------------------------------------------------------------------------------------------ C-ABI, host side
def test_signatures_and_interface():
    sz, i, vp = C.c_size_t, C.c_int, C.c_void_p
    assert SIGNATURE == (i, [vp, vp, sz, sz, vp, sz, sz, vp, sz, sz, sz, i, vp, sz, sz, vp, vp, vp])
    assert hasattr(_ffi.load(), "gj_cancel2_dev") and _ffi.GJ_VERSION == 150
    for name in ("cancel2", "cancel2_dev", "cancel", "cancel_dev"):
        assert callable(getattr(gpsjam.Device, name))
    assert callable(coherence.spectral_matrix) and callable(coherence.cancel_weights2) and callable(mitigate.clean_spatial2)
    assert mitigate.CleanedSpatial2._fields[:len(mitigate.CleanedSpatial._fields)] == mitigate.CleanedSpatial._fields
    assert mitigate.CleanedSpatial2._fields[-2:] == ("scan_c", "scan_bc")
    assert "--spatial2" in mitigate.__doc__ and "1 + |W1|^2 + |W2|^2" in mitigate.__doc__


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("nfft", (16, 64, 512))
def test_restatement_against_a_per_frame_loop(nfft):
    a, b, c = c2.parity_triple()
    n = 11 * nfft + nfft // 2 + 3                                  # 22 frames and a ragged tail
    w = c2.parity_weights(nfft)[:4]                                # four sets of five frames, the last one holds seven
    thr = c2.parity_threshold(nfft)
    for offset, scale in c2.CONVENTIONS:
        want_out, want_rec = c2.cancel2_loop(a, b, c, w, thr, nfft, 3, 8, 5, n, 5, offset, scale)
        got = c2.cancel2(a, b, c, w, thr, nfft, 3, 8, 5, n, 5, offset, scale)
        assert got.records.size == 22 == er.frames_loop(n, nfft) and np.array_equal(got.out, want_out)
        np.testing.assert_array_equal(got.records["n_excised"], want_rec["n_excised"])
        for key in ("total_in", "total", "removed"):
            np.testing.assert_allclose(got.records[key], want_rec[key], rtol=1e-12)
        assert got.records["n_excised"].any() and (got.lo, got.hi) == (nfft, 22 * nfft)
        assert np.array_equal(got.out[:got.lo], a[6:6 + nfft]) and np.array_equal(got.out[got.hi:], a[6 + got.hi:6 + 2 * n])


@pytest.mark.parametrize("nfft", (16, 256, 4096))
def test_restatement_anchors(nfft):
    a, b, c = c2.parity_triple()
    fa, fb, fc, n, fps = c2.PARITY_FIRST_A, c2.PARITY_FIRST_B, c2.PARITY_FIRST_C, c2.PARITY_SAMPLES, c2.PARITY_FRAMES_PER_SET
    thr, w = c2.parity_threshold(nfft), c2.parity_weights(nfft)
    same = lambda x, y: np.array_equal(x.out, y.out) and x.records.tobytes() == y.records.tobytes() and np.array_equal(x.value, y.value)
    for single in (False, True):
        # W2 = 0: the two-antenna canceller on (a, b) with W1, whatever c is
        w1 = w.copy()
        w1[:, 1] = 0
        ref = cr.cancel(a, b, w[:, 0], thr, nfft, fa, fb, n, fps, single=single)
        assert same(c2.cancel2(a, b, c, w1, thr, nfft, fa, fb, fc, n, fps, single=single), ref)
        assert same(c2.cancel2(a, b, a, w1, thr, nfft, fa, fb, 0, n, fps, single=single), ref)
        # W1 = 0: the two-antenna canceller on (a, c) with W2, whatever b is
        w2 = w.copy()
        w2[:, 0] = 0
        ref = cr.cancel(a, c, w[:, 1], thr, nfft, fa, fc, n, fps, single=single)
        assert same(c2.cancel2(a, b, c, w2, thr, nfft, fa, fb, fc, n, fps, single=single), ref)
        assert same(c2.cancel2(a, a, c, w2, thr, nfft, fa, 0, fc, n, fps, single=single), ref)
    # both zero: the excisor on capture a
    zero = c2.cancel2(a, b, c, np.zeros((2, nfft)), thr, nfft, fa, fb, fc, n)
    plain = er.excise(a, thr, nfft, fa, n)
    assert np.array_equal(zero.out, plain.out) and np.array_equal(zero.records["total"], plain.records["total"])
    assert np.array_equal(zero.records["total_in"], zero.records["total"]) and np.array_equal(zero.records["removed"], plain.records["removed"])
    # b = c = a with W1 = W2 = (0.5, 0): exactly nothing is left, and rint(127.5) = 128
    for single in (False, True):
        none = c2.cancel2(a, a, a, np.full((2, nfft), 0.5), None, nfft, fa, fa, fa, n, single=single)
        assert not none.records["total"].any() and np.all(none.out[none.lo:none.hi] == 128) and np.all(none.records["total_in"] > 0)
    # every threshold negative
    gone = c2.cancel2(a, b, c, w, np.full(nfft, -1.0), nfft, fa, fb, fc, n, fps)
    assert np.array_equal(gone.records["removed"], gone.records["total"]) and np.all(gone.records["n_excised"] == nfft)


def test_parity_inputs_keep_clear_of_thresholds_and_rounding_ties():
    """What the GPU parity test rests on, asserted on the restatement alone; re-measures E32."""
    a, b, c = c2.parity_triple()
    assert c.size == 2 * (c2.PARITY_FIRST_C + c2.PARITY_SAMPLES), "not a byte more"
    assert len({c2.PARITY_FIRST_A, c2.PARITY_FIRST_B, c2.PARITY_FIRST_C}) == 3 and c2.PARITY_FIRST_A % 2 == c2.PARITY_FIRST_C % 2 == 1
    assert (a, b) == cr.parity_pair() or (a is cr.parity_pair()[0] and b is cr.parity_pair()[1])
    worst_e32, worst_margin, worst_share = 0.0, np.inf, 0.0
    for nfft in c2.NFFT:
        for offset, scale in c2.CONVENTIONS:
            w = c2.parity_weights(nfft, offset)
            sets = c2.parity_sets(nfft)
            assert w.shape == (sets, 2, nfft) and w.dtype == np.complex64 and np.abs(w).max() <= 1.0
            assert w[0, 0, 3] == 1.0 and w[-1, 1, 3] == 0 and w[-1, 0, -2] == np.complex64(-0.6 + 0.3j) and w[0, 1, -2] == np.complex64(0.5 - 0.7j)
            assert np.count_nonzero(w[:, 0]) >= 0.9 * w[:, 0].size and np.count_nonzero(w[:, 1]) >= 0.9 * w[:, 1].size
            frames = er.frames_loop(c2.PARITY_SAMPLES, nfft)
            assert (sets - 1) * c2.PARITY_FRAMES_PER_SET < frames <= sets * c2.PARITY_FRAMES_PER_SET
            r64, r32 = c2.parity_reference(nfft, offset, scale), c2.parity_reference(nfft, offset, scale, single=True)
            margin = er.threshold_margin(r64.power, c2.parity_threshold(nfft, scale))
            share = float(np.mean(er.tie_distance(r64.value) <= c2.TIE_BAND))
            e32 = float(np.max(np.abs(r64.value - r32.value)))
            cut = int(r64.cut.sum())
            print(f"nfft {nfft} offset {offset}: margin {margin:.2e}, {cut} of {r64.cut.size} bins cut, tie share {share:.2e}, e32 {e32:.2e}")
            assert margin >= c2.NEAR_TIE, (nfft, offset, margin)
            assert share <= c2.TIE_SHARE_MAX, (nfft, offset, share)
            assert 0 < cut < r64.cut.size // 4 and np.array_equal(r32.cut, r64.cut)
            assert r64.records["total"].sum() < 0.5 * r64.records["total_in"].sum(), "the common source is taken out"
            worst_e32, worst_margin, worst_share = max(worst_e32, e32), min(worst_margin, margin), max(worst_share, share)
    print(f"smallest margin {worst_margin:.2e}, largest tie share {worst_share:.2e}, E32 {worst_e32!r} (recorded {c2.E32_MEASURED!r})")
    assert worst_e32 <= c2.E32 and abs(worst_e32 - c2.E32_MEASURED) <= 0.02 * c2.E32_MEASURED
    assert c2.E32 <= 1.02 * c2.E32_MEASURED, "E32 is the measured value rounded up"
    assert c2.TIE_BAND == 8 * c2.E32 and c2.TIE_SHARE_MAX == 0.002 and c2.NEAR_TIE == 1e-4


# ------------------------------------------------------------------------------------------------ the weights
def _matrix(saa, sbb, scc, sab, sac, sbc, nfft, m=8):
    f32 = lambda v: np.asarray(v, np.float32)
    msc = lambda sxx, syy, sxy: f32(np.abs(sxy) ** 2 / np.where(sxx * syy > 0, sxx * syy, np.nan))
    with np.errstate(invalid="ignore", divide="ignore"):
        return coherence.SpectralMatrix(cs.as_result(f32(saa), f32(sbb), np.complex64(sab), msc(saa, sbb, sab), nfft, nfft, m),
                                        cs.as_result(f32(saa), f32(scc), np.complex64(sac), msc(saa, scc, sac), nfft, nfft, m),
                                        cs.as_result(f32(sbb), f32(scc), np.complex64(sbc), msc(sbb, scc, sbc), nfft, nfft, m), (0, 0))


def _sums(A, B, Cc):
    """Saa, Sbb, Scc, Sab, Sac, Sbc of spectra [rows][frames][nfft], the project's convention Sxy = sum Y conj(X)."""
    p = lambda x: (np.abs(x) ** 2).sum(axis=1)
    x = lambda u, v: (v * np.conj(u)).sum(axis=1)
    return p(A), p(B), p(Cc), x(A, B), x(A, Cc), x(B, Cc)


def test_cancel_weights2():
    rows, m, nfft = 3, 6, 16
    rng = np.random.default_rng(9)
    z = lambda: rng.normal(size=(rows, m, nfft)) + 1j * rng.normal(size=(rows, m, nfft))
    B, Cc = z(), z()
    alpha = rng.normal(size=(rows, 1, nfft)) + 1j * rng.normal(size=(rows, 1, nfft))
    beta = rng.normal(size=(rows, 1, nfft)) + 1j * rng.normal(size=(rows, 1, nfft))
    A = alpha * B + beta * Cc                                       # exact: the solution is (alpha, beta)
    mat = _matrix(*_sums(A, B, Cc), nfft, m)
    flagged = np.ones((rows, nfft), bool)
    flagged[1, 4] = flagged[2, 0] = False
    w = coherence.cancel_weights2(mat, flagged)
    assert w.shape == (rows, 2, nfft) and w.dtype == np.complex64
    np.testing.assert_allclose(w[:, 0][flagged], alpha[:, 0][flagged], rtol=2e-5)      # the sums went through float32
    np.testing.assert_allclose(w[:, 1][flagged], beta[:, 0][flagged], rtol=2e-5)
    assert w[1, 0, 4] == w[1, 1, 4] == w[2, 0, 0] == w[2, 1, 0] == 0, "unflagged cells are exactly 0"
    one = coherence.cancel_weights2(mat, flagged.all(axis=0))      # flags per bin
    assert one.shape == (rows, 2, nfft) and not one[:, :, [0, 4]].any() and np.array_equal(one[:, :, 5], w[:, :, 5])
    with pytest.raises(ValueError):
        coherence.cancel_weights2(mat, np.ones((2, nfft), bool))
    # c is b: det = 0, the single weight of b (ties go to b), the other exactly 0
    saa, sbb, _, sab, _, _ = _sums(A, B, B)
    twin = coherence.cancel_weights2(_matrix(saa, sbb, sbb, sab, sab, sbb, nfft, m), np.ones((rows, nfft), bool))
    assert not twin[:, 1].any() and np.array_equal(twin[:, 0], (np.conj(np.complex64(sab).astype(np.complex128)) /
                                                                   np.float32(sbb).astype(np.float64)).astype(np.complex64))
    # alike enough to fall under the loading (here a large one): the auxiliary more coherent with a is taken, here c
    C2 = B + 0.3 * z()                                              # |rho_bc|^2 = 0.92: det = 0.08 Sbb Scc
    A2 = 0.7 * C2 + 0.01 * z()
    near = coherence.cancel_weights2(_matrix(*_sums(A2, B, C2), nfft, m), np.ones((rows, nfft), bool), loading=0.5)
    assert not near[:, 0].any() and np.all(np.abs(near[:, 1] - 0.7) < 0.05), "c alone, and b's weight exactly 0"
    assert np.all(coherence.cancel_weights2(_matrix(*_sums(A2, B, C2), nfft, m), np.ones((rows, nfft), bool)) != 0), "the default loading: solved"
    # zero and non-finite sums
    saa, sbb, scc, sab, sac, sbc = (v.copy() for v in _sums(A, B, Cc))
    sbb[0, 2], scc[0, 3] = 0.0, 0.0                                 # b unusable: c alone; c unusable: b alone
    sbb[0, 5] = scc[0, 5] = 0.0                                     # neither
    sab[1, 6] = np.nan                                              # b's sum is not finite: c alone
    sbc[1, 7] = np.inf                                              # det is not finite: the more coherent one
    got = coherence.cancel_weights2(_matrix(saa, sbb, scc, sab, sac, sbc, nfft, m), np.ones((rows, nfft), bool))
    assert np.all(np.isfinite(got.view(np.float32)))
    assert got[0, 0, 2] == 0 and got[0, 1, 2] == np.complex64(np.conj(np.complex64(sac[0, 2]).astype(np.complex128)) / np.float64(np.float32(scc[0, 2])))
    assert got[0, 1, 3] == 0 and got[0, 0, 3] != 0 and not got[0, :, 5].any()
    assert got[1, 0, 6] == 0 and got[1, 1, 6] != 0 and np.count_nonzero(got[1, :, 7]) == 1


def test_two_weights_leave_no_more_than_one():
    """The restated residual sum |A - W1 B - W2 C|^2 of the end-to-end triple's jammed row against both single-auxiliary
    residuals, cell by cell."""
    a, b, c = c2.e2e_triple(True)
    nfft, m = c2.E2E_NFFT, c2.E2E_FRAMES_PER_ROW
    row = 4
    spectra = [cs.frame_spectra(r, nfft, nfft, 0, row * m, m) for r in (a, b, c)]
    A, B, Cc = (s[None] for s in spectra)
    sums = _sums(A, B, Cc)
    mat = _matrix(*sums, nfft, m)
    w = coherence.cancel_weights2(mat, np.ones((1, nfft), bool)).astype(np.complex128)
    both = (np.abs(A[0] - w[0, 0] * B[0] - w[0, 1] * Cc[0]) ** 2).sum(axis=0)
    only_b = (np.abs(A[0] - np.conj(sums[3][0]) / sums[1][0] * B[0]) ** 2).sum(axis=0)
    only_c = (np.abs(A[0] - np.conj(sums[4][0]) / sums[2][0] * Cc[0]) ** 2).sum(axis=0)
    print(f"residual / Saa: both {both.sum() / sums[0].sum():.3f}, b alone {only_b.sum() / sums[0].sum():.3f}, c alone {only_c.sum() / sums[0].sum():.3f}")
    assert np.all(both <= only_b * (1 + 1e-5)) and np.all(both <= only_c * (1 + 1e-5))   # float32 weights and sums
    assert both.sum() < 0.25 * min(only_b.sum(), only_c.sum()), "two jammers: each single auxiliary is half blind"


# ------------------------------------------------------------------------------------------------ the Python layer
class HostLib(host_lib.HostLib):
    """gj_cancel2_dev, gj_cancel_dev and gj_csd_dev, which Device.cancel2, spectral_matrix and the chains reach, computed by
    the restatements on host memory (tests/host_lib.py); gj_excise_frames and gj_csd_rows are the real library's (pure
    host arithmetic)."""

    def gj_cancel2_dev(self, ctx, d_a, nbytes_a, first_a, d_b, nbytes_b, first_b, d_c, nbytes_c, first_c, n_samples, nfft, d_w,
                       frames_per_set, n_sets, d_thr, d_out, d_frames):
        self.calls.append(("cancel2", first_a, first_b, first_c, n_samples, nfft, frames_per_set, n_sets))
        assert d_w % 8 == 0 and d_thr % 4 == 0 and frames_per_set >= 1 and n_sets >= 1
        w = self.view(d_w, n_sets * 2 * nfft, np.complex64).reshape(n_sets, 2, nfft)
        got = c2.cancel2(self.view(d_a, nbytes_a), self.view(d_b, nbytes_b), self.view(d_c, nbytes_c), w,
                         self.view(d_thr, nfft, np.float32), nfft, first_a, first_b, first_c, n_samples, frames_per_set)
        self.view(d_out, 2 * n_samples)[:] = got.out
        if d_frames:
            rec = self.view(d_frames, got.records.size, gpsjam.CANCEL_DTYPE)
            for key in gpsjam.CANCEL_DTYPE.names:
                rec[key] = got.records[key]
        self.last = got
        return 0

    def gj_csd_dev(self, ctx, d_a, nbytes_a, first_a, d_b, nbytes_b, first_b, nfft, hop, frames_per_row, n_rows, d_saa, d_sbb, d_sab, d_msc):
        self.calls.append(("csd", first_a, first_b, nfft, hop, frames_per_row, n_rows))
        saa, sbb, sab, msc = cs.csd(self.view(d_a, nbytes_a), self.view(d_b, nbytes_b), nfft, hop, frames_per_row, first_a, first_b, n_rows)
        self.view(d_saa, n_rows * nfft, np.float32)[:] = saa.reshape(-1)
        self.view(d_sbb, n_rows * nfft, np.float32)[:] = sbb.reshape(-1)
        self.view(d_sab, n_rows * nfft, np.complex64)[:] = sab.reshape(-1)
        self.view(d_msc, n_rows * nfft, np.float32)[:] = msc.reshape(-1)
        return 0

    def gj_timer_start(self, ctx):
        return 0

    def gj_timer_stop(self, ctx, ref):
        ref._obj.value = 0.25
        return 0


@pytest.fixture
def host_dev():
    dev = host_lib.host_device(HostLib())
    yield dev
    dev._ctx = None            # a Capture that outlives the test frees nothing


W_NFFT, W_FA, W_FB, W_FC, W_N = 64, 3, 8, 5, 11 * 64 + 35           # 22 frames


def test_device_cancel2_on_the_host_double(host_dev):
    lib = host_dev._lib
    a, b, c = c2.parity_triple()
    w, thr = c2.parity_weights(W_NFFT)[:4], c2.parity_threshold(W_NFFT)
    want = c2.cancel2(a, b, c, w, thr, W_NFFT, W_FA, W_FB, W_FC, W_N, 5)
    n = 0
    for src_a, held_a in host_lib.sources(host_dev, a):
        for src_c, held_c in host_lib.sources(host_dev, c):
            n += 1
            lib.calls.clear()
            uploads = gpsjam.Capture.uploads
            cleaned, rec = host_dev.cancel2(src_a, b, src_c, w, thr, nfft=W_NFFT, first_a=W_FA, first_b=W_FB, first_c=W_FC, n_samples=W_N,
                                            frames_per_set=5)
            assert gpsjam.Capture.uploads == uploads + (src_a is a) + 1 + (src_c is c), "host bytes are uploaded once, a resident capture never"
            assert isinstance(cleaned, gpsjam.Capture) and cleaned.nbytes == 2 * W_N and rec.dtype == gpsjam.CANCEL_DTYPE and rec.size == 22
            assert np.array_equal(HostLib.view(cleaned.ptr, cleaned.nbytes), want.out)
            for key in gpsjam.CANCEL_DTYPE.names:
                assert np.array_equal(rec[key], want.records[key].astype(rec[key].dtype))
            # the threshold, the weights as float32 pairs (two per bin and set), the output, the records -- and one call
            assert host_lib.mallocs(lib) == [4 * W_NFFT, 8 * 2 * 4 * W_NFFT, 2 * W_N, 16 * 22]
            assert lib.calls[-1] == ("cancel2", W_FA, W_FB, W_FC, W_N, W_NFFT, 5, 4) and host_dev.kernel_calls == {"cancel2": n}
            assert set(lib.mem) == held_a | held_c | {cleaned.ptr}, "every buffer but the result is freed"
            cleaned.free()
    # the defaults: one set for every frame, no threshold (+inf: nothing is cut), what all three hold from sample 0; one
    # capture three times is uploaded once
    lib.calls.clear()
    uploads = gpsjam.Capture.uploads
    short = a[:2 * 300]
    cleaned, rec = host_dev.cancel2(short, short, short, np.full((2, W_NFFT), 0.5), nfft=W_NFFT)
    assert gpsjam.Capture.uploads == uploads + 1 and lib.calls[-1] == ("cancel2", 0, 0, 0, 300, W_NFFT, rec.size, 1) and rec.size == 8
    assert not rec["n_excised"].any() and not rec["total"].any() and np.all(HostLib.view(cleaned.ptr, 600)[W_NFFT:8 * W_NFFT] == 128)
    cleaned.free()
    cleaned, rec = host_dev.cancel2(a, b[:2 * 500], c, w[0], nfft=W_NFFT, first_a=1, first_b=4, first_c=7)
    assert lib.calls[-1] == ("cancel2", 1, 4, 7, 496, W_NFFT, gpsjam.excise_frames(496, W_NFFT), 1) and cleaned.nsamples == 496
    cleaned.free()
    assert not lib.mem
    # what the wrapper itself refuses, on the grounds cancel does
    for bad in (np.zeros(W_NFFT), np.zeros((2, W_NFFT + 1)), np.zeros((3, W_NFFT)), np.zeros((2, 3, 2, W_NFFT)), np.zeros((0, 2, W_NFFT))):
        with pytest.raises(ValueError, match="weights"):
            host_dev.cancel2(a, b, c, bad, nfft=W_NFFT)
    with pytest.raises(ValueError, match="frames_per_set"):
        host_dev.cancel2(a, b, c, w, nfft=W_NFFT)
    with pytest.raises(ValueError, match="threshold"):
        host_dev.cancel2(a, b, c, w[0], np.zeros(W_NFFT - 1), nfft=W_NFFT)
    assert not lib.mem and host_dev.kernel_calls == {"cancel2": 6}
    # a freed capture and the library's own refusal: nothing leaks
    host_lib.check_freed(host_dev, c, lambda cap: host_dev.cancel2(a, b, cap, w[0], nfft=W_NFFT))
    lib.refuse("gj_cancel2_dev")
    host_lib.check_refused(host_dev, c, lambda s: host_dev.cancel2(a, b, s, w[0], nfft=W_NFFT, n_samples=W_N), gpsjam.GpsJamError,
                           host_lib.REFUSED_TEXT, counted="cancel2")


S_NFFT, S_M = 64, 16                                                # rows of 16 frame triples of 64 points: 1024 samples


def _spatial_triple(jam_rows=(2, 3), rows=4, tail=200):
    """Independent noise in all three; in the given rows (the last one with the tail behind it) two independent wide-band
    sources, which b and c see turned by (1.0, 1.0 + pi / 3) and (-0.8, -0.8 - pi / 3) rad."""
    n = rows * S_NFFT * S_M + tail
    r = np.random.default_rng(12)
    za, zb, zc = (r.normal(0, 6.0, n) + 1j * r.normal(0, 6.0, n) for _ in range(3))
    on = np.zeros(n, bool)
    for row in jam_rows:
        on[row * S_NFFT * S_M:(n if row == rows - 1 else (row + 1) * S_NFFT * S_M)] = True
    for phase_b, phase_c in ((1.0, -0.8), (1.0 + np.pi / 3, -0.8 - np.pi / 3)):
        src = (r.normal(0, 25.0, n) + 1j * r.normal(0, 25.0, n)) * on
        za, zb, zc = za + src, zb + src * np.exp(1j * phase_b), zc + src * np.exp(1j * phase_c)
    out = []
    for z in (za, zb, zc):
        iq = np.empty(2 * n)
        iq[0::2], iq[1::2] = z.real, z.imag
        out.append((np.clip(np.round(iq), -128, 127) + 128).astype(np.uint8))
    return out


def test_clean_spatial2_on_the_host_double(host_dev):
    lib = host_dev._lib
    a, b, c = _spatial_triple()
    n = a.size // 2
    uploads = gpsjam.Capture.uploads
    res = mitigate.clean_spatial2(host_dev, a, b, c, nfft=S_NFFT, frames_per_row=S_M, p_fa=1e-4, lags=(0, 0))
    try:
        assert gpsjam.Capture.uploads == uploads + 3, "host bytes are uploaded once each"
        kinds = [k for k in lib.calls if k[0] != "malloc"]
        frames = gpsjam.excise_frames(n, S_NFFT)
        assert kinds == [("csd", 0, 0, S_NFFT, S_NFFT, S_M, 4)] * 3 + [("cancel2", 0, 0, 0, n, S_NFFT, 2 * S_M, 4)], \
            "three pair calls over the same rows at hop = nfft; a set per row, 2 M frames each"
        assert host_dev.kernel_calls == {"cross_spectrum": 3, "cancel2": 1} and frames == 2 * 4 * S_M + 5
        assert isinstance(res, mitigate.CleanedSpatial2) and res.cancelled and res.note == "" and res.capture.nsamples == n
        assert res.records.size == frames and res.weights.shape == (4, 2, S_NFFT) and res.weights.dtype == np.complex64
        # the weights are cancel_weights2 of the scans' own results, cell by cell: none in the quiet rows
        mat = coherence.SpectralMatrix(res.scan.result, res.scan_c.result, res.scan_bc.result, (0, 0))
        flagged = coherence.detect_cells(mat.ab, 1e-4).flagged | coherence.detect_cells(mat.ac, 1e-4).flagged
        assert np.array_equal(res.weights, coherence.cancel_weights2(mat, flagged)) and (res.scan.lag, res.scan_c.lag, res.scan_bc.lag) == (0, 0, 0)
        assert not res.weights[:2].any() and not res.weights[:, :, [0, 1, -1]].any(), "quiet rows and the DC guard: exactly 0"
        assert flagged[2:].sum() >= 2 * (S_NFFT - 3) * 0.9 and np.all(np.any(res.weights != 0, axis=1)[flagged])
        # rows 0 and 1 are excisor frames [0, 4 M): identity there (the last of them ends where row 2 begins)
        quiet = 2 * (2 * S_M * S_NFFT - S_NFFT)
        out = HostLib.view(res.capture.ptr, res.capture.nbytes)
        assert np.array_equal(out[:quiet], a[:quiet]) and not np.array_equal(out[quiet:], a[quiet:])
        # the leftover frames use the last set; the suppression is that of the frames with a weight in the band
        sets = cr.set_of(frames, 2 * S_M, 4)
        assert list(sets[-6:]) == [3] * 6 and len(res.bands) >= 1 and len(res.suppression_db) == len(res.bands)
        active = sets >= 2
        t_in, t_out = res.records["total_in"].astype(np.float64), res.records["total"].astype(np.float64)
        whole = max(range(len(res.bands)), key=lambda i: res.bands[i].n_bins)
        assert res.suppression_db[whole] == pytest.approx(10 * np.log10(t_in[active].sum() / t_out[active].sum()))
        # two sources of 1250 each in noise of 72, both nulled: what a single auxiliary leaves of the second source, about
        # half of it (3 dB of suppression), is gone too
        one = mitigate.clean_spatial(host_lib.host_device(_PairLib()), a, b, nfft=S_NFFT, frames_per_row=S_M, p_fa=1e-4, lag=0)
        print(f"suppression {res.suppression_db[whole]:.1f} dB with two auxiliaries, {max(one.suppression_db):.1f} dB with one")
        assert res.suppression_db[whole] > max(one.suppression_db) + 3.0
        assert sum(bd.n_bins for bd in res.bands) == int(np.any(res.weights != 0, axis=(0, 1)).sum())
    finally:
        res.capture.free()
    assert not lib.mem, "every buffer but the result is freed"
    # resident captures and integer lags: the triple is aligned first, and the result covers the aligned range
    lib.calls.clear()
    with gpsjam.Capture(host_dev, a) as ca, gpsjam.Capture(host_dev, b) as cb, gpsjam.Capture(host_dev, c) as cc:
        uploads = gpsjam.Capture.uploads
        shifted = mitigate.clean_spatial2(host_dev, ca, cb, cc, nfft=S_NFFT, frames_per_row=S_M, p_fa=1e-4, lags=(-2, 3),
                                          threshold=np.full(S_NFFT, 1e9))
        assert gpsjam.Capture.uploads == uploads
        kinds = [k for k in lib.calls if k[0] != "malloc"]
        assert [k[:3] for k in kinds[:3]] == [("csd", 2, 0), ("csd", 2, 5), ("csd", 0, 5)]
        assert kinds[3][:5] == ("cancel2", 2, 0, 5, n - 5) and (shifted.scan.lag, shifted.scan_c.lag, shifted.scan_bc.lag) == (-2, 3, 5)
        shifted.capture.free()


class _PairLib(HostLib):
    """The double with the two-antenna canceller, for the comparison with a single auxiliary."""

    def gj_cancel_dev(self, ctx, d_a, nbytes_a, first_a, d_b, nbytes_b, first_b, n_samples, nfft, d_w, frames_per_set, n_sets, d_thr,
                      d_out, d_frames):
        w = self.view(d_w, n_sets * nfft, np.complex64).reshape(n_sets, nfft)
        got = cr.cancel(self.view(d_a, nbytes_a), self.view(d_b, nbytes_b), w, self.view(d_thr, nfft, np.float32), nfft, first_a,
                        first_b, n_samples, frames_per_set)
        self.view(d_out, 2 * n_samples)[:] = got.out
        rec = self.view(d_frames, got.records.size, gpsjam.CANCEL_DTYPE)
        for key in gpsjam.CANCEL_DTYPE.names:
            rec[key] = got.records[key]
        return 0


class _CountingLib(_PairLib):
    """The double with every entry point that cross_spectrum, cancel, cancel2 and xcorr_fine reach, which also keeps the
    size of every upload in ``uploads``."""

    def __init__(self):
        super().__init__()
        self.uploads = []

    def gj_upload(self, ctx, data, nbytes, ref):
        self.uploads.append(int(nbytes))
        return super().gj_upload(ctx, data, nbytes, ref)

    def gj_xcorr_fine_dev(self, *args):                             # the sums are not what the test below reads
        return 0


def test_an_input_given_twice_is_resident_once():
    """Device._residents under the four wrappers that take several captures, at the smallest valid shape: the same object
    in every place is uploaded once and freed, equal but distinct arrays once each, a caller's Capture never uploaded and
    never freed, and a freed Capture in any place is the one ValueError with nothing allocated."""
    nfft, n = 16, 64
    dev = host_lib.host_device(_CountingLib())
    lib = dev._lib
    raw = c2.parity_triple()[0][:2 * n]
    twin = raw.copy()
    calls = {                                                       # name -> (captures it takes, the call)
        "cross_spectrum": (2, lambda x, y: dev.cross_spectrum(x, y, nfft=nfft, frames_per_row=2)),
        "cancel": (2, lambda x, y: dev.cancel(x, y, np.zeros(nfft), nfft=nfft)[0].free()),
        "cancel2": (3, lambda x, y, z: dev.cancel2(x, y, z, np.zeros((2, nfft)), nfft=nfft)[0].free()),
        "xcorr_fine": (2, lambda x, y: dev.xcorr_fine(x, y, half_width=2)),
    }
    for name, (places, call) in calls.items():
        lib.uploads.clear()
        call(*[raw] * places)
        assert lib.uploads == [2 * n] and not lib.mem, f"{name}: one object in every place is uploaded once, and freed"
        call(*[raw, twin, raw][:places])
        assert lib.uploads == [2 * n] * 3 and not lib.mem, f"{name}: equal but distinct arrays are uploaded once each"
        assert dev.kernel_calls[name] == 2
        with gpsjam.Capture(dev, raw) as cap:
            lib.uploads.clear()
            call(*[cap] * places)
            assert lib.uploads == [] and cap.ptr and set(lib.mem) == {cap.ptr}, f"{name}: a caller's capture is left alone"
            for k in range(places):
                host_lib.check_freed(dev, raw, lambda dead: call(*[dead if j == k else cap for j in range(places)]))
            assert lib.uploads == [2 * n] * places, "check_freed's own captures, and nothing else"
        assert not lib.mem
    dev._ctx = None


def test_clean_spatial2_with_nothing_flagged_returns_a_copy(host_dev):
    lib = host_dev._lib
    a, b, c = _spatial_triple(jam_rows=())
    res = mitigate.clean_spatial2(host_dev, a, b, c, nfft=S_NFFT, frames_per_row=S_M, lags=(0, 0))
    try:
        assert not res.cancelled and res.note == "nothing coherent was flagged: a copy of main" and res.bands == [] and res.suppression_db == []
        assert np.array_equal(HostLib.view(res.capture.ptr, res.capture.nbytes), a) and not res.weights.any()
        kinds = [k for k in lib.calls if k[0] != "malloc"]
        assert kinds[-1] == ("cancel2", 0, 0, 0, a.size // 2, S_NFFT, res.records.size, 1)
    finally:
        res.capture.free()
    # a capture shorter than a row: no row, nothing flagged, still a copy; shorter than a frame: refused
    short = mitigate.clean_spatial2(host_dev, a[:2 * 300], b[:2 * 300], c[:2 * 300], nfft=S_NFFT, frames_per_row=S_M, lags=(0, 0))
    assert not short.cancelled and len(short.scan.result) == 0 and np.array_equal(HostLib.view(short.capture.ptr, 600), a[:600])
    short.capture.free()
    with pytest.raises(ValueError, match="fewer than one frame"):
        mitigate.clean_spatial2(host_dev, a[:100], b[:100], c[:100], nfft=S_NFFT, frames_per_row=S_M, lags=(0, 0))
    assert not lib.mem


def test_command_line_takes_the_third_antenna(monkeypatch, tmp_path, capsys):
    """python -m gpsjam.mitigate A.bin OUT.bin --spatial B.bin --spatial2 C.bin on the host double."""
    a, b, c = _spatial_triple()
    pa, pb, pc, po = (str(tmp_path / name) for name in ("a.bin", "b.bin", "c.bin", "out.bin"))
    for raw, path in ((a, pa), (b, pb), (c, pc)):
        raw.tofile(path)

    double, other = host_lib.host_device(HostLib()), host_lib.host_device(HostLib())
    double.capture = lambda path: gpsjam.Capture(double, np.fromfile(path, np.uint8))

    class Dev:
        def __init__(self, index):
            assert index == 0

        def __enter__(self):
            return double

        def __exit__(self, *exc):
            pass
    monkeypatch.setattr(gpsjam, "Device", Dev)
    common = ["--nfft", str(S_NFFT), "--frames-per-row", str(S_M), "--p-fa", "1e-4", "--lag", "0"]
    assert mitigate.main([pa, po, "--spatial", pb, "--spatial2", pc] + common) == 0
    text = capsys.readouterr().out
    want = mitigate.clean_spatial2(other, a, b, c, nfft=S_NFFT, frames_per_row=S_M, p_fa=1e-4, lags=(0, 0))
    assert np.array_equal(np.fromfile(po, np.uint8), HostLib.view(want.capture.ptr, want.capture.nbytes))
    assert not double._lib.mem, "the command frees what it made"
    double._ctx = other._ctx = None
    assert "cancelled with two auxiliaries" in text and "suppression" in text and "aligned by 0 and 0" in text
    # --spatial2 without --spatial, and with another cleaner, is an error; nothing is written
    for bad in ([pa, po + ".x", "--spatial2", pc], [pa, po + ".x", "--spatial", pb, "--spatial2", pc, "--pulsed"],
                [pa, po + ".x", "--spatial", pb, "--spatial2", pc, "--lag", "k5", "--lag2", "1"]):
        with pytest.raises(SystemExit) as e:
            mitigate.main(bad)
        assert e.value.code != 0 and not (tmp_path / "out.bin.x").exists()
    assert "--spatial2 needs --spatial" in capsys.readouterr().err


# ------------------------------------------------------------------------------------------------ end to end
def test_end_to_end_on_the_cpu_gives_the_gpu_tests_tolerance():
    """The restated chain on c2.e2e_triple(): the three pairs' csd at hop = nfft, detect_cells, cancel_weights2, the
    canceller, C/N0 by the oracle's acquisition.  Asserts what the GPU test takes for granted -- raw, none acquires;
    jammer-free, all do; a single auxiliary brings back at most one -- and re-measures E2E_CPU_RESIDUAL_DB, which
    E2E_CN0_TOL_DB is twice of."""
    from oracle import gpsjam_oracle as orc
    free_a = c2.e2e_triple(False)[0]
    a, b, c = c2.e2e_triple(True)
    lead, nfft, m = er.E2E_LEAD, c2.E2E_NFFT, c2.E2E_FRAMES_PER_ROW
    assert a[:2 * lead].tobytes() == free_a[:2 * lead].tobytes() and a.size == b.size == c.size == 2 * (lead + er.E2E_AFTER)
    assert a.tobytes() != cr.e2e_pair(True)[0].tobytes() and free_a.tobytes() == cr.e2e_pair(False)[0].tobytes(), "main's noise and satellites are the pair's"
    clipped = float(np.mean((a == 0) | (a == 255)))
    print(f"clipped bytes of main: {100 * clipped:.3f} %")
    assert clipped < 0.001

    def acquire(raw):
        return [orc.acq_search(raw, lead, prn)[0] for prn, *_ in er.E2E_SATS]
    free, before = acquire(free_a), acquire(a)
    assert all(r["acquired"] for r in free) and not any(r["acquired"] for r in before)
    assert [r["codei"] for r in free] == [517, 1201, 88]
    pair = lambda x, y: cs.as_result(*cs.csd(x, y, nfft, nfft, m), nfft, nfft, m)
    mat = coherence.SpectralMatrix(pair(a, b), pair(a, c), pair(b, c), (0, 0))
    cells_b, cells_c = coherence.detect_cells(mat.ab, c2.E2E_P_FA), coherence.detect_cells(mat.ac, c2.E2E_P_FA)
    flagged = cells_b.flagged | cells_c.flagged
    msc = [float(np.median(r.msc[4])) for r in mat[:3]]
    print(f"median MSC of the jammed row: {msc[0]:.2f} (a,b), {msc[1]:.2f} (a,c), {msc[2]:.2f} (b,c); {int(flagged[4].sum())} of {nfft} bins flagged")
    assert len(mat.ab) == 5 and not flagged[:4].any() and flagged[4].sum() >= nfft - 8
    assert 0.35 < msc[0] < 0.55 and 0.35 < msc[1] < 0.55 and msc[2] < 0.1, "each auxiliary is half blind, and they share little"
    w = coherence.cancel_weights2(mat, flagged)
    w1, w2 = w[4, 0][flagged[4]], w[4, 1][flagged[4]]
    got = c2.cancel2(a, b, c, w, None, nfft, frames_per_set=2 * m)
    assert got.out[:2 * (lead - nfft)].tobytes() == a[:2 * (lead - nfft)].tobytes(), "the quiet lead-in comes back byte-identical"
    jam = c2.set_of(got.records.size, 2 * m, 5) == 4
    removed_db = lambda rec: float(10 * np.log10(rec["total_in"][jam].sum() / rec["total"][jam].sum()))
    # a single auxiliary: one null per bin fits one of the two jammers
    for name, aux, result, cells in (("b", b, mat.ab, cells_b), ("c", c, mat.ac, cells_c)):
        one = cr.cancel(a, aux, coherence.cancel_weights(result, cells), None, nfft, frames_per_set=2 * m)
        back = sum(r["acquired"] for r in acquire(one.out))
        print(f"auxiliary {name} alone: {removed_db(one.records):.2f} dB removed, {back} of 3 acquired")
        assert back <= 1 and removed_db(one.records) < 4.0
    print(f"both: {removed_db(got.records):.2f} dB removed, median |W1| {np.median(np.abs(w1)):.3f}, |W2| {np.median(np.abs(w2)):.3f}")
    assert removed_db(got.records) > 8.0
    worst = 0.0
    for (prn, *_), (psi_b, psi_c), r, f, j in zip(er.E2E_SATS, c2.E2E_SAT_PHASE, acquire(got.out), free, before):
        predicted = c2.e2e_predicted_db(w1, w2, psi_b, psi_c)
        resid = r["cn0"] - (f["cn0"] + predicted)
        worst = max(worst, abs(resid))
        print(f"PRN {prn}: C/N0 {f['cn0']:.2f} jammer-free, {j['cn0']:.2f} jammed, {r['cn0']:.2f} cancelled; the weights predict "
              f"{predicted:+.2f} dB, residual {resid:+.3f} dB")
        assert r["acquired"] and r["codei"] == f["codei"] and abs(r["freqi"] - f["freqi"]) <= 1
    print(f"worst residual {worst:.3f} dB (recorded {c2.E2E_CPU_RESIDUAL_MEASURED}), tolerance {c2.E2E_CN0_TOL_DB} dB")
    assert worst <= c2.E2E_CPU_RESIDUAL_DB and abs(worst - c2.E2E_CPU_RESIDUAL_MEASURED) < 0.005
    assert c2.E2E_CN0_TOL_DB == 2.0 * c2.E2E_CPU_RESIDUAL_DB
