"""CPU side of the two-antenna per-bin canceller (gj_cancel_dev) and of what is built on it (Device.cancel,
coherence.cancel_weights, mitigate.clean_spatial): the binding, the float64 restatement the GPU tests compare with
(tests/cancel_restatement.py) against a per-frame loop and its anchors, the conditions the GPU tests rely on -- no power
of any parity input near its threshold, few output values near a rounding tie -- the weights, the call sequences of the
Python layer on a host double of the library, and the end-to-end chain in float64.  No GPU call is made."""
import ctypes as C

import numpy as np
import pytest

import cancel_restatement as cr
import csd_restatement as cs
import excise_restatement as er
import gpsjam
import host_lib
from gpsjam import _ffi, coherence, mitigate


# ------------------------------------------------------------------------------------------------ C-ABI, host side
def test_signatures_and_layout():
    sz, i, vp = C.c_size_t, C.c_int, C.c_void_p
    assert _ffi.SIGNATURES["gj_cancel_dev"] == (i, [vp, vp, sz, sz, vp, sz, sz, sz, i, vp, sz, sz, vp, vp, vp])
    assert hasattr(_ffi.load(), "gj_cancel_dev") and _ffi.GJ_VERSION == 150
    assert C.sizeof(_ffi.CancelFrame) == gpsjam.CANCEL_DTYPE.itemsize == 16
    assert [(n, gpsjam.CANCEL_DTYPE.fields[n][1]) for n in gpsjam.CANCEL_DTYPE.names] == \
        [("total_in", 0), ("total", 4), ("removed", 8), ("n_excised", 12)]
    assert [f[0] for f in _ffi.CancelFrame._fields_] == list(gpsjam.CANCEL_DTYPE.names)


def test_python_interface_is_there():
    for name in ("cancel", "cancel_dev"):
        assert callable(getattr(gpsjam.Device, name))
    assert callable(coherence.cancel_weights) and callable(coherence.detect_cells) and callable(mitigate.clean_spatial)
    assert "CANCEL_DTYPE" in gpsjam.__all__
    assert mitigate.CleanedSpatial._fields == ("capture", "records", "weights", "scan", "bands", "suppression_db", "cancelled", "note")
    assert "one null per bin" in mitigate.__doc__ and "1 + |W|^2" in mitigate.__doc__ and "--spatial" in mitigate.__doc__


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("nfft", (16, 64, 512))
def test_restatement_against_a_per_frame_loop(nfft):
    a, b = cr.parity_pair()
    n = 11 * nfft + nfft // 2 + 3                                  # 22 frames and a ragged tail
    w = cr.parity_weights(nfft)[:4]                                # four sets of five frames, the last one holds seven
    thr = cr.parity_threshold(nfft)
    for offset, scale in cr.CONVENTIONS:
        want_out, want_rec = cr.cancel_loop(a, b, w, thr, nfft, 3, 8, n, 5, offset, scale)
        got = cr.cancel(a, b, w, thr, nfft, 3, 8, n, 5, offset, scale)
        assert got.records.size == 22 == er.frames_loop(n, nfft) and np.array_equal(got.out, want_out)
        np.testing.assert_array_equal(got.records["n_excised"], want_rec["n_excised"])
        for key in ("total_in", "total", "removed"):
            np.testing.assert_allclose(got.records[key], want_rec[key], rtol=1e-12)
        assert got.records["n_excised"].any() and (got.lo, got.hi) == (nfft, 22 * nfft)
        assert np.array_equal(got.out[:got.lo], a[6:6 + nfft]) and np.array_equal(got.out[got.hi:], a[6 + got.hi:6 + 2 * n])
    np.testing.assert_array_equal(cr.set_of(22, 5, 4), [0] * 5 + [1] * 5 + [2] * 5 + [3] * 7)


@pytest.mark.parametrize("nfft", (16, 256, 4096))
def test_restatement_anchors(nfft):
    a, b = cr.parity_pair()
    fa, fb, n = cr.PARITY_FIRST_A, cr.PARITY_FIRST_B, cr.PARITY_SAMPLES
    thr = cr.parity_threshold(nfft)
    # W = 0: the excisor on capture a
    zero = cr.cancel(a, b, np.zeros(nfft), thr, nfft, fa, fb, n)
    plain = er.excise(a, thr, nfft, fa, n)
    assert np.array_equal(zero.out, plain.out) and np.array_equal(zero.records["total"], plain.records["total"])
    assert np.array_equal(zero.records["total_in"], zero.records["total"]) and np.array_equal(zero.records["removed"], plain.records["removed"])
    # a capture against itself, W = 1: nothing is left, and rint(127.5) = 128
    none = cr.cancel(a, a, np.ones(nfft), None, nfft, fa, fa, n)
    assert not none.records["total"].any() and np.all(none.out[none.lo:none.hi] == 128) and np.all(none.records["total_in"] > 0)
    # every threshold negative
    w = cr.parity_weights(nfft)
    gone = cr.cancel(a, b, w, np.full(nfft, -1.0), nfft, fa, fb, n, cr.PARITY_FRAMES_PER_SET)
    assert np.array_equal(gone.records["removed"], gone.records["total"]) and np.all(gone.records["n_excised"] == nfft)
    # NaN never cuts, +inf never cuts
    for v in (np.nan, np.inf):
        assert not cr.cancel(a, b, w, np.full(nfft, v), nfft, fa, fb, n, cr.PARITY_FRAMES_PER_SET).cut.any()


def test_parity_inputs_keep_clear_of_thresholds_and_rounding_ties():
    """What the GPU parity test rests on, asserted on the restatement alone; re-measures E32."""
    worst_e32, worst_margin, worst_share = 0.0, np.inf, 0.0
    for nfft in cr.NFFT:
        for offset, scale in cr.CONVENTIONS:
            w = cr.parity_weights(nfft, offset)
            sets = cr.parity_sets(nfft)
            assert w.shape == (sets, nfft) and w.dtype == np.complex64 and np.abs(w).max() <= 1.0
            assert w[0, 3] == 1.0 and w[-1, -2] == np.complex64(-0.6 + 0.3j)
            frames = er.frames_loop(cr.PARITY_SAMPLES, nfft)
            assert (sets - 1) * cr.PARITY_FRAMES_PER_SET < frames <= sets * cr.PARITY_FRAMES_PER_SET
            r64, r32 = cr.parity_reference(nfft, offset, scale), cr.parity_reference(nfft, offset, scale, single=True)
            margin = er.threshold_margin(r64.power, cr.parity_threshold(nfft, scale))
            share = float(np.mean(er.tie_distance(r64.value) <= cr.TIE_BAND))
            e32 = float(np.max(np.abs(r64.value - r32.value)))
            cut = int(r64.cut.sum())
            print(f"nfft {nfft} offset {offset}: margin {margin:.2e}, {cut} of {r64.cut.size} bins cut, tie share {share:.2e}, e32 {e32:.2e}")
            assert margin >= cr.NEAR_TIE, (nfft, offset, margin)
            assert share <= cr.TIE_SHARE_MAX, (nfft, offset, share)
            assert 0 < cut < r64.cut.size // 4 and np.array_equal(r32.cut, r64.cut)
            assert r64.records["total"].sum() < 0.5 * r64.records["total_in"].sum(), "the common source is taken out"
            worst_e32, worst_margin, worst_share = max(worst_e32, e32), min(worst_margin, margin), max(worst_share, share)
    print(f"smallest margin {worst_margin:.2e}, largest tie share {worst_share:.2e}, E32 {worst_e32!r} (recorded {cr.E32_MEASURED!r})")
    assert worst_e32 <= cr.E32 and abs(worst_e32 - cr.E32_MEASURED) <= 0.02 * cr.E32_MEASURED
    assert cr.TIE_BAND == 8 * cr.E32 and cr.TIE_SHARE_MAX == 0.002
    # the last set is short wherever 5 does not divide the frame count
    assert [er.frames_loop(cr.PARITY_SAMPLES, n) % 5 for n in cr.NFFT] == [0, 2, 3, 1, 0, 2, 3, 1, 0]


# ------------------------------------------------------------------------------------------------ the weights
def _spectrum(rows=3, nfft=16, seed=5):
    rng = np.random.default_rng(seed)
    sab = (rng.normal(size=(rows, nfft)) + 1j * rng.normal(size=(rows, nfft))).astype(np.complex64)
    sbb = rng.uniform(1.0, 2.0, (rows, nfft)).astype(np.float32)
    saa = (np.abs(sab) ** 2 / sbb * rng.uniform(1.0, 3.0, (rows, nfft))).astype(np.float32)
    msc = (np.abs(sab) ** 2 / (saa * sbb)).astype(np.float32)
    return saa, sbb, sab, msc


def test_cancel_weights():
    saa, sbb, sab, msc = _spectrum()
    sbb[1, 5] = 0.0
    msc[1, 5] = np.nan
    res = cs.as_result(saa, sbb, sab, msc, 16, 16, 8)
    flagged = np.zeros(16, bool)
    flagged[[2, 5, 9, 14]] = True
    det = coherence.Detection(flagged, 0.5, 1e-6)
    w = coherence.cancel_weights(res, det)
    assert w.shape == (3, 16) and w.dtype == np.complex64
    assert not w[:, ~flagged].any() and w[1, 5] == 0, "exactly 0 elsewhere, and where Sbb = 0"
    want = (np.conj(sab.astype(np.complex128)) / np.where(sbb > 0, sbb, 1.0).astype(np.float64)).astype(np.complex64)
    assert np.array_equal(w[:, [2, 9, 14]], want[:, [2, 9, 14]]) and np.array_equal(w[[0, 2], 5], want[[0, 2], 5])
    # the row-summed sums
    one = coherence.cancel_weights(res, det, per_row=False)
    tot = np.conj(sab.astype(np.complex128).sum(axis=0)) / sbb.astype(np.float64).sum(axis=0)
    assert one.shape == (16,) and not one[~flagged].any() and np.array_equal(one[flagged], tot[flagged].astype(np.complex64))
    # flags per cell
    cells = np.zeros((3, 16), bool)
    cells[0, 2] = cells[2, 9] = True
    per = coherence.cancel_weights(res, coherence.Detection(cells, 0.5, 1e-6))
    assert np.count_nonzero(per) == 2 and per[0, 2] == want[0, 2] and per[2, 9] == want[2, 9]
    both = coherence.cancel_weights(res, coherence.Detection(cells, 0.5, 1e-6), per_row=False)
    assert set(np.flatnonzero(both)) == {2, 9}
    with pytest.raises(ValueError):
        coherence.cancel_weights(res, coherence.Detection(np.zeros((2, 16), bool), 0.5, 1e-6))
    # |W|^2 <= Saa / Sbb, and the weight minimises the residual Saa - 2 Re(W Sab) + |W|^2 Sbb
    live = sbb > 0
    assert np.all(np.abs(want[live]) ** 2 <= (saa[live] / sbb[live]) * (1 + 1e-6))
    resid = lambda v: saa - 2 * np.real(v * sab) + np.abs(v) ** 2 * sbb
    assert np.all(resid(want)[live] <= resid(want * 1.01)[live]) and np.all(resid(want)[live] <= resid(want * np.exp(0.01j))[live])
    # detect never flags the DC guard bins, so their weights are 0; detect_cells decides every cell on its own
    msc2 = np.full((3, 16), 0.9, np.float32)
    msc2[0, 4] = 0.1
    full = cs.as_result(saa, np.abs(sbb) + 1, sab, msc2, 16, 16, 8)
    w_all = coherence.cancel_weights(full, coherence.detect(full, 1e-6))
    assert not w_all[:, [0, 1, 15]].any() and w_all[:, 2:15].all()
    c = coherence.detect_cells(full, 1e-6)
    assert c.flagged.shape == (3, 16) and not c.flagged[0, 4] and c.flagged[1, 4] and not c.flagged[:, [0, 1, 15]].any()
    assert c.threshold == coherence.threshold(8, 1e-6) and coherence.cancel_weights(full, c)[0, 4] == 0


# ------------------------------------------------------------------------------------------------ the Python layer
class HostLib(host_lib.HostLib):
    """gj_cancel_dev and gj_csd_dev, which Device.cancel and coherence.scan reach, computed by the restatements on host
    memory (tests/host_lib.py); gj_excise_frames is the real library's (pure host arithmetic)."""

    def gj_cancel_dev(self, ctx, d_a, nbytes_a, first_a, d_b, nbytes_b, first_b, n_samples, nfft, d_w, frames_per_set, n_sets, d_thr,
                      d_out, d_frames):
        self.calls.append(("cancel", first_a, first_b, n_samples, nfft, frames_per_set, n_sets))
        assert d_w % 8 == 0 and d_thr % 4 == 0 and frames_per_set >= 1 and n_sets >= 1
        w = self.view(d_w, n_sets * nfft, np.complex64).reshape(n_sets, nfft)
        got = cr.cancel(self.view(d_a, nbytes_a), self.view(d_b, nbytes_b), w, self.view(d_thr, nfft, np.float32), nfft, first_a,
                        first_b, n_samples, frames_per_set)
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


W_NFFT, W_FA, W_FB, W_N = 64, 3, 8, 11 * 64 + 35                   # 22 frames


def test_device_cancel_on_the_host_double(host_dev):
    lib = host_dev._lib
    a, b = cr.parity_pair()
    w, thr = cr.parity_weights(W_NFFT)[:4], cr.parity_threshold(W_NFFT)
    want = cr.cancel(a, b, w, thr, W_NFFT, W_FA, W_FB, W_N, 5)
    n = 0
    for src_a, held_a in host_lib.sources(host_dev, a):
        for src_b, held_b in host_lib.sources(host_dev, b):
            n += 1
            lib.calls.clear()
            uploads = gpsjam.Capture.uploads
            cleaned, rec = host_dev.cancel(src_a, src_b, w, thr, nfft=W_NFFT, first_a=W_FA, first_b=W_FB, n_samples=W_N, frames_per_set=5)
            assert gpsjam.Capture.uploads == uploads + (src_a is a) + (src_b is b), "host bytes are uploaded once, a resident capture never"
            assert isinstance(cleaned, gpsjam.Capture) and cleaned.nbytes == 2 * W_N and rec.dtype == gpsjam.CANCEL_DTYPE and rec.size == 22
            assert np.array_equal(HostLib.view(cleaned.ptr, cleaned.nbytes), want.out)
            for key in gpsjam.CANCEL_DTYPE.names:
                assert np.array_equal(rec[key], want.records[key].astype(rec[key].dtype))
            # the threshold, the weights as float32 pairs, the output, the records -- and one call
            assert host_lib.mallocs(lib) == [4 * W_NFFT, 8 * 4 * W_NFFT, 2 * W_N, 16 * 22]
            assert lib.calls[-1] == ("cancel", W_FA, W_FB, W_N, W_NFFT, 5, 4) and host_dev.kernel_calls == {"cancel": n}
            assert set(lib.mem) == held_a | held_b | {cleaned.ptr}, "every buffer but the result is freed"
            cleaned.free()
    # the defaults: one set for every frame, no threshold (+inf: nothing is cut), what both captures hold from sample 0;
    # one capture against itself is uploaded once
    lib.calls.clear()
    uploads = gpsjam.Capture.uploads
    short = a[:2 * 300]
    cleaned, rec = host_dev.cancel(short, short, np.ones(W_NFFT), nfft=W_NFFT)
    assert gpsjam.Capture.uploads == uploads + 1 and lib.calls[-1] == ("cancel", 0, 0, 300, W_NFFT, rec.size, 1) and rec.size == 8
    assert not rec["n_excised"].any() and not rec["total"].any() and np.all(HostLib.view(cleaned.ptr, 600)[W_NFFT:8 * W_NFFT] == 128)
    cleaned.free()
    cleaned, rec = host_dev.cancel(a, b[:2 * 500], w[0], nfft=W_NFFT, first_a=1, first_b=4)
    assert lib.calls[-1] == ("cancel", 1, 4, 496, W_NFFT, gpsjam.excise_frames(496, W_NFFT), 1) and cleaned.nsamples == 496
    cleaned.free()
    assert not lib.mem
    # what the wrapper itself refuses
    for bad in (np.zeros(W_NFFT + 1), np.zeros((2, 3, W_NFFT)), np.zeros((0, W_NFFT))):
        with pytest.raises(ValueError, match="weights"):
            host_dev.cancel(a, b, bad, nfft=W_NFFT)
    with pytest.raises(ValueError, match="frames_per_set"):
        host_dev.cancel(a, b, w, nfft=W_NFFT)
    with pytest.raises(ValueError, match="threshold"):
        host_dev.cancel(a, b, w[0], np.zeros(W_NFFT - 1), nfft=W_NFFT)
    assert not lib.mem and host_dev.kernel_calls == {"cancel": 6}


def test_device_cancel_refusals(host_dev):
    lib = host_dev._lib
    a, b = cr.parity_pair()
    w = cr.parity_weights(W_NFFT)[0]
    host_lib.check_freed(host_dev, a, lambda cap: host_dev.cancel(cap, b, w, nfft=W_NFFT))
    host_lib.check_freed(host_dev, b, lambda cap: host_dev.cancel(a, cap, w, nfft=W_NFFT))
    lib.refuse("gj_cancel_dev")
    host_lib.check_refused(host_dev, a, lambda s: host_dev.cancel(s, b, w, nfft=W_NFFT, n_samples=W_N), gpsjam.GpsJamError,
                           host_lib.REFUSED_TEXT, counted="cancel")
    assert host_lib.mallocs(lib) == [4 * W_NFFT, 8 * W_NFFT, 2 * W_N, 16 * 22] * 2
    lib.calls.clear()
    # an empty range: the buffers are never empty, the library refuses
    host_lib.check_refused(host_dev, a, lambda s: host_dev.cancel(s, b, w, nfft=W_NFFT, first_a=a.size // 2), gpsjam.GpsJamError,
                           host_lib.REFUSED_TEXT, counted="cancel")
    assert host_lib.mallocs(lib) == [4 * W_NFFT, 8 * W_NFFT, 1, 16] * 2 and host_dev.kernel_calls == {"cancel": 4}


S_NFFT, S_M = 64, 8                                                 # rows of 8 frame pairs of 64 points: 512 samples


def _spatial_pair(jam_rows=(2, 3), rows=4, tail=200):
    """Independent noise in both; in the given rows (the last one with the tail behind it) a common wide-band source, in
    b turned by 1 rad."""
    n = rows * S_NFFT * S_M + tail
    r = np.random.default_rng(12)
    za, zb = (r.normal(0, 6.0, n) + 1j * r.normal(0, 6.0, n) for _ in range(2))
    src = r.normal(0, 25.0, n) + 1j * r.normal(0, 25.0, n)
    on = np.zeros(n, bool)
    for row in jam_rows:
        on[row * S_NFFT * S_M:(n if row == rows - 1 else (row + 1) * S_NFFT * S_M)] = True
    za, zb = za + src * on, zb + src * on * np.exp(1j)
    out = []
    for z in (za, zb):
        iq = np.empty(2 * n)
        iq[0::2], iq[1::2] = z.real, z.imag
        out.append((np.clip(np.round(iq), -128, 127) + 128).astype(np.uint8))
    return out


def test_clean_spatial_on_the_host_double(host_dev):
    lib = host_dev._lib
    a, b = _spatial_pair()
    n = a.size // 2
    res = mitigate.clean_spatial(host_dev, a, b, nfft=S_NFFT, frames_per_row=S_M, p_fa=1e-4, lag=0)
    try:
        kinds = [c for c in lib.calls if c[0] != "malloc"]
        frames = gpsjam.excise_frames(n, S_NFFT)
        assert kinds == [("csd", 0, 0, S_NFFT, S_NFFT, S_M, 4), ("cancel", 0, 0, n, S_NFFT, 2 * S_M, 4)], "hop = nfft; a set per row, 2 M frames each"
        assert host_dev.kernel_calls == {"cross_spectrum": 1, "cancel": 1} and frames == 2 * 4 * S_M + 5
        assert isinstance(res, mitigate.CleanedSpatial) and res.cancelled and res.note == "" and res.capture.nsamples == n
        assert res.records.size == frames and res.weights.shape == (4, S_NFFT) and res.weights.dtype == np.complex64
        # the weights are cancel_weights of the scan's own result, cell by cell: none in the quiet rows
        cells = coherence.detect_cells(res.scan.result, 1e-4)
        assert np.array_equal(res.weights, coherence.cancel_weights(res.scan.result, cells)) and res.scan.lag == 0
        assert not res.weights[:2].any() and np.count_nonzero(res.weights[2]) >= S_NFFT - 8 and not res.weights[:, [0, 1, -1]].any()
        # arg W = -1 rad; over M = 8 pairs at MSC 0.9 its standard deviation is sqrt((1 - MSC) / (2 M MSC)) = 0.08 rad: five of them
        np.testing.assert_allclose(np.angle(res.weights[3][res.weights[3] != 0]), -1.0, atol=0.4)
        # rows 0 and 1 are excisor frames [0, 32): identity there (frame 31 ends where row 2 begins)
        quiet = 2 * (2 * S_M * S_NFFT - S_NFFT)
        out = HostLib.view(res.capture.ptr, res.capture.nbytes)
        assert np.array_equal(out[:quiet], a[:quiet]) and not np.array_equal(out[quiet:], a[quiet:])
        # the leftover frames use the last set; the suppression is that of the frames with a weight in the band
        sets = cr.set_of(frames, 2 * S_M, 4)
        assert list(sets[-6:]) == [3] * 6 and len(res.bands) >= 1 and len(res.suppression_db) == len(res.bands)
        active = sets >= 2
        t_in, t_out = res.records["total_in"].astype(np.float64), res.records["total"].astype(np.float64)
        assert res.suppression_db[0] == pytest.approx(10 * np.log10(t_in[active].sum() / t_out[active].sum()))
        # a source of 1250 in noise of 72, MSC 0.894: a cancelled bin keeps (1 - MSC) (1 + 1 / M) = 0.12 of its power, and
        # at least 56 of the 64 bins are cancelled (above): at most 8 / 64 + 0.12 * 56 / 64 = 0.23 is left, 6.4 dB
        assert res.suppression_db[0] > 6.0
        assert sum(bd.n_bins for bd in res.bands) == int(np.any(res.weights != 0, axis=0).sum())
    finally:
        res.capture.free()
    assert not lib.mem, "every buffer but the result is freed"
    # resident captures and an integer lag: the pair is aligned first, and the result covers the aligned range
    lib.calls.clear()
    with gpsjam.Capture(host_dev, a) as ca, gpsjam.Capture(host_dev, b) as cb:
        uploads = gpsjam.Capture.uploads
        shifted = mitigate.clean_spatial(host_dev, ca, cb, nfft=S_NFFT, frames_per_row=S_M, p_fa=1e-4, lag=-2, threshold=np.full(S_NFFT, 1e9))
        assert gpsjam.Capture.uploads == uploads
        kinds = [c for c in lib.calls if c[0] != "malloc"]
        assert kinds[0][:3] == ("csd", 2, 0) and kinds[1][:4] == ("cancel", 2, 0, n - 2) and shifted.scan.lag == -2
        shifted.capture.free()


def test_clean_spatial_with_nothing_flagged_returns_a_copy(host_dev):
    lib = host_dev._lib
    a, b = _spatial_pair(jam_rows=())
    res = mitigate.clean_spatial(host_dev, a, b, nfft=S_NFFT, frames_per_row=S_M, lag=0)
    try:
        assert not res.cancelled and res.note == "nothing coherent was flagged: a copy of main" and res.bands == [] and res.suppression_db == []
        assert np.array_equal(HostLib.view(res.capture.ptr, res.capture.nbytes), a) and not res.weights.any()
        kinds = [c for c in lib.calls if c[0] != "malloc"]
        assert kinds[-1] == ("cancel", 0, 0, a.size // 2, S_NFFT, res.records.size, 1)
    finally:
        res.capture.free()
    # a capture shorter than a row: no row, nothing flagged, still a copy; shorter than a frame: refused
    short = mitigate.clean_spatial(host_dev, a[:2 * 300], b[:2 * 300], nfft=S_NFFT, frames_per_row=S_M, lag=0)
    assert not short.cancelled and len(short.scan.result) == 0 and np.array_equal(HostLib.view(short.capture.ptr, 600), a[:600])
    short.capture.free()
    with pytest.raises(ValueError, match="fewer than one frame"):
        mitigate.clean_spatial(host_dev, a[:100], b[:100], nfft=S_NFFT, frames_per_row=S_M, lag=0)
    assert not lib.mem


def test_command_line_takes_the_second_antenna(monkeypatch, tmp_path, capsys):
    """python -m gpsjam.mitigate A.bin OUT.bin --spatial B.bin on the host double."""
    a, b = _spatial_pair()
    pa, pb, po = (str(tmp_path / name) for name in ("a.bin", "b.bin", "out.bin"))
    a.tofile(pa)
    b.tofile(pb)

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
    assert mitigate.main([pa, po, "--spatial", pb, "--nfft", str(S_NFFT), "--frames-per-row", str(S_M), "--p-fa", "1e-4", "--lag", "0"]) == 0
    text = capsys.readouterr().out
    want = mitigate.clean_spatial(other, a, b, nfft=S_NFFT, frames_per_row=S_M, p_fa=1e-4, lag=0)
    assert np.array_equal(np.fromfile(po, np.uint8), HostLib.view(want.capture.ptr, want.capture.nbytes))
    assert not double._lib.mem, "the command frees what it made"
    double._ctx = other._ctx = None
    assert "band(s) cancelled" in text and "suppression" in text and "aligned by 0" in text
    with pytest.raises(SystemExit):
        mitigate.main([pa, po, "--spatial", pb, "--pulsed"])


# ------------------------------------------------------------------------------------------------ end to end
def test_end_to_end_on_the_cpu_gives_the_gpu_tests_tolerance():
    """The restated chain on cr.e2e_pair(): csd at hop = nfft, detect_cells, cancel_weights, the canceller, C/N0 by the
    oracle's acquisition.  Asserts what the GPU test takes for granted -- raw and excised, none acquires; jammer-free, all
    do -- and re-measures E2E_CPU_RESIDUAL_DB, which E2E_CN0_TOL_DB is twice of."""
    from oracle import gpsjam_oracle as orc
    free_a, _ = cr.e2e_pair(False)
    a, b = cr.e2e_pair(True)
    lead, nfft, m = er.E2E_LEAD, cr.E2E_NFFT, cr.E2E_FRAMES_PER_ROW
    assert a[:2 * lead].tobytes() == free_a[:2 * lead].tobytes() and a.size == b.size == 2 * (lead + er.E2E_AFTER)
    assert all(abs(abs(d) % (2 * np.pi)) >= np.pi / 2 and abs(abs(d) % (2 * np.pi)) <= 1.5 * np.pi for d in cr.E2E_SAT_DPHI), "90 degrees from the jammer's"

    def acquire(raw):
        return [orc.acq_search(raw, lead, prn)[0] for prn, *_ in er.E2E_SATS]
    free, before = acquire(free_a), acquire(a)
    assert all(r["acquired"] for r in free) and not any(r["acquired"] for r in before)
    # mitigate.clean restated: the per-bin floor of the quiet part raised by 12 dB
    floor = (np.abs(cr.frame_spectra(a, nfft, 0, lead)) ** 2).mean(axis=0) / 127.5 ** 2
    excised = er.excise(a, (floor * 10.0 ** 1.2).astype(np.float32), nfft)
    assert not any(r["acquired"] for r in acquire(excised.out)), "the excisor has nothing to cut in a flat jammer"
    # clean_spatial restated
    result = cs.as_result(*cs.csd(a, b, nfft, nfft, m), nfft, nfft, m)
    cells = coherence.detect_cells(result, 1e-6)
    assert len(result) == 5 and not cells.flagged[:4].any() and cells.flagged[4].sum() >= nfft - 16
    w = coherence.cancel_weights(result, cells)
    w_abs = float(np.median(np.abs(w[4][cells.flagged[4]])))
    got = cr.cancel(a, b, w, None, nfft, frames_per_set=2 * m)
    assert got.out[:2 * (lead - nfft)].tobytes() == a[:2 * (lead - nfft)].tobytes(), "the quiet lead-in comes back byte-identical"
    worst = 0.0
    for (prn, *_), dphi, r, f, j in zip(er.E2E_SATS, cr.E2E_SAT_DPHI, acquire(got.out), free, before):
        resid = r["cn0"] - (f["cn0"] + cr.e2e_predicted_db(w_abs, dphi))
        worst = max(worst, abs(resid))
        print(f"PRN {prn}: C/N0 {f['cn0']:.2f} jammer-free, {j['cn0']:.2f} jammed, {r['cn0']:.2f} cancelled; median |W| {w_abs:.3f} "
              f"predicts {cr.e2e_predicted_db(w_abs, dphi):+.2f} dB, residual {resid:+.3f} dB")
        assert r["acquired"] and r["codei"] == f["codei"] and abs(r["freqi"] - f["freqi"]) <= 1
    print(f"worst residual {worst:.3f} dB (recorded {cr.E2E_CPU_RESIDUAL_MEASURED}), tolerance {cr.E2E_CN0_TOL_DB} dB")
    assert worst <= cr.E2E_CPU_RESIDUAL_DB and abs(worst - cr.E2E_CPU_RESIDUAL_MEASURED) < 0.005
    assert cr.E2E_CN0_TOL_DB == 2.0 * cr.E2E_CPU_RESIDUAL_DB
