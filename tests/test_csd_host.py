"""CPU side of the cross-spectral density (gj_csd_dev) and of the detector built on it (gpsjam/coherence.py): the row
arithmetic and the workspace formula of the C-ABI, identities of the float64 restatement the GPU tests compare with
(tests/csd_restatement.py), the threshold's distribution, the detector, the bands and their delays on the restatement's
arrays, and the guarantee the GPU end-to-end test relies on: no off-DC cell of any input it uses lies near the
threshold.  No GPU call is made."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

SKRYPTY = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gps-jamming_amd", "skrypty")
if SKRYPTY not in sys.path:
    sys.path.append(SKRYPTY)

import csd_restatement as cs
import gpsjam
import host_lib
import ridge_restatement as rr
import skurt_restatement as sr
from gpsjam import _ffi, coherence, kurtosis


# ------------------------------------------------------------------------------------------------ C-ABI, host side
def test_signatures_and_layout():
    sz, i, vp = C.c_size_t, C.c_int, C.c_void_p
    assert _ffi.SIGNATURES["gj_csd_rows"] == (sz, [sz, sz, sz, sz, i, sz, i])
    assert _ffi.SIGNATURES["gj_csd_workspace"] == (sz, [vp, i, i, sz])
    assert _ffi.SIGNATURES["gj_csd_dev"] == (i, [vp, vp, sz, sz, vp, sz, sz, i, sz, i, sz, vp, vp, vp, vp])
    assert _ffi.GJ_VERSION == 150 and _ffi.load().gj_version() == 150
    r = gpsjam.CrossSpectrum(np.arange(12), np.arange(12) * 2, np.arange(12) * 1j, np.ones(12), 4, 4, 5, first_a=3, first_b=7)
    assert len(r) == 3 and r.saa.dtype == r.sbb.dtype == r.msc.dtype == np.float32 and r.sab.dtype == np.complex64
    assert r.saa.shape == r.sbb.shape == r.sab.shape == r.msc.shape == (3, 4)
    assert (r.nfft, r.hop, r.frames_per_row, r.first_a, r.first_b) == (4, 4, 5, 3, 7)
    np.testing.assert_array_equal(r.freq_hz(8.0), [0.0, 2.0, -4.0, -2.0])


def test_python_interface_is_there():
    for name in ("cross_spectrum", "cross_spectrum_dev", "csd_workspace"):
        assert callable(getattr(gpsjam.Device, name))
    for name in ("threshold", "detect", "bands", "band_delay", "scan", "main"):
        assert callable(getattr(coherence, name))
    assert callable(gpsjam.csd_rows) and "CrossSpectrum" in gpsjam.__all__ and "csd_rows" in gpsjam.__all__
    assert "independent frames" in coherence.threshold.__doc__.lower() and "hop >= nfft" in coherence.threshold.__doc__
    assert "share a clock" in coherence.__doc__ and "small against nfft" in coherence.__doc__


def test_csd_rows_matches_the_loop_at_every_boundary():
    lib = _ffi.load()
    for nfft in (16, 48, 256, 4096):
        for hop in (1, 7, nfft // 2 + 37, nfft, 3 * nfft):
            for nbytes_a in (0, 1, 2 * nfft - 1, 2 * nfft, 2 * (nfft + hop), 2 * (nfft + 5 * hop) + 1, 40961):
                for nbytes_b in (2 * nfft, 2 * (nfft + hop) + 1, 2 * (nfft + 9 * hop) - 2, 40961):      # the shorter of two decides
                    for first_a, first_b in ((0, 0), (1, 4), (hop, 0), (0, nbytes_b // 2 - nfft), (nbytes_a // 2 + 1, 0), (3, nbytes_b + 7)):
                        for m in (1, 2, 3, 5):
                            want = cs.rows_that_fit(nbytes_a, first_a, nbytes_b, first_b, nfft, hop, m)
                            args = (nbytes_a, first_a, nbytes_b, first_b, nfft, hop, m)
                            assert lib.gj_csd_rows(*args) == want == gpsjam.csd_rows(*args), args
                            assert want == min(sr.rows_that_fit(nbytes_a, first_a, nfft, hop, m), sr.rows_that_fit(nbytes_b, first_b, nfft, hop, m))
    # a row ends exactly on the last byte of b, a is longer; and one byte pair short of it
    for nfft, hop, fa, fb, m, rows in ((256, 256, 0, 0, 256, 8), (64, 101, 3, 8, 17, 5), (4096, 1, 1, 0, 2, 3)):
        nb = 2 * (fb + (rows * m - 1) * hop + nfft)
        na = 2 * (fa + (rows * m - 1) * hop + nfft) + 1000
        assert lib.gj_csd_rows(na, fa, nb, fb, nfft, hop, m) == rows and lib.gj_csd_rows(na, fa, nb - 2, fb, nfft, hop, m) == rows - 1
        assert lib.gj_csd_rows(nb, fb, na, fa, nfft, hop, m) == rows, "the pair's order does not matter"
    # impossible geometries
    big = 1 << 20
    assert lib.gj_csd_rows(big, 0, big, 0, 0, 8, 4) == 0 and lib.gj_csd_rows(big, 0, big, 0, -16, 8, 4) == 0
    assert lib.gj_csd_rows(big, 0, big, 0, 16, 0, 4) == 0 and lib.gj_csd_rows(big, 0, big, 0, 16, 8, 0) == 0
    assert lib.gj_csd_rows(big, 0, big, 0, 16, 8, -3) == 0
    assert lib.gj_csd_rows(big, 2 ** 64 - 8, big, 0, 16, 8, 4) == 0 and lib.gj_csd_rows(big, 0, big, 2 ** 64 - 8, 16, 8, 4) == 0
    assert lib.gj_csd_rows(2 ** 64 - 1, 0, 2 ** 64 - 1, 1, 16, 1, 2) == ((2 ** 63 - 2) - 16 + 1) // 2
    assert gpsjam.csd_rows(-2, 0, big, 0, 16, 8, 4) == 0 and gpsjam.csd_rows(big, 0, big, 0, 16, 8, 2 ** 40) == 0


def test_workspace_is_one_partial_of_four_per_block():
    lib = _ffi.load()
    for nfft in (16, 256, 4096):
        for m in (2, 15, 16, 17, 33, 130, 65536):
            blocks = -(-m // cs.MAX_RUN)
            for rows in (1, 3, 1000):
                assert lib.gj_csd_workspace(None, nfft, m, rows) == rows * blocks * 4 * nfft * 4, (nfft, m, rows)
    # what gj_csd_dev refuses needs nothing; a product that does not fit a size_t does not wrap
    for nfft, m in ((8, 16), (48, 16), (8192, 16), (256, 1), (256, 0), (256, -2), (256, 65537)):
        assert lib.gj_csd_workspace(None, nfft, m, 4) == 0
    assert lib.gj_csd_workspace(None, 4096, 65536, 2 ** 60) == 0
    assert lib.gj_csd_workspace(None, 16, 2, 2 ** 56) == 0 and lib.gj_csd_workspace(None, 16, 2, 2 ** 55) == 2 ** 63


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("nfft", [16, 256, 4096])
def test_restatement_identities(nfft):
    a, b = cs.parity_pair()
    hop, m = nfft // 2 + 37, 5
    saa, sbb, sab, msc = cs.csd(a, b, nfft, hop, m, 1, 4, 3)
    assert saa.shape == sbb.shape == sab.shape == msc.shape == (3, nfft) and np.all(msc > 0) and np.all(msc <= 1 + 1e-12)
    # the auto-spectra are the kurtosis's S1 of each capture
    np.testing.assert_allclose(saa, sr.sk(a, nfft, hop, m, 1, 3)[0], rtol=1e-12)
    np.testing.assert_allclose(sbb, sr.sk(b, nfft, hop, m, 4, 3)[0], rtol=1e-12)
    # a against itself: MSC = 1 and Sab = Saa
    s1, s2, s12, one = cs.csd(a, a, nfft, hop, m, 1, 1, 3)
    np.testing.assert_allclose(one, 1.0, rtol=1e-12)
    np.testing.assert_allclose(s12.real, s1, rtol=1e-12)
    np.testing.assert_allclose(s12.imag, 0.0, atol=1e-12 * s1.max())
    assert np.array_equal(s1, s2) and np.array_equal(s1, saa)
    # the pair swapped: Sab conjugated, the auto-spectra exchanged, MSC the same
    tbb, taa, tba, tmsc = cs.csd(b, a, nfft, hop, m, 4, 1, 3)
    assert np.array_equal(taa, saa) and np.array_equal(tbb, sbb)
    np.testing.assert_allclose(tba, np.conj(sab), rtol=1e-13, atol=1e-13 * np.abs(sab).max())
    np.testing.assert_allclose(tmsc, msc, rtol=1e-12)
    # silence: NaN
    flat = np.full(2 * 64, 128, np.uint8)
    z = cs.csd(flat, a, 16, 8, 3, 0, 0, None, 128.0, 1 / 128.0)
    assert z[0].shape == (2, 16) and not z[0].any() and not z[2].any() and np.isnan(z[3]).all() and z[1].all()


def test_the_sign_of_the_phase_is_k5s():
    """b delayed by D: arg Sab[k] = -2 pi k D / N, D positive -- on the parity pair (2.5 samples, wide band), over the
    bins 5 .. 100: clear of the DC spur and of the tone at bin -48, which both captures hold without a delay.  With MSC
    0.45 over 512 frame pairs a bin's phase scatters by 0.034 rad and the slope over 96 bins by 0.005 samples: the
    bound is five of those."""
    a, b = cs.parity_pair()
    _, _, sab, msc = cs.csd(a, b, 256, 256, 512, 0, 0, 1)
    res = cs.as_result(np.ones(256), np.ones(256), sab, msc, 256, 256, 512)
    k = np.arange(5, 101)
    want = -2.0 * np.pi * k * cs.PARITY_DELAY / 256
    assert np.max(np.abs(np.angle(sab[0, k] * np.exp(-1j * want)))) < 0.2
    whole = coherence.Band(5, 100, 96, 0.0, 0.0, 0.0)
    print(f"parity pair: {coherence.band_delay(res, whole):.4f} against {cs.PARITY_DELAY}")
    assert abs(coherence.band_delay(res, whole) - cs.PARITY_DELAY) < 0.025
    assert coherence.band_delay(res, whole, coarse_lag=-7) == coherence.band_delay(res, whole) - 7
    assert coherence.band_delay(res, coherence.Band(20, 21, 2, 0.0, 0.0, 0.0)) is None


# ------------------------------------------------------------------------------------------------ the detector
def test_threshold_formula_and_its_distribution():
    assert coherence.threshold(2, 0.25) == 0.75 and abs(coherence.threshold(1024) - (1 - 1e-6 ** (1 / 1023))) < 1e-15
    assert abs(coherence.threshold(4096, 1e-6) - 0.0033680663) < 1e-9
    for bad in ((1, 1e-6), (0, 1e-6), (16, 0.0), (16, 1.0)):
        with pytest.raises(ValueError):
            coherence.threshold(*bad)
    # the noise pair: 4 rows of 1024 frame pairs, 1012 off-DC cells.  P(MSC > g) = (1 - g)^(M - 1)
    ref, msc = cs.detect_reference("noise")
    cells = msc[:, cs.off_dc(cs.DETECT_NFFT)]
    assert len(ref) == 4 and cells.size == 4 * 253
    for p in (1e-3, 1e-2, 1e-1):
        seen, expected = int(np.sum(cells > coherence.threshold(1024, p))), cells.size * p
        print(f"p_fa {p:g}: {seen} of {cells.size} cells exceed the threshold, {expected:.1f} expected")
        assert expected / 3.0 <= seen <= expected * 3.0, (p, seen, expected)
    assert abs(cells.mean() * 1024 - 1.0) < 0.1, "E[MSC] = 1 / M under noise"


def test_no_gpu_input_has_a_cell_near_the_threshold():
    """tests/csd/test_round6_gpu.py expects the flags of the restatement from the device; that is only fair where
    float32 cannot carry a cell across the threshold."""
    worst = {case: cs.edge_distance(cs.detect_reference(case)[1], cs.DETECT_M[case]) for case in cs.CASES}
    print("smallest relative distance of an off-DC cell's MSC to the threshold:", {k: f"{v:.2e}" for k, v in worst.items()})
    bad = {k: v for k, v in worst.items() if v < cs.EDGE}
    assert not bad, bad


def test_noise_flags_nothing_and_dc_is_excluded():
    ref, msc = cs.detect_reference("noise")
    d = coherence.detect(ref, cs.P_FA)
    assert d.threshold == coherence.threshold(1024, 1e-6) and not d.flagged.any() and coherence.bands(ref, d, cs.FS) == []
    # both captures carry the mixer's truncation offset: two constants are perfectly coherent
    print(f"noise: MSC at bin 0 {msc[:, 0]}, at bins +-1 {msc[:, 1]} {msc[:, -1]}, threshold {d.threshold:.4f}")
    assert np.all(msc[:, 0] > 0.2) and np.all(msc[:, [1, -1]] > d.threshold)
    open_dc = coherence.detect(ref, cs.P_FA, dc_guard=-1)
    assert np.flatnonzero(open_dc.flagged).tolist() == [0, 1, 255]
    assert np.flatnonzero(coherence.detect(ref, cs.P_FA, dc_guard=0).flagged).tolist() == [1, 255]
    assert not coherence.detect(cs.detect_reference("noise", 4096)[0], cs.P_FA).flagged.any()


def test_a_jammer_below_the_noise_floor_is_found():
    """Band-limited Gaussian noise 10 dB under the receiver noise inside 100..400 kHz: +0.07 dB in total power, SK = 1."""
    a, b = cs.detect_pair("subnoise")
    a0, b0 = cs.detect_pair("subnoise", False)
    rise = (cs.power_db(a, a0), cs.power_db(b, b0))
    print(f"subnoise: total power +{rise[0]:.3f} dB and +{rise[1]:.3f} dB")
    assert 0.0 < min(rise) and max(rise) < 0.1
    ref, _ = cs.detect_reference("subnoise")
    d = coherence.detect(ref, cs.P_FA)
    hit = np.flatnonzero(d.flagged)
    assert len(ref) == 1 and ref.frames_per_row == 4096
    assert set(range(cs.SUB_BINS_INSIDE[0], cs.SUB_BINS_INSIDE[1] + 1)) <= set(hit.tolist()), hit
    assert hit.min() >= cs.SUB_BINS_OUTSIDE[0] and hit.max() <= cs.SUB_BINS_OUTSIDE[1], hit
    (band,) = coherence.bands(ref, d, cs.FS)
    assert band.n_bins == hit.size and band.freq_lo_hz <= cs.SUB_BAND_HZ[0] + cs.FS / 256 and band.freq_hi_hz >= cs.SUB_BAND_HZ[1] - cs.FS / 256
    # what the one-capture detectors see: K1's +6 dB rule nothing (the rise is 0.07 dB), the kurtosis nothing
    assert max(rise) < 6.0
    for raw in (a, b):
        s1, s2, skv = sr.sk(raw, 256, 256, 256)
        assert not kurtosis.detect(sr.as_result(s1, s2, skv, 256, 256, 256), sr.SIGMAS).flagged.any()


def test_two_jammers_give_two_delays():
    a, b = cs.detect_pair("two")
    ref, _ = cs.detect_reference("two")
    d = coherence.detect(ref, cs.P_FA)
    found = coherence.bands(ref, d, cs.FS)
    assert len(ref) == 4 and len(found) == 2
    lower, upper = found                                                   # ascending frequency
    assert lower.freq_hi_hz < 0 < upper.freq_lo_hz and upper.median_msc > lower.median_msc
    got = (coherence.band_delay(ref, upper), coherence.band_delay(ref, lower))
    print(f"two: {got[0]:.4f} and {got[1]:.4f} against {cs.TWO_DELAY}")
    for have, want in zip(got, cs.TWO_DELAY):
        assert abs(have - want) <= 0.01, (have, want)
    assert cs.full_band_lag(a, b) == 3, "a full-band correlation names the stronger one's delay, rounded"
    # aligned by that lag first, as scan(lag="k5") does: 3 rows, the same two delays, no cell near the threshold
    assert cs.full_band_lag(a, b, coherence.K5_SAMPLES) == 3
    saa, sbb, sab, msc = cs.csd(a, b, cs.DETECT_NFFT, cs.DETECT_HOP, 1024, 0, 3)
    ref = cs.as_result(saa, sbb, sab, msc, cs.DETECT_NFFT, cs.DETECT_HOP, 1024, 0, 3)
    lower, upper = coherence.bands(ref, coherence.detect(ref, cs.P_FA), cs.FS)
    got = (coherence.band_delay(ref, upper, 3), coherence.band_delay(ref, lower, 3))
    print(f"two, aligned by 3: {got[0]:.4f} and {got[1]:.4f}")
    assert len(ref) == 3 and cs.edge_distance(msc, 1024) >= cs.EDGE
    for have, want in zip(got, cs.TWO_DELAY):
        assert abs(have - want) <= 0.01, (have, want)


def test_detector_votes_and_bands():
    msc = np.zeros((4, 16), np.float32)
    msc[:3, 3] = 0.9         # three of four rows: flagged
    msc[:2, 4] = 0.9         # two of four: not more than half
    msc[:, 5] = np.nan       # a dead bin never votes
    msc[:3, 6] = 0.9
    msc[3, 6] = np.nan
    msc[:, 0] = msc[:, 1] = msc[:, 15] = 1.0      # DC and its neighbours
    msc[:, 8] = msc[:, 9] = 0.9                   # -8 and -7: the lowest frequencies
    msc[:, 14] = 0.9                              # -2: just outside the guard
    res = gpsjam.CrossSpectrum(np.ones((4, 16)), np.ones((4, 16)), np.ones((4, 16), np.complex64), msc, 16, 16, 64)
    d = coherence.detect(res, 1e-6)
    assert np.flatnonzero(d.flagged).tolist() == [3, 6, 8, 9, 14]
    got = [(b.first_bin, b.last_bin, b.n_bins, b.freq_lo_hz, b.freq_hi_hz, b.delay) for b in coherence.bands(res, d, 16.0)]
    assert got == [(8, 9, 2, -8.5, -6.5, None), (14, 14, 1, -2.5, -1.5, None), (3, 3, 1, 2.5, 3.5, None), (6, 6, 1, 5.5, 6.5, None)]
    assert np.flatnonzero(coherence.detect(res, 1e-6, dc_guard=2).flagged).tolist() == [3, 6, 8, 9]


# ------------------------------------------------------------------------------------------------ the Python layer
class HostLib(host_lib.HostLib):
    """gj_csd_dev, which Device.cross_spectrum reaches, computed by the restatement on host memory (tests/host_lib.py);
    the timer around it returns a constant."""

    def gj_csd_dev(self, ctx, d_a, nbytes_a, first_a, d_b, nbytes_b, first_b, nfft, hop, frames_per_row, n_rows, d_saa, d_sbb, d_sab, d_msc):
        self.calls.append(("csd", first_a, first_b, nfft, hop, frames_per_row, n_rows))
        assert d_sab % 8 == 0 and d_saa % 4 == 0 and d_sbb % 4 == 0
        saa, sbb, sab, msc = cs.csd(self.view(d_a, nbytes_a), self.view(d_b, nbytes_b), nfft, hop, frames_per_row, first_a, first_b, n_rows)
        self.view(d_saa, n_rows * nfft, np.float32)[:] = saa.reshape(-1)
        self.view(d_sbb, n_rows * nfft, np.float32)[:] = sbb.reshape(-1)
        self.view(d_sab, n_rows * nfft, np.complex64)[:] = sab.reshape(-1)
        if d_msc:
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


W_NFFT, W_HOP, W_M, W_FA, W_FB, W_ROWS = 16, 5, 3, 2, 5, 4
_PAIR = cs.parity_pair()
W_A = _PAIR[0][:2 * (W_FA + (W_ROWS * W_M - 1) * W_HOP + W_NFFT + 40)]              # a is longer: b decides
W_B = _PAIR[1][:2 * (W_FB + (W_ROWS * W_M - 1) * W_HOP + W_NFFT + 2 * W_HOP)]        # two frames short of a 5th row


def _want(*args):
    saa, sbb, sab, msc = cs.csd(*args)
    return saa.astype(np.float32), sbb.astype(np.float32), sab.astype(np.complex64), msc.astype(np.float32)


def test_device_cross_spectrum_on_the_host_double(host_dev):
    lib = host_dev._lib
    want = _want(W_A, W_B, W_NFFT, W_HOP, W_M, W_FA, W_FB)
    assert want[0].shape == (W_ROWS, W_NFFT) and gpsjam.csd_rows(W_A.size, W_FA, W_B.size, W_FB, W_NFFT, W_HOP, W_M) == W_ROWS
    n = 0
    for src_a, held_a in host_lib.sources(host_dev, W_A):
        for src_b, held_b in host_lib.sources(host_dev, W_B):
            n += 1
            lib.calls.clear()
            uploads, host_dev.last_kernel_ms = gpsjam.Capture.uploads, 0.0
            got = host_dev.cross_spectrum(src_a, src_b, W_NFFT, W_HOP, W_M, first_a=W_FA, first_b=W_FB)
            assert gpsjam.Capture.uploads == uploads + (src_a is W_A) + (src_b is W_B), "host bytes are uploaded once, a resident capture never"
            assert isinstance(got, gpsjam.CrossSpectrum)
            assert (got.nfft, got.hop, got.frames_per_row, got.first_a, got.first_b) == (W_NFFT, W_HOP, W_M, W_FA, W_FB)
            for have, ref in zip((got.saa, got.sbb, got.sab, got.msc), want):
                assert have.shape == (W_ROWS, W_NFFT) and have.dtype == ref.dtype and have.tobytes() == ref.tobytes()
            assert host_lib.mallocs(lib) == [5 * 4 * W_ROWS * W_NFFT], "one buffer holds the four arrays"
            assert lib.calls[-1] == ("csd", W_FA, W_FB, W_NFFT, W_HOP, W_M, W_ROWS) and host_dev.kernel_calls == {"cross_spectrum": n}
            assert host_dev.last_kernel_ms == 0.25
            assert set(lib.mem) == held_a | held_b, "every buffer of the call's own is freed"
    # the defaults: hop nfft, both ranges from sample 0; a given row count is taken as it is; one capture against itself
    lib.calls.clear()
    uploads = gpsjam.Capture.uploads
    part = host_dev.cross_spectrum(W_A, W_A, W_NFFT, frames_per_row=2, n_rows=2)
    assert gpsjam.Capture.uploads == uploads + 1, "the same object is uploaded once"
    assert lib.calls == [("malloc", 5 * 4 * 2 * W_NFFT), ("csd", 0, 0, W_NFFT, W_NFFT, 2, 2)] and (part.hop, len(part)) == (W_NFFT, 2)
    for have, ref in zip((part.saa, part.sbb, part.sab, part.msc), _want(W_A, W_A, W_NFFT, W_NFFT, 2, 0, 0, 2)):
        assert have.tobytes() == ref.tobytes()
    assert not lib.mem and host_dev.kernel_calls == {"cross_spectrum": 5}
    np.testing.assert_allclose(part.merged(), 1.0, rtol=1e-6)


def test_device_cross_spectrum_refusals_and_the_empty_result(host_dev):
    lib = host_dev._lib
    host_lib.check_freed(host_dev, W_A, lambda cap: host_dev.cross_spectrum(cap, W_B, W_NFFT))
    host_lib.check_freed(host_dev, W_B, lambda cap: host_dev.cross_spectrum(W_A, cap, W_NFFT))
    # no row fits: an empty result with the call's geometry, and the library is not reached
    short = W_B[:2 * (W_FB + (W_M - 1) * W_HOP + W_NFFT - 1)]                        # one sample short of the first row
    for source, held in host_lib.sources(host_dev, short):
        empty = host_dev.cross_spectrum(W_A, source, W_NFFT, W_HOP, W_M, first_a=W_FA, first_b=W_FB)
        assert len(empty) == 0 and empty.saa.shape == empty.sbb.shape == empty.sab.shape == empty.msc.shape == (0, W_NFFT)
        assert empty.sab.dtype == np.complex64 and empty.msc.dtype == np.float32 and np.isnan(empty.merged()).all()
        assert (empty.nfft, empty.hop, empty.frames_per_row, empty.first_a, empty.first_b) == (W_NFFT, W_HOP, W_M, W_FA, W_FB)
        assert set(lib.mem) == held and host_dev.kernel_calls == {} and not host_lib.mallocs(lib)
    # ... unless the geometry is one the library refuses: that is left to the library
    lib.refuse("gj_csd_dev")
    host_lib.check_refused(host_dev, short, lambda s: host_dev.cross_spectrum(W_A, s, W_NFFT, W_HOP, 1, first_b=40),
                           gpsjam.GpsJamError, host_lib.REFUSED_TEXT, counted="cross_spectrum")
    assert host_lib.mallocs(lib) == [5 * 4 * W_NFFT] * 2, "the buffer is never empty"
    lib.calls.clear()
    host_lib.check_refused(host_dev, W_A, lambda s: host_dev.cross_spectrum(s, W_B, W_NFFT, W_HOP, W_M), gpsjam.GpsJamError,
                           host_lib.REFUSED_TEXT, counted="cross_spectrum")
    rows = cs.rows_that_fit(W_A.size, 0, W_B.size, 0, W_NFFT, W_HOP, W_M)        # both ranges from sample 0: one row more
    assert rows == W_ROWS + 1 and host_lib.mallocs(lib) == [5 * 4 * rows * W_NFFT] * 2
    assert host_dev.kernel_calls == {"cross_spectrum": 4}


def test_scan_aligns_the_pair_by_the_integer_lag(host_dev):
    lib = host_dev._lib
    for lag, firsts in ((0, (0, 0)), (3, (0, 3)), (-2, (2, 0))):
        lib.calls.clear()
        got = coherence.scan(host_dev, W_A, W_B, lag=lag, nfft=W_NFFT, frames_per_row=W_M)
        (call,) = [c for c in lib.calls if c[0] == "csd"]
        assert call[1:3] == firsts and got.lag == lag and (got.result.first_a, got.result.first_b) == firsts
        assert got.detection.threshold == coherence.threshold(W_M) and not lib.mem
        for band in got.bands:
            assert band.delay is None or band.delay == coherence.band_delay(got.result, band._replace(delay=None), lag)


def test_the_drop_in_lists_one_lag_per_band(host_dev, monkeypatch):
    """triangulateTDOA.correlation_lag_bands(file_b, file_a): b first, as correlation_lag takes its slices."""
    import triangulateTDOA as tt
    monkeypatch.setattr(gpsjam, "default_device", lambda: host_dev)
    a, b = cs.parity_pair()
    want = coherence.scan(host_dev, a, b, lag=2, nfft=64, frames_per_row=256)
    assert len(want.bands) >= 1 and any(bd.delay is not None for bd in want.bands)
    got = tt.correlation_lag_bands(tt.IQCapture(b), tt.IQCapture(a), lag=2, nfft=64, frames_per_row=256)
    assert got == [(bd.freq_lo_hz, bd.freq_hi_hz, bd.delay) for bd in want.bands if bd.delay is not None]
    assert all(lo < hi and isinstance(lag, float) for lo, hi, lag in got) and not host_dev._lib.mem
    (upper,) = [r for r in got if r[0] > 0]            # the positive frequencies: clear of the tone, which has no delay
    assert abs(upper[2] - cs.PARITY_DELAY) < 0.1, upper
