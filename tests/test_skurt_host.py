"""CPU side of the spectral kurtosis (gj_sk_dev) and of the detector built on it (gpsjam/kurtosis.py): the row
arithmetic of the C-ABI, the float64 restatement the GPU tests compare with (tests/skurt_restatement.py) checked
against the ridge's restatement, the detector and the excision thresholds on the restatement's sums, and the guarantee
the GPU detection test relies on: no cell of any input it uses lies near a band edge.  No GPU call is made."""
import ctypes as C

import numpy as np
import pytest

import excise_restatement as er
import gpsjam
import host_lib
import ridge_restatement as rr
import skurt_restatement as sr
from gpsjam import _ffi, kurtosis


# ------------------------------------------------------------------------------------------------ C-ABI, host side
def test_sk_rows_matches_the_loop_at_every_boundary():
    lib = _ffi.load()
    for nfft in (16, 48, 256, 4096):
        for hop in (1, 7, nfft // 2, nfft // 2 + 37, nfft, nfft + 5, 3 * nfft):
            lengths = {0, 1, 2 * nfft - 2, 2 * nfft - 1, 2 * nfft, 2 * nfft + 1, 2 * (nfft + hop) - 1, 2 * (nfft + hop),
                       2 * (nfft + hop) + 1, 2 * (nfft + 5 * hop) + 1, 2 * (nfft + 9 * hop) - 2, 40961}
            for nbytes in sorted(lengths):
                for first in (0, 1, 2, hop, nbytes // 2 - nfft, nbytes // 2 - nfft + 1, nbytes // 2, nbytes // 2 + 1, nbytes + 7):
                    if first < 0:
                        continue
                    for m in (1, 2, 3, 5, 10):
                        want = sr.rows_that_fit(nbytes, first, nfft, hop, m)
                        assert lib.gj_sk_rows(nbytes, first, nfft, hop, m) == want, (nbytes, first, nfft, hop, m)
                        assert gpsjam.sk_rows(nbytes, first, nfft, hop, m) == want
                        assert want == rr.frames_that_fit(nbytes, first, nfft, hop) // m
    # a row ends exactly on the capture's last byte, and one byte pair short of it
    for nfft, hop, first, m, rows in ((256, 256, 0, 256, 8), (64, 101, 3, 17, 5), (4096, 1, 1, 2, 3)):
        nbytes = 2 * (first + (rows * m - 1) * hop + nfft)
        assert lib.gj_sk_rows(nbytes, first, nfft, hop, m) == rows and lib.gj_sk_rows(nbytes - 2, first, nfft, hop, m) == rows - 1
        assert lib.gj_sk_rows(nbytes + 1, first, nfft, hop, m) == rows
    # impossible geometries
    assert lib.gj_sk_rows(1 << 20, 0, 0, 8, 4) == 0
    assert lib.gj_sk_rows(1 << 20, 0, -16, 8, 4) == 0
    assert lib.gj_sk_rows(1 << 20, 0, 16, 0, 4) == 0
    assert lib.gj_sk_rows(1 << 20, 0, 16, 8, 0) == 0
    assert lib.gj_sk_rows(1 << 20, 0, 16, 8, -3) == 0
    assert lib.gj_sk_rows(1 << 20, 2 ** 64 - 8, 16, 8, 4) == 0          # first_sample + nfft must not wrap
    assert lib.gj_sk_rows(2 ** 64 - 1, 0, 16, 1, 2) == ((2 ** 63 - 1) - 16 + 1) // 2
    assert lib.gj_sk_rows(2 ** 64 - 1, 0, 16, 1, 2 ** 31 - 1) == ((2 ** 63 - 1) - 16 + 1) // (2 ** 31 - 1)
    assert gpsjam.sk_rows(-2, 0, 16, 8, 4) == 0 and gpsjam.sk_rows(1 << 20, 0, 16, 8, 2 ** 40) == 0


def test_workspace_is_one_partial_pair_per_block():
    lib = _ffi.load()
    for nfft in (16, 256, 4096):
        for m in (2, 15, 16, 17, 33, 130, 65536):
            blocks = -(-m // sr.MAX_RUN)
            for rows in (1, 3, 1000):
                assert lib.gj_sk_workspace(None, nfft, m, rows) == rows * blocks * 2 * nfft * 4, (nfft, m, rows)
    # what gj_sk_dev refuses needs nothing; a product that does not fit a size_t does not wrap
    for nfft, m in ((8, 16), (48, 16), (8192, 16), (256, 1), (256, 0), (256, 65537)):
        assert lib.gj_sk_workspace(None, nfft, m, 4) == 0
    assert lib.gj_sk_workspace(None, 4096, 65536, 2 ** 60) == 0


def test_signatures_and_layout():
    assert _ffi.SIGNATURES["gj_sk_rows"] == (C.c_size_t, [C.c_size_t, C.c_size_t, C.c_int, C.c_size_t, C.c_int])
    assert _ffi.SIGNATURES["gj_sk_workspace"] == (C.c_size_t, [C.c_void_p, C.c_int, C.c_int, C.c_size_t])
    res, args = _ffi.SIGNATURES["gj_sk_dev"]
    assert res is C.c_int and len(args) == 11 and args[-3:] == [C.c_void_p] * 3 and args[6] is C.c_int and args[7] is C.c_size_t
    assert _ffi.GJ_VERSION == 150
    r = gpsjam.SpectralKurtosis(np.arange(12), np.arange(12) * 2, np.ones(12), 4, 4, 5, first_sample=3)
    assert len(r) == 3 and r.s1.dtype == r.s2.dtype == r.sk.dtype == np.float32 and r.s1.shape == r.s2.shape == r.sk.shape == (3, 4)
    assert (r.nfft, r.hop, r.frames_per_row, r.first_sample) == (4, 4, 5, 3)
    np.testing.assert_array_equal(r.freq_hz(8.0), [0.0, 2.0, -4.0, -2.0])


def test_python_interface_is_there():
    for name in ("spectral_kurtosis", "spectral_kurtosis_dev", "sk_workspace"):
        assert callable(getattr(gpsjam.Device, name))
    for name in ("band", "detect", "bands", "excision_threshold", "scan", "main"):
        assert callable(getattr(kurtosis, name))
    assert callable(gpsjam.sk_rows) and "SpectralKurtosis" in gpsjam.__all__ and "sk_rows" in gpsjam.__all__
    assert kurtosis.Detection._fields[:2] == ("steady", "intermittent")
    lo, hi = kurtosis.band(256)
    assert (lo, hi) == (0.5, 1.5) and kurtosis.band(64, 2.0) == (0.5, 1.5)
    with pytest.raises(ValueError):
        kurtosis.band(1)


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("nfft", [16, 256, 4096])
def test_restatement_agrees_with_the_ridge_restatement(nfft):
    """sum_k S1[r][k] is the sum of the row's frame totals (the ridge's `total`, same window, no mean removal, same units)."""
    raw = rr.parity_capture()
    for hop, first, m in ((nfft, 0, 5), (nfft // 2 + 37, 1, 3)):
        s1, s2, skv = sr.sk(raw, nfft, hop, m, first, 4)
        rec, _ = rr.ridge(raw, nfft, hop, first, 4 * m)
        np.testing.assert_allclose(s1.sum(axis=1), rec["total"].reshape(4, m).sum(axis=1), rtol=1e-12)
        assert np.all(s2.max(axis=1) <= (rec["peak"].reshape(4, m) ** 2).sum(axis=1) * (1 + 1e-12))
        assert s1.shape == s2.shape == skv.shape == (4, nfft) and np.all(skv > -1e-9)


def test_restatement_limits():
    # one constant power per frame: S2 = S1^2 / M, SK = 0; alternating 0 and P: SK = (M + 1) / (M - 1) * 1
    p = np.full((8, 4), 3.0)
    np.testing.assert_allclose(sr.sums_of(p, 8)[2], 0.0, atol=1e-15)
    p[1::2] = 0.0
    np.testing.assert_allclose(sr.sums_of(p, 8)[2], 9.0 / 7.0)
    # silence: NaN, in the restatement and in merged()
    s1, s2, skv = sr.sk(np.full(2 * 64, 128, np.uint8), 16, 8, 3, 0, None, 128.0, 1 / 128.0)
    assert s1.shape == (2, 16) and not s1.any() and not s2.any() and np.isnan(skv).all()
    assert np.isnan(sr.as_result(s1, s2, skv, 16, 8, 3).merged()).all()
    # exponential powers (Gaussian noise): mean 1, standard deviation 2 / sqrt(M)
    rng = np.random.default_rng(5)
    v = sr.sums_of(rng.exponential(size=(512, 4000)), 512)[2]
    assert abs(v.mean() - 1.0) < 0.01 and abs(v.std() / (2.0 / np.sqrt(512)) - 1.0) < 0.05


def test_merged_is_the_estimator_over_all_rows():
    raw = sr.detect_capture("tone")
    s1, s2, skv = sr.sk(raw, 256, 256, 256)
    whole = sr.sk(raw, 256, 256, 2048)[2][0]
    np.testing.assert_allclose(sr.as_result(s1, s2, skv, 256, 256, 256).merged(), whole, rtol=1e-5)       # s1, s2 pass through float32


# ------------------------------------------------------------------------------------------------ the detector
def test_interferers_are_far_below_the_power_rule():
    want = {"tone": 0.23, "pulse": 0.21, "chirp": 0.50}
    for case in ("tone", "pulse", "chirp"):
        db = sr.power_db(sr.detect_capture(case), sr.detect_capture(case, False))
        print(f"{case}: +{db:.3f} dB")
        assert 0.0 < db < 1.0 and abs(db - want[case]) < 0.02, (case, db)


def test_detector_on_restated_sums():
    """2^19 samples, nfft 256, hop 256, M 256: 8 rows; a bin is flagged when more than half of them lie outside 1 +- 0.5."""
    res, _ = sr.detect_reference("noise")
    d = kurtosis.detect(res, sr.SIGMAS)
    assert len(res) == 8 and (d.lo, d.hi) == (0.5, 1.5)
    assert not d.steady.any() and not d.intermittent.any() and kurtosis.bands(res, d, sr.FS) == []

    res, _ = sr.detect_reference("tone")
    d = kurtosis.detect(res, sr.SIGMAS)
    assert np.flatnonzero(d.steady).tolist() == [sr.TONE_BIN] and not d.intermittent.any()
    (b,) = kurtosis.bands(res, d, sr.FS)
    assert (b.kind, b.first_bin, b.last_bin, b.n_bins) == ("steady", 25, 25, 1) and b.median_sk < 0.5
    assert b.freq_lo_hz < rr.TONE_HZ < b.freq_hi_hz and b.freq_hi_hz - b.freq_lo_hz == sr.FS / 256

    res, _ = sr.detect_reference("pulse")
    d = kurtosis.detect(res, sr.SIGMAS)
    hit = np.flatnonzero(d.intermittent)
    assert not d.steady.any() and hit.size >= 1 and sr.PULSE_BINS[0] <= hit.min() and hit.max() <= sr.PULSE_BINS[1], hit
    assert np.all(np.diff(hit) == 1)
    (b,) = kurtosis.bands(res, d, sr.FS)
    assert b.kind == "intermittent" and b.freq_lo_hz < sr.PULSE_HZ < b.freq_hi_hz and b.median_sk > 1.5

    res, _ = sr.detect_reference("chirp")
    d = kurtosis.detect(res, sr.SIGMAS)
    assert not d.steady.any() and d.intermittent.sum() > 100
    assert all(b.kind == "intermittent" for b in kurtosis.bands(res, d, sr.FS))


def test_detector_votes_and_bands():
    sk = np.ones((4, 8), np.float32)
    sk[:3, 1] = 0.1          # three of four rows low: steady
    sk[:2, 2] = 0.1          # two of four: not more than half
    sk[:3, 7] = 9.0          # bins 7 and 0 are neighbours in frequency but differ in kind
    sk[:3, 0] = 0.1
    sk[:, 4] = np.nan        # a dead bin never votes
    sk[:3, 5] = 9.0
    sk[3, 5] = np.nan
    res = gpsjam.SpectralKurtosis(np.ones((4, 8)), np.ones((4, 8)), sk, 8, 8, 256)
    d = kurtosis.detect(res)
    assert np.flatnonzero(d.steady).tolist() == [0, 1] and np.flatnonzero(d.intermittent).tolist() == [5, 7]
    got = [(b.kind, b.first_bin, b.last_bin, b.n_bins, b.freq_lo_hz, b.freq_hi_hz) for b in kurtosis.bands(res, d, 8.0)]
    assert got == [("intermittent", 5, 5, 1, -3.5, -2.5), ("intermittent", 7, 7, 1, -1.5, -0.5), ("steady", 0, 1, 2, -0.5, 1.5)]
    assert [b.median_sk for b in kurtosis.bands(res, d, 8.0)][0] == 9.0


def test_excision_threshold_rules():
    m = 256
    sk = np.ones((4, 8), np.float32)
    s1 = np.tile(np.arange(1, 9, dtype=np.float64) * m, (4, 1))      # floor k + 1 at bin k
    sk[:3, 1] = 0.1           # steady: notch
    sk[:3, 5] = 9.0           # intermittent: the flat median
    sk[:2, 2] = 9.0           # unflagged, two cells inside: the mean over those
    s1[2:, 2] = 10.0 * m
    sk[:, 6] = 3.0
    sk[:2, 6] = 0.2           # unflagged (two high, two low) without a cell inside: the flat median
    res = gpsjam.SpectralKurtosis(s1, s1, sk, 8, 8, m)
    d = kurtosis.detect(res)
    assert np.flatnonzero(d.flagged).tolist() == [1, 5]
    thr = kurtosis.excision_threshold(res, d, rise_db=10.0)
    flat = np.median([1.0, 10.0, 4.0, 5.0, 8.0])          # unflagged bins with a cell inside: 0, 2, 3, 4, 7
    np.testing.assert_allclose(thr, np.float32([10.0, -1.0, 100.0, 40.0, 50.0, 10 * flat, 10 * flat, 80.0]))
    assert thr.dtype == np.float32
    with pytest.raises(ValueError):
        kurtosis.excision_threshold(res, kurtosis.Detection(np.ones(8, bool), np.zeros(8, bool), d.lo, d.hi))


@pytest.mark.parametrize("amp", sr.EXCISE_AMPS)
def test_detect_excise_detect_leaves_nothing_flagged(amp):
    """A tone that is on from the first sample: no quiet part, no onset.  The thresholds come from the sums alone."""
    raw = sr.excise_capture(amp)
    s1, s2, skv = sr.sk(raw, sr.DETECT_NFFT, sr.DETECT_HOP, sr.DETECT_M)
    res = sr.as_result(s1, s2, skv, sr.DETECT_NFFT, sr.DETECT_HOP, sr.DETECT_M)
    d = kurtosis.detect(res, sr.SIGMAS)
    assert d.steady[sr.TONE_BIN] and not d.intermittent.any() and d.steady.sum() <= 3
    thr = kurtosis.excision_threshold(res, d, rise_db=12.0)
    assert np.all(thr[d.steady] == -1.0) and np.all(thr[~d.steady] > 0)
    # 12 dB over a floor that is the noise's: sum(w^2) 2 sigma^2 scale^2, less what the mixer's truncation takes (11 %).
    # The median, since single bins rightly differ: the truncation's DC line at bins 0 and +-1 (no mean removal) and the
    # window's leakage of the tone into an unflagged neighbour.
    nominal = er.noise_floor(sr.DETECT_NFFT, rr.NOISE_SIGMA, 1.0 / 127.5)
    assert abs(np.median(thr[~d.steady]) / (10 ** 1.2 * nominal) - 1.0) < 0.25
    cleaned = er.excise(raw, thr, sr.DETECT_NFFT)
    s1, s2, skv = sr.sk(cleaned.out, sr.DETECT_NFFT, sr.DETECT_HOP, sr.DETECT_M)
    again = kurtosis.detect(sr.as_result(s1, s2, skv, sr.DETECT_NFFT, sr.DETECT_HOP, sr.DETECT_M), sr.SIGMAS)
    assert not again.flagged.any(), (amp, np.flatnonzero(again.flagged))
    # the GPU test scans the cleaned capture again: its cells keep the same distance from the band edges.  (The GPU
    # excisor's bytes may differ from these by 1 where a value lies within 2.2e-4 LSB of a rounding tie, 0.05 % of them:
    # a change of SK far below EDGE.)
    dist = sr.edge_distance(skv, sr.DETECT_M)
    print(f"tone of {amp} LSB: cleaned, smallest distance to a band edge {dist:.2e}")
    assert dist >= sr.EDGE, (amp, dist)


# ------------------------------------------------------------------------------------------------ GPU inputs
def test_no_gpu_input_has_a_cell_near_a_band_edge():
    """tests/skurt/test_round6_gpu.py expects the flags of the restatement from the device; that is only fair where
    float32 cannot carry a cell across a band edge.  Seeds are chosen so that every cell keeps a distance of 1e-3."""
    worst = {case: sr.edge_distance(sr.detect_reference(case)[1], sr.DETECT_M) for case in sr.CASES}
    for amp in sr.EXCISE_AMPS:
        worst[f"tone {amp}"] = sr.edge_distance(sr.sk(sr.excise_capture(amp), sr.DETECT_NFFT, sr.DETECT_HOP, sr.DETECT_M)[2], sr.DETECT_M)
    print("smallest distance of a cell's SK to a band edge:", {k: f"{v:.2e}" for k, v in worst.items()})
    bad = {k: v for k, v in worst.items() if v < sr.EDGE}
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ the Python layer
class HostLib(host_lib.HostLib):
    """gj_sk_dev, which Device.spectral_kurtosis reaches, computed by the restatement on host memory (tests/host_lib.py)."""

    def gj_sk_dev(self, ctx, d_iq, nbytes, first, nfft, hop, frames_per_row, n_rows, d_s1, d_s2, d_sk):
        self.calls.append(("sk", first, nfft, hop, frames_per_row, n_rows))
        for addr, a in zip((d_s1, d_s2, d_sk), sr.sk(self.view(d_iq, nbytes), nfft, hop, frames_per_row, first, n_rows)):
            if addr:
                self.view(addr, n_rows * nfft, np.float32)[:] = a.reshape(-1)
        return 0


@pytest.fixture
def host_dev():
    dev = host_lib.host_device(HostLib())
    yield dev
    dev._ctx = None            # a Capture that outlives the test frees nothing


W_NFFT, W_HOP, W_M, W_FIRST, W_ROWS = 16, 5, 3, 2, 4
W_RAW = rr.parity_capture()[:2 * (W_FIRST + (W_ROWS * W_M - 1) * W_HOP + W_NFFT + 2 * W_HOP)]      # two frames short of a 5th row


def test_device_spectral_kurtosis_on_the_host_double(host_dev):
    lib = host_dev._lib
    want = [a.astype(np.float32) for a in sr.sk(W_RAW, W_NFFT, W_HOP, W_M, W_FIRST)]
    assert want[0].shape == (W_ROWS, W_NFFT) and gpsjam.sk_rows(W_RAW.size, W_FIRST, W_NFFT, W_HOP, W_M) == W_ROWS
    for n, (source, held) in enumerate(host_lib.sources(host_dev, W_RAW), 1):
        lib.calls.clear()
        uploads = gpsjam.Capture.uploads
        got = host_dev.spectral_kurtosis(source, W_NFFT, W_HOP, W_M, first_sample=W_FIRST)
        assert gpsjam.Capture.uploads == uploads + (source is W_RAW), "host bytes are uploaded once, a resident capture never"
        assert isinstance(got, gpsjam.SpectralKurtosis) and (got.nfft, got.hop, got.frames_per_row, got.first_sample) == (W_NFFT, W_HOP, W_M, W_FIRST)
        for have, ref in zip((got.s1, got.s2, got.sk), want):
            assert have.shape == (W_ROWS, W_NFFT) and have.tobytes() == ref.tobytes()
        assert host_lib.mallocs(lib) == [3 * 4 * W_ROWS * W_NFFT], "one buffer holds the three arrays"
        assert lib.calls[-1] == ("sk", W_FIRST, W_NFFT, W_HOP, W_M, W_ROWS) and host_dev.kernel_calls == {"spectral_kurtosis": n}
        assert set(lib.mem) == held, "every buffer of the call's own is freed"
    # the defaults: hop nfft, the range from sample 0; a given row count is taken as it is
    lib.calls.clear()
    part = host_dev.spectral_kurtosis(W_RAW, W_NFFT, frames_per_row=2, n_rows=2)
    assert lib.calls == [("malloc", 3 * 4 * 2 * W_NFFT), ("sk", 0, W_NFFT, W_NFFT, 2, 2)] and (part.hop, len(part)) == (W_NFFT, 2)
    for have, ref in zip((part.s1, part.s2, part.sk), sr.sk(W_RAW, W_NFFT, W_NFFT, 2, 0, 2)):
        assert have.tobytes() == ref.astype(np.float32).tobytes()
    assert not lib.mem and host_dev.kernel_calls == {"spectral_kurtosis": 3}


def test_device_spectral_kurtosis_refusals_and_the_empty_result(host_dev):
    lib = host_dev._lib
    host_lib.check_freed(host_dev, W_RAW, lambda cap: host_dev.spectral_kurtosis(cap, W_NFFT))
    # no row fits: an empty result with the call's geometry, and the library is not reached
    short = W_RAW[:2 * (W_FIRST + (W_M - 1) * W_HOP + W_NFFT - 1)]                     # one sample short of the first row
    for source, held in host_lib.sources(host_dev, short):
        empty = host_dev.spectral_kurtosis(source, W_NFFT, W_HOP, W_M, first_sample=W_FIRST)
        assert len(empty) == 0 and empty.s1.shape == empty.s2.shape == empty.sk.shape == (0, W_NFFT) and empty.sk.dtype == np.float32
        assert (empty.nfft, empty.hop, empty.frames_per_row, empty.first_sample) == (W_NFFT, W_HOP, W_M, W_FIRST)
        assert set(lib.mem) == held and host_dev.kernel_calls == {} and not host_lib.mallocs(lib)
    # ... unless the geometry is one the library refuses: that is left to the library
    lib.refuse("gj_sk_dev")
    host_lib.check_refused(host_dev, short, lambda s: host_dev.spectral_kurtosis(s, W_NFFT, W_HOP, 1, first_sample=40),
                           gpsjam.GpsJamError, host_lib.REFUSED_TEXT, counted="spectral_kurtosis")
    assert host_lib.mallocs(lib) == [3 * 4 * W_NFFT] * 2, "the buffer is never empty"
    lib.calls.clear()
    host_lib.check_refused(host_dev, W_RAW, lambda s: host_dev.spectral_kurtosis(s, W_NFFT, W_HOP, W_M), gpsjam.GpsJamError,
                           host_lib.REFUSED_TEXT, counted="spectral_kurtosis")
    assert host_lib.mallocs(lib) == [3 * 4 * W_ROWS * W_NFFT] * 2
    assert host_dev.kernel_calls == {"spectral_kurtosis": 4}
