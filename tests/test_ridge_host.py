"""CPU side of the short-time spectral ridge (gj_ridge_dev) and of the jammer-kind classifier (gpsjam/classify.py):
the frame arithmetic of the C-ABI, the float64 restatement the GPU tests compare with (tests/ridge_restatement.py)
checked against itself, the classifier on the restatement's records, and the guarantee the GPU parity test relies on:
no input it uses has a frame whose peak is nearly tied.  No GPU call is made."""
import ctypes as C

import numpy as np
import pytest

import gpsjam
import host_lib
import ridge_restatement as rr
from gpsjam import _ffi, classify

NFFT, HOP = 256, 128


def as_ridge(rec, nfft=NFFT, hop=HOP, first_sample=0):
    return gpsjam.Ridge(rec.astype(gpsjam.RIDGE_DTYPE), nfft, hop, first_sample)


# ------------------------------------------------------------------------------------------------ C-ABI, host side
def test_ridge_frames_matches_the_loop_at_every_boundary():
    lib = _ffi.load()
    for nfft in (16, 48, 256, 4096):
        for hop in (1, 7, nfft // 2, nfft // 2 + 37, nfft, nfft + 5, 3 * nfft):
            lengths = {0, 1, 2 * nfft - 2, 2 * nfft - 1, 2 * nfft, 2 * nfft + 1, 2 * (nfft + hop) - 1, 2 * (nfft + hop),
                       2 * (nfft + hop) + 1, 2 * (nfft + 5 * hop) + 1, 2 * (nfft + 9 * hop) - 2, 40961}
            for nbytes in sorted(lengths):
                for first in (0, 1, 2, hop, nbytes // 2 - nfft, nbytes // 2 - nfft + 1, nbytes // 2, nbytes // 2 + 1, nbytes + 7):
                    if first < 0:
                        continue
                    want = rr.frames_that_fit(nbytes, first, nfft, hop)
                    assert lib.gj_ridge_frames(nbytes, first, nfft, hop) == want, (nbytes, first, nfft, hop)
                    assert gpsjam.ridge_frames(nbytes, first, nfft, hop) == want
    # impossible geometries
    assert lib.gj_ridge_frames(1 << 20, 0, 0, 8) == 0
    assert lib.gj_ridge_frames(1 << 20, 0, -16, 8) == 0
    assert lib.gj_ridge_frames(1 << 20, 0, 16, 0) == 0
    assert lib.gj_ridge_frames(1 << 20, 2 ** 64 - 8, 16, 8) == 0          # first_sample + nfft must not wrap
    assert lib.gj_ridge_frames(2 ** 64 - 1, 0, 16, 1) == (2 ** 63 - 1) - 16 + 1


def test_record_layout():
    assert C.sizeof(_ffi.RidgeFrame) == 16 == gpsjam.RIDGE_DTYPE.itemsize
    assert [(_ffi.RidgeFrame.total.offset, _ffi.RidgeFrame.peak.offset, _ffi.RidgeFrame.second.offset, _ffi.RidgeFrame.peak_bin.offset)] == [(0, 4, 8, 12)]
    assert [gpsjam.RIDGE_DTYPE.fields[k][1] for k in ("total", "peak", "second", "peak_bin")] == [0, 4, 8, 12]
    assert _ffi.SIGNATURES["gj_ridge_dev"][1][-1] is C.c_void_p and len(_ffi.SIGNATURES["gj_ridge_dev"][1]) == 9
    assert _ffi.GJ_VERSION == 150


def test_python_interface_is_there():
    for name in ("ridge", "ridge_dev"):
        assert callable(getattr(gpsjam.Device, name))
    assert classify.KINDS == ("none", "cw", "chirp", "pulsed", "broadband")
    assert classify.Interference._fields == ("kind", "jnr_db", "freq_hz", "sweep_hz_per_s", "prf_hz", "duty", "evidence")


def test_ridge_object_slices_by_frame():
    rec = np.zeros(10, gpsjam.RIDGE_DTYPE)
    rec["total"], rec["peak"] = 4.0, np.arange(10)
    rec["peak_bin"] = [0, 1, 127, 128, 129, 255, 3, 4, 5, 6]
    r = gpsjam.Ridge(rec, 256, 100, first_sample=7, guard=3)
    assert len(r) == 10 and len(r[2:5]) == 3
    s = r[2:5]
    assert (s.first_sample, s.hop, s.nfft, s.guard) == (207, 100, 256, 3)
    np.testing.assert_array_equal(s.peak_bin, [127, 128, 129])
    np.testing.assert_array_equal(s.freq_hz(2.048e6), [127 * 8000.0, -128 * 8000.0, -127 * 8000.0])
    np.testing.assert_allclose(r.concentration, np.arange(10) / 4.0)
    assert gpsjam.Ridge(np.zeros(2, gpsjam.RIDGE_DTYPE), 16, 8).concentration.tolist() == [0.0, 0.0]
    with pytest.raises(ValueError):
        r[::2]
    with pytest.raises(TypeError):
        r[3]


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("nfft", [16, 256, 4096])
def test_restatement_parseval(nfft):
    raw = rr.parity_capture()
    for hop, first in ((nfft // 2, 0), (nfft // 2 + 37, 1)):
        rec, _ = rr.ridge(raw, nfft, hop, first, 20)
        x = rr.unpack(raw)
        w = rr.hann(nfft)
        for f in (0, 7, 19):
            seg = x[first + f * hop:first + f * hop + nfft] * w
            np.testing.assert_allclose(rec["total"][f], nfft * np.sum(np.abs(seg) ** 2), rtol=1e-12)
            assert rec["second"][f] <= rec["peak"][f] <= rec["total"][f]


@pytest.mark.parametrize("nfft", [16, 64, 1024])
def test_restatement_tone_on_a_bin(nfft):
    n = 4 * nfft
    for b in (1, 3, nfft // 2 - 1, -1, -5, -(nfft // 2)):
        x = 0.7 * np.exp(2j * np.pi * b * np.arange(n) / nfft + 0.3j)
        rec2, margin = rr.ridge_of(x, nfft, nfft // 2 + 1, 1, None, 2)
        rec0, _ = rr.ridge_of(x, nfft, nfft // 2 + 1, 1, None, 0)
        assert rec2.size == (n - 1 - nfft) // (nfft // 2 + 1) + 1
        assert np.all(rec2["peak_bin"] == b % nfft)                        # FFT order: k >= N/2 is negative frequency
        np.testing.assert_allclose(rec2["peak"] / rec2["total"], 2.0 / 3.0, rtol=1e-12)
        np.testing.assert_allclose(rec2["peak"], (0.7 * nfft / 2) ** 2, rtol=1e-12)
        # the Hann main lobe is bins b-1, b, b+1 (1/4, 1, 1/4 of the peak): guard 0 sees a neighbour, guard 2 sees nothing
        np.testing.assert_allclose(rec0["second"] / rec0["peak"], 0.25, rtol=1e-9)
        assert np.all(rec2["second"] <= 1e-20 * rec2["peak"])
        np.testing.assert_allclose(margin, 0.75, rtol=1e-9)
        r = as_ridge(rec2, nfft, nfft // 2 + 1, 1)
        want_hz = b * rr.FS / nfft
        np.testing.assert_allclose(r.freq_hz(rr.FS), want_hz)


def test_restatement_ties_take_the_smallest_bin_and_silence_is_zero():
    rec, margin = rr.ridge(np.full(2 * 64, 128, np.uint8), 16, 8, 0, None, 2, 128.0, 1 / 128.0)
    assert rec.size == 7 and not rec["total"].any() and not rec["peak"].any() and not rec["second"].any() and not rec["peak_bin"].any()
    assert np.all(margin == 1.0)
    # a real cosine has two equal lines: the smaller bin index wins
    x = np.cos(2 * np.pi * 4 * np.arange(64) / 32)
    rec, margin = rr.ridge_of(x, 32, 16)
    assert np.all(rec["peak_bin"] == 4) and np.all(margin < 1e-9)


# ------------------------------------------------------------------------------------------------ the classifier
@pytest.mark.parametrize("case", rr.CASES)
def test_classifier_on_restated_records(case):
    """fs 2.048e6, nfft 256, hop 128, 2^18 samples: the first half noise of sigma 6.25 LSB, the second half noise plus
    the case's interferer, quantised as the reference's mixer does; classify(second half, noise=first half).

    The broadband jnr_db is compared with the issue's 10 log10((30^2 + 6.25^2) / 6.25^2) = 13.81 dB.  The estimate is
    14.04 dB: the mixer truncates toward zero, which takes 1 LSB off every negative value and with it 11 % of the power
    of sigma-6.25 noise but only 2.5 % of the sigma-30.6 sum, so the capture really holds 0.2 dB more contrast than the
    formula's ideal quantiser (floor measured 0.887 of 2 * 6.25^2, the jammed half 0.973 of 2 * 30.64^2)."""
    raw = rr.classifier_capture(case)
    half = raw.size // 2
    quiet, _ = rr.ridge(raw[:half], NFFT, HOP)
    busy, _ = rr.ridge(raw[half:], NFFT, HOP)
    res = classify.classify(as_ridge(busy), rr.FS, HOP, NFFT, noise=as_ridge(quiet))
    rr.check_interference(case, res)
    assert isinstance(res.evidence, dict) and res.evidence["frames"] == busy.size
    if case != "none":
        assert abs(res.jnr_db - rr.BROADBAND_JNR_DB) < 1.0 or case != "broadband"
        for key in ("floor", "excess", "on_fraction", "concentration", "second_over_peak", "modal_bin"):
            assert key in res.evidence
    if case in ("cw", "chirp", "pulsed"):
        # one line: the peak bin holds what a Hann-windowed tone must, and nothing rivals it outside the guard
        assert 0.5 * 0.48 * 0.9 < res.evidence["concentration"] <= 2.0 / 3.0 + 1e-6
        assert res.evidence["lines"] == "one"
    if case == "pulsed":
        assert res.freq_hz == 0.0                     # the carrier sits at 0 Hz: a detrend would have erased it


def test_classifier_without_quiet_frames_uses_the_percentile_floor():
    """The whole capture, no noise Ridge: the quiet half supplies the low percentile."""
    for case in rr.CASES:
        rec, _ = rr.ridge(rr.classifier_capture(case), NFFT, HOP)
        res = classify.classify(as_ridge(rec), rr.FS, HOP, NFFT)
        assert res.evidence["floor_from"] == "percentile"
        want = {"none": "none", "cw": "cw", "chirp": "chirp", "broadband": "broadband", "pulsed": "pulsed"}[case]
        assert res.kind == want, (case, res)
    assert classify.classify(as_ridge(rec[:0]), rr.FS, HOP, NFFT).kind == "none"


def test_thresholds_come_from_the_window_not_from_the_inputs():
    """sqrt(35/18) / sqrt(N) and (ln(N / 1.5) + 0.58) / N, checked on fresh Gaussian noise at sizes the other tests do not use."""
    rng = np.random.default_rng(1)
    for nfft in (64, 1024):
        x = rng.normal(size=200 * nfft) + 1j * rng.normal(size=200 * nfft)
        rec, _ = rr.ridge_of(x, nfft, nfft)                                  # disjoint frames: independent totals
        assert abs(np.std(rec["total"]) / np.mean(rec["total"]) / classify.total_rel_sigma(nfft) - 1.0) < 0.15
        assert abs(np.median(rec["peak"] / rec["total"]) / classify.noise_concentration(nfft) - 1.0) < 0.1
        assert classify.noise_concentration(nfft) < (np.log(nfft) + 0.58) * 1.5 / nfft


# ------------------------------------------------------------------------------------------------ GPU inputs
def test_no_gpu_input_has_a_nearly_tied_peak():
    """tests/ridge/test_round6_gpu.py compares peak_bin on EVERY frame; that is only fair where float32 cannot turn the
    order of the two largest bins round.  Seeds are chosen so that every frame of every input keeps a margin of 1e-4."""
    worst = {}
    for offset, scale in ((127.5, 1 / 127.5), (128.0, 1 / 128.0)):
        for nfft in rr.PARITY_NFFT:
            for hop in rr.parity_hops(nfft):
                for first in (0, 1):
                    _, margin = rr.parity_reference(nfft, hop, first, 2, offset, scale)
                    worst[(nfft, hop, first, offset)] = float(margin.min())
    for case in rr.CASES:
        _, margin = rr.ridge(rr.classifier_capture(case), NFFT, HOP)
        worst[case] = float(margin.min())
    bad = {k: v for k, v in worst.items() if v < rr.NEAR_TIE}
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ the Python layer
class HostLib(host_lib.HostLib):
    """gj_ridge_dev, which Device.ridge reaches, computed by the restatement on host memory (tests/host_lib.py)."""

    def gj_ridge_dev(self, ctx, d_iq, nbytes, first, nfft, hop, n_frames, guard, d_out):
        self.calls.append(("ridge", first, nfft, hop, n_frames, guard))
        rec, _ = rr.ridge(self.view(d_iq, nbytes), nfft, hop, first, n_frames, guard)
        out = self.view(d_out, n_frames, gpsjam.RIDGE_DTYPE)
        for key in gpsjam.RIDGE_DTYPE.names:
            out[key] = rec[key]
        return 0


@pytest.fixture
def host_dev():
    dev = host_lib.host_device(HostLib())
    yield dev
    dev._ctx = None            # a Capture that outlives the test frees nothing


W_NFFT, W_HOP, W_FIRST, W_FRAMES = 16, 5, 3, 12
W_RAW = rr.parity_capture()[:2 * (W_FIRST + (W_FRAMES - 1) * W_HOP + W_NFFT + 2)]      # two samples short of a 13th frame


def test_device_ridge_on_the_host_double(host_dev):
    lib = host_dev._lib
    want = rr.ridge(W_RAW, W_NFFT, W_HOP, W_FIRST)[0].astype(gpsjam.RIDGE_DTYPE)
    assert want.size == W_FRAMES == gpsjam.ridge_frames(W_RAW.size, W_FIRST, W_NFFT, W_HOP)
    for n, (source, held) in enumerate(host_lib.sources(host_dev, W_RAW), 1):
        lib.calls.clear()
        uploads = gpsjam.Capture.uploads
        got = host_dev.ridge(source, W_NFFT, W_HOP, first_sample=W_FIRST, guard=1)
        assert gpsjam.Capture.uploads == uploads + (source is W_RAW), "host bytes are uploaded once, a resident capture never"
        assert isinstance(got, gpsjam.Ridge) and (got.nfft, got.hop, got.first_sample, got.guard) == (W_NFFT, W_HOP, W_FIRST, 1)
        assert got.records.tobytes() == rr.ridge(W_RAW, W_NFFT, W_HOP, W_FIRST, guard=1)[0].astype(gpsjam.RIDGE_DTYPE).tobytes()
        assert got.total.tobytes() == want["total"].tobytes() and np.array_equal(got.peak_bin, want["peak_bin"])
        assert host_lib.mallocs(lib) == [16 * W_FRAMES], "one record buffer"
        assert lib.calls[-1] == ("ridge", W_FIRST, W_NFFT, W_HOP, W_FRAMES, 1) and host_dev.kernel_calls == {"ridge": n}
        assert set(lib.mem) == held, "every buffer of the call's own is freed"
    # the defaults: hop nfft / 2, guard 2, the range from sample 0; a given frame count is taken as it is
    lib.calls.clear()
    part = host_dev.ridge(W_RAW, W_NFFT, n_frames=7)
    assert lib.calls == [("malloc", 16 * 7), ("ridge", 0, W_NFFT, W_NFFT // 2, 7, 2)] and (part.hop, part.guard, len(part)) == (8, 2, 7)
    assert part.records.tobytes() == rr.ridge(W_RAW, W_NFFT, 8, 0, 7)[0].astype(gpsjam.RIDGE_DTYPE).tobytes()
    assert not lib.mem and host_dev.kernel_calls == {"ridge": 3}


def test_device_ridge_refusals_and_the_empty_result(host_dev):
    lib = host_dev._lib
    host_lib.check_freed(host_dev, W_RAW, lambda cap: host_dev.ridge(cap, W_NFFT))
    # no frame fits: an empty Ridge with the call's geometry, and the library is not reached
    for source, held in host_lib.sources(host_dev, W_RAW[:2 * (W_NFFT - 1)]):
        empty = host_dev.ridge(source, W_NFFT, W_HOP, guard=3)
        assert len(empty) == 0 and empty.records.dtype == gpsjam.RIDGE_DTYPE and (empty.nfft, empty.hop, empty.guard) == (W_NFFT, W_HOP, 3)
        assert set(lib.mem) == held and host_dev.kernel_calls == {} and not host_lib.mallocs(lib)
    # ... unless the geometry is one the library refuses: that is left to the library
    lib.refuse("gj_ridge_dev")
    host_lib.check_refused(host_dev, W_RAW[:2 * 7], lambda s: host_dev.ridge(s, 8), gpsjam.GpsJamError,
                           host_lib.REFUSED_TEXT, counted="ridge")
    host_lib.check_refused(host_dev, W_RAW, lambda s: host_dev.ridge(s, W_NFFT, n_frames=0), gpsjam.GpsJamError,
                           host_lib.REFUSED_TEXT, counted="ridge")
    assert host_lib.mallocs(lib) == [16] * 4, "a record buffer is never empty"
    assert host_dev.kernel_calls == {"ridge": 4}
