"""CPU side of the chirp-rate search (gj_chirp_dev) and of classify_swept: the float64 restatement the GPU tests compare
with (tests/chirp_restatement.py) checked against the ridge's and against itself, the guarantee the GPU parity test
relies on (no frame of its inputs has a nearly tied rate or bin), the size of float32's error, the record layout, and the
classifier on restated records.  No GPU call is made."""
import ctypes as C

import numpy as np
import pytest

import chirp_restatement as cr
import gpsjam
import host_lib
import ridge_restatement as rr
from gpsjam import _ffi, classify

NFFT, HOP = cr.CLASSIFIER_NFFT, cr.CLASSIFIER_HOP


def as_scan(scan, rates, nfft=NFFT, hop=HOP, first_sample=0):
    rec = np.zeros(scan.records.size, gpsjam.CHIRP_DTYPE)
    for key in ("total", "peak", "second", "peak_bin", "rate_index"):
        rec[key] = scan.records[key]
    return gpsjam.ChirpScan(rec, nfft, hop, rates, first_sample, peaks=scan.peaks)


# ------------------------------------------------------------------------------------------------ C-ABI, host side
def test_record_layout_and_binding():
    assert C.sizeof(_ffi.ChirpFrame) == 24 == gpsjam.CHIRP_DTYPE.itemsize
    names = ("total", "peak", "second", "peak_bin", "rate_index", "reserved")
    assert [getattr(_ffi.ChirpFrame, k).offset for k in names] == [0, 4, 8, 12, 16, 20]
    assert [gpsjam.CHIRP_DTYPE.fields[k][1] for k in names] == [0, 4, 8, 12, 16, 20]
    # the first 16 bytes are the ridge's record
    assert [gpsjam.CHIRP_DTYPE.fields[k] for k in names[:4]] == [gpsjam.RIDGE_DTYPE.fields[k] for k in names[:4]]
    assert len(_ffi.SIGNATURES["gj_chirp_dev"][1]) == 13 and _ffi.SIGNATURES["gj_chirp_dev"][1][-2:] == [C.c_void_p, C.c_void_p]
    assert hasattr(_ffi.load(), "gj_chirp_dev")
    assert _ffi.GJ_VERSION == 150 and _ffi.GJ_CHIRP_MAX_RATES == 256
    for name in ("chirp", "chirp_dev"):
        assert callable(getattr(gpsjam.Device, name))
    assert callable(classify.classify_swept) and callable(classify.characterise_swept)


def test_chirp_scan_object():
    rec = np.zeros(6, gpsjam.CHIRP_DTYPE)
    rec["total"], rec["peak"] = 4.0, np.arange(6)
    rec["peak_bin"] = [0, 1, 127, 128, 250, 255]
    rec["rate_index"] = [0, 1, 2, 3, 4, 4]
    peaks = np.arange(30, dtype=np.float32).reshape(6, 5)
    s = gpsjam.ChirpScan(rec, 256, 100, (-4, 2, 5), first_sample=7, guard=3, peaks=peaks)
    assert len(s) == 6 and s.rates == (-4, 2, 5)
    np.testing.assert_array_equal(s.rate, [-4, -2, 0, 2, 4, 4])
    np.testing.assert_allclose(s.sweep_hz_per_s(2.048e6), np.array([-4, -2, 0, 2, 4, 4]) * 64e6)
    # bin + q / 2, wrapped: 0 - 2 = -2, 1 - 1 = 0, 127, 128 + 1 = 129 -> -127, 250 + 2 = 252 -> -4, 255 + 2 = 257 -> 1
    np.testing.assert_allclose(s.centre_freq_hz(2.048e6), np.array([-2, 0, 127, -127, -4, 1]) * 8000.0)
    np.testing.assert_allclose(s.concentration, np.arange(6) / 4.0)
    part = s[2:5]
    assert (part.first_sample, part.hop, part.nfft, part.guard, part.rates, len(part)) == (207, 100, 256, 3, (-4, 2, 5), 3)
    np.testing.assert_array_equal(part.peaks, peaks[2:5])
    assert gpsjam.ChirpScan(rec, 256, 100, (0, 1, 5)).peaks is None
    with pytest.raises(ValueError):
        s[::2]
    with pytest.raises(TypeError):
        s[3]


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("nfft", [16, 1024, 4096])
def test_single_rate_zero_is_the_ridge(nfft):
    raw = cr.parity_capture(nfft)
    for first in (0, 1):
        hop = cr.parity_hop(nfft)
        scan = cr.chirp_scan(raw, nfft, hop, (0, 1, 1), first)
        want, margin = rr.ridge(raw, nfft, hop, first)
        assert not scan.records["rate_index"].any()
        for key in ("total", "peak", "second", "peak_bin"):
            np.testing.assert_array_equal(scan.records[key], want[key])
        np.testing.assert_array_equal(scan.peaks[:, 0], want["peak"])
        np.testing.assert_array_equal(scan.bin_margin, margin)


@pytest.mark.parametrize("nfft", [16, 64, 1024])
def test_the_matching_rate_makes_a_tone_of_a_sweep(nfft):
    """x[n] = exp(i pi q n^2 / N^2 + 2 pi i k0 n / N): at rate q the frame that starts at n = 0 is the tone k0 again, with
    the Hann tone's 2/3 of the power in bin k0 -- the start frequency; no other rate of the grid does as well."""
    for q, k0 in ((5, 3), (-7, nfft // 2 - 2), (nfft, 1), (nfft * nfft // 2, 4)):
        n = np.arange(nfft)
        x = 0.7 * np.exp(1j * np.pi * q * n * n / nfft ** 2 + 2j * np.pi * k0 * n / nfft)
        half = nfft * nfft // 2
        rates = (min(max(q - 3, -half), half - 6), 1, 7)     # seven rates around q, inside the limits
        scan = cr.chirp_scan_of(x, nfft, nfft, rates, n_frames=1)
        assert cr.rate_values(rates)[scan.records["rate_index"][0]] == q
        assert scan.records["peak_bin"][0] == k0
        np.testing.assert_allclose(scan.records["peak"] / scan.records["total"], 2.0 / 3.0, rtol=1e-9)
        assert scan.rate_margin[0] > 0.01
        # the integer phase reduction changes nothing but the size of the sine's argument
        m = np.exp(-1j * np.pi * q * n.astype(np.float64) ** 2 / nfft ** 2)
        assert np.max(np.abs(cr.dechirp(q, nfft) - m)) < 1e-7


def test_rates_are_independent_and_ties_take_the_smallest_rate():
    raw = cr.parity_capture(64)
    full = cr.chirp_scan(raw, 64, 69, (-3, 2, 5), 1, 40)
    for r, q in enumerate(cr.rate_values((-3, 2, 5))):
        one = cr.chirp_scan(raw, 64, 69, (q, 1, 1), 1, 40)
        np.testing.assert_array_equal(one.records["peak"], full.peaks[:, r])
    np.testing.assert_array_equal(full.records["peak"], full.peaks.max(axis=1))
    # silence: every rate gives 0, rate 0 and bin 0 win
    flat = cr.chirp_scan(np.full(2 * 64, 128, np.uint8), 16, 8, (-1, 1, 3), offset=128.0, scale=1 / 128.0)
    assert not flat.records["rate_index"].any() and not flat.records["peak_bin"].any() and not flat.records["peak"].any()
    assert np.all(flat.rate_margin == 1.0) and np.all(flat.bin_margin == 1.0)


# ------------------------------------------------------------------------------------------------ GPU inputs
def gpu_parity_cases():
    """Every (nfft, rate set, first sample, unpack convention) tests/chirp/test_round6_gpu.py compares with the restatement."""
    for nfft in cr.PARITY_NFFT:
        for rates in cr.parity_rate_sets(nfft):
            for first in (0, 1):
                yield nfft, rates, first, 127.5, 1.0 / 127.5
    yield 256, (-3, 2, 5), 1, 127.5, 1.0 / 127.5          # the per-rate identity and
    yield 256, (-3, 2, 5), 1, 128.0, 1.0 / 128.0          # the unpack-convention test


def test_no_gpu_input_has_a_nearly_tied_rate_or_bin():
    """The GPU test compares rate_index and peak_bin on EVERY frame; that is only fair where float32 cannot turn the
    order of the two best rates, or of the two largest bins at the best rate, round.  The bin margin is taken against
    every other bin, the neighbours included, which asks more than bins outside +-1 would."""
    bad = {}
    for nfft, rates, first, offset, scale in gpu_parity_cases():
        scan = cr.parity_reference(nfft, rates, first, 2, offset, scale)
        worst = (float(scan.rate_margin.min()), float(scan.bin_margin.min()))
        if min(worst) < cr.NEAR_TIE:
            bad[(nfft, rates, first, offset)] = worst
    assert not bad, bad


def test_float32_stays_within_the_gpu_tolerance():
    """The definition evaluated in float32 / complex64 against float64, on every GPU parity input: total and peak within
    rtol 1e-5.  The worst values are printed (profiles/NOTES_chirp.md records them)."""
    worst = {"total": 0.0, "peak": 0.0}
    for nfft, rates, first, offset, scale in gpu_parity_cases():
        want = cr.parity_reference(nfft, rates, first, 2, offset, scale)
        got = cr.chirp_scan(cr.parity_capture(nfft), nfft, cr.parity_hop(nfft), rates, first, None, 2, offset, scale, single=True)
        np.testing.assert_array_equal(got.records["rate_index"], want.records["rate_index"])
        np.testing.assert_array_equal(got.records["peak_bin"], want.records["peak_bin"])
        for key in worst:
            err = float(np.max(np.abs(got.records[key] - want.records[key]) / want.records[key]))
            worst[key] = max(worst[key], err)
        err = float(np.max(np.abs(got.peaks - want.peaks) / want.peaks))
        worst["peak"] = max(worst["peak"], err)
    print(f"float32 against float64: total {worst['total']:.3e}, peak {worst['peak']:.3e} (tolerance {cr.RTOL:.0e})")
    assert worst["total"] <= cr.RTOL and worst["peak"] <= cr.RTOL, worst


# ------------------------------------------------------------------------------------------------ the classifier
@pytest.fixture(scope="module")
def swept():
    """classify_swept on the restated records of a case's jammed half against its quiet half, computed once per case."""
    cache = {}

    def run(case):
        if case not in cache:
            raw = cr.classifier_capture(case)
            half = raw.size // 2
            quiet = cr.chirp_scan(raw[:half], NFFT, HOP, (0, 1, 1))
            busy = cr.chirp_scan(raw[half:], NFFT, HOP, cr.SWEPT_RATES)
            cache[case] = classify.classify_swept(as_scan(busy, cr.SWEPT_RATES), cr.FS, noise=as_scan(quiet, (0, 1, 1)))
        return cache[case]
    return run


def test_fast_chirp_is_a_chirp_with_its_rate(swept):
    res = swept("fast chirp")
    assert res.kind == "chirp", res
    print(f"fast chirp: {res.sweep_hz_per_s:.4g} Hz/s against {cr.FAST_SWEEP:.4g}, one unit is {cr.RATE_UNIT:.4g}")
    assert abs(res.sweep_hz_per_s - cr.FAST_SWEEP) <= cr.RATE_UNIT, res
    assert res.evidence["rate_resolution_hz_per_s"] == cr.RATE_UNIT and res.evidence["modal_rate"] in (15, 16)
    assert res.freq_hz is None and res.prf_hz is None and res.duty is None
    assert abs(res.jnr_db - 10 * np.log10(40.0 ** 2 / (2 * rr.NOISE_SIGMA ** 2))) < 1.0


def test_tone_noise_and_broadband_keep_their_kinds(swept):
    cw = swept("cw")
    assert cw.kind == "cw" and cw.evidence["modal_rate"] == 0, cw
    assert abs(cw.freq_hz - rr.TONE_HZ) <= rr.FREQ_TOL_HZ and cw.sweep_hz_per_s is None
    assert swept("none").kind == "none"
    bb = swept("broadband")
    assert bb.kind == "broadband" and bb.sweep_hz_per_s is None and not bb.evidence["dechirped_line"], bb
    assert abs(bb.jnr_db - rr.BROADBAND_JNR_DB) <= rr.JNR_TOL_DB
    assert swept("pulsed").kind == "pulsed"
    # the simulator-rate sweep of the ridge tests is 0.78 rate units: the grid's nearest rate, to one unit
    slow = swept("chirp")
    assert slow.kind == "chirp" and slow.evidence["modal_rate"] == 1
    assert abs(slow.sweep_hz_per_s - rr.CHIRP_RATE) <= cr.RATE_UNIT


def test_the_ridge_alone_reads_the_fast_chirp_as_broadband():
    """a sweep that crosses many bins inside one frame no longer concentrates.  classify on the
    ridge's restated records of the fast-chirp capture, checked once."""
    raw = cr.fast_chirp_capture()
    half = raw.size // 2
    quiet, _ = rr.ridge(raw[:half], NFFT, HOP)
    busy, _ = rr.ridge(raw[half:], NFFT, HOP)
    res = classify.classify(gpsjam.Ridge(busy.astype(gpsjam.RIDGE_DTYPE), NFFT, HOP), cr.FS, HOP, NFFT,
                            noise=gpsjam.Ridge(quiet.astype(gpsjam.RIDGE_DTYPE), NFFT, HOP))
    print(f"classify on the ridge of the fast chirp: {res.kind}, concentration {res.evidence['concentration']:.4f}, "
          f"line needs {max(0.5 * res.evidence['line_min'], 2 * res.evidence['noise_concentration']):.4f}")
    assert res.kind == "broadband", res
    assert res.sweep_hz_per_s is None


# ------------------------------------------------------------------------------------------------ the Python layer
class HostLib(host_lib.HostLib):
    """gj_chirp_dev, which Device.chirp reaches, computed by the restatement on host memory (tests/host_lib.py)."""

    def gj_chirp_dev(self, ctx, d_iq, nbytes, first, nfft, hop, n_frames, guard, rate_first, rate_step, n_rates, d_out, d_peaks):
        self.calls.append(("chirp", first, nfft, hop, n_frames, guard, rate_first, rate_step, n_rates, bool(d_peaks)))
        scan = cr.chirp_scan(self.view(d_iq, nbytes), nfft, hop, (rate_first, rate_step, n_rates), first, n_frames, guard)
        rec = self.view(d_out, n_frames, gpsjam.CHIRP_DTYPE)
        for key in ("total", "peak", "second", "peak_bin", "rate_index"):
            rec[key] = scan.records[key]
        if d_peaks:
            self.view(d_peaks, n_frames * n_rates, np.float32)[:] = scan.peaks.reshape(-1)
        return 0


@pytest.fixture
def host_dev():
    dev = host_lib.host_device(HostLib())
    yield dev
    dev._ctx = None            # a Capture that outlives the test frees nothing


W_NFFT, W_HOP, W_FIRST, W_FRAMES, W_RATES = 16, 5, 1, 10, (-2, 1, 5)
W_RAW = rr.parity_capture()[:2 * (W_FIRST + (W_FRAMES - 1) * W_HOP + W_NFFT + 3)]      # two samples short of an 11th frame


def test_device_chirp_on_the_host_double(host_dev):
    lib = host_dev._lib
    ref = cr.chirp_scan(W_RAW, W_NFFT, W_HOP, W_RATES, W_FIRST, guard=1)
    want = as_scan(ref, W_RATES, W_NFFT, W_HOP, W_FIRST)
    assert len(want) == W_FRAMES == gpsjam.ridge_frames(W_RAW.size, W_FIRST, W_NFFT, W_HOP) and want.rate_index.any()
    for n, (source, held) in enumerate(host_lib.sources(host_dev, W_RAW), 1):
        lib.calls.clear()
        uploads = gpsjam.Capture.uploads
        got = host_dev.chirp(source, W_NFFT, W_HOP, W_RATES, first_sample=W_FIRST, guard=1, want_peaks=True)
        assert gpsjam.Capture.uploads == uploads + (source is W_RAW), "host bytes are uploaded once, a resident capture never"
        assert isinstance(got, gpsjam.ChirpScan) and got.records.tobytes() == want.records.tobytes()
        assert (got.nfft, got.hop, got.first_sample, got.guard, got.rates) == (W_NFFT, W_HOP, W_FIRST, 1, W_RATES)
        assert got.peaks.shape == (W_FRAMES, 5) and got.peaks.tobytes() == want.peaks.tobytes()
        assert host_lib.mallocs(lib) == [24 * W_FRAMES, 4 * W_FRAMES * 5], "the records, then the peaks"
        assert lib.calls[-1] == ("chirp", W_FIRST, W_NFFT, W_HOP, W_FRAMES, 1, -2, 1, 5, True) and host_dev.kernel_calls == {"chirp": n}
        assert set(lib.mem) == held, "every buffer of the call's own is freed"
    # the defaults: hop nfft / 2, the one rate 0, guard 2, no peaks; a given frame count is taken as it is
    lib.calls.clear()
    part = host_dev.chirp(W_RAW, W_NFFT, n_frames=6)
    assert lib.calls == [("malloc", 24 * 6), ("chirp", 0, W_NFFT, W_NFFT // 2, 6, 2, 0, 1, 1, False)]
    assert part.peaks is None and (part.hop, part.guard, part.rates, len(part)) == (8, 2, (0, 1, 1), 6)
    assert part.records.tobytes() == as_scan(cr.chirp_scan(W_RAW, W_NFFT, 8, (0, 1, 1), 0, 6), (0, 1, 1)).records.tobytes()
    assert not lib.mem and host_dev.kernel_calls == {"chirp": 3}


def test_device_chirp_refusals_and_the_empty_result(host_dev):
    lib = host_dev._lib
    host_lib.check_freed(host_dev, W_RAW, lambda cap: host_dev.chirp(cap, W_NFFT))
    # no frame fits: an empty ChirpScan with the call's geometry, and the library is not reached
    for source, held in host_lib.sources(host_dev, W_RAW[:2 * (W_NFFT - 1)]):
        for want_peaks in (False, True):
            empty = host_dev.chirp(source, W_NFFT, W_HOP, W_RATES, guard=3, want_peaks=want_peaks)
            assert len(empty) == 0 and empty.records.dtype == gpsjam.CHIRP_DTYPE
            assert (empty.nfft, empty.hop, empty.guard, empty.rates) == (W_NFFT, W_HOP, 3, W_RATES)
            assert (empty.peaks.shape == (0, 5) and empty.peaks.dtype == np.float32) if want_peaks else empty.peaks is None
            assert set(lib.mem) == held and host_dev.kernel_calls == {} and not host_lib.mallocs(lib)
    # ... unless the geometry or the rate grid is one the library refuses: that is left to the library
    lib.refuse("gj_chirp_dev")
    host_lib.check_refused(host_dev, W_RAW[:2 * (W_NFFT - 1)], lambda s: host_dev.chirp(s, W_NFFT, rates=(0, 1, 257)),
                           gpsjam.GpsJamError, host_lib.REFUSED_TEXT, counted="chirp")
    assert host_lib.mallocs(lib) == [24] * 2, "a record buffer is never empty"
    lib.calls.clear()
    host_lib.check_refused(host_dev, W_RAW, lambda s: host_dev.chirp(s, W_NFFT, W_HOP, W_RATES, want_peaks=True), gpsjam.GpsJamError,
                           host_lib.REFUSED_TEXT, counted="chirp")
    assert host_lib.mallocs(lib) == [24 * W_FRAMES, 4 * W_FRAMES * 5] * 2
    assert host_dev.kernel_calls == {"chirp": 4}
