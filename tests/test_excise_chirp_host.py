"""CPU side of the chirp-domain excisor (gj_excise_chirp_dev, gj_chirp_rates_dev, Device.excise_chirp,
mitigate.clean_swept): the interface, the float64 restatement the GPU tests compare with
(tests/excise_chirp_restatement.py) checked against the definition's own consequences, the conditions on the GPU tests'
inputs, the Python layers on a host double of the library, and the end-to-end figures the GPU test's tolerances come
from.  No GPU call is made.

The tests under "the restatement", "GPU inputs" and "end to end" exercise tests/excise_chirp_restatement.py alone: they
check the yardstick against the definition's own consequences and do not cover the library.  The interface test and the
two tests on the host double run the package's code, and tests/excise_chirp/test_round6_gpu.py runs the kernels."""
import ctypes as C

import numpy as np
import pytest

import chirp_restatement as cr
import excise_chirp_restatement as xr
import excise_restatement as er
import gpsjam
import host_lib
from gpsjam import _ffi, classify, mitigate


# ------------------------------------------------------------------------------------------------ interface
def test_symbols_bindings_and_python_interface():
    lib = _ffi.load()
    assert len(_ffi.SIGNATURES["gj_excise_chirp_dev"][1]) == 10 and len(_ffi.SIGNATURES["gj_chirp_rates_dev"][1]) == 7
    for name in ("gj_excise_chirp_dev", "gj_chirp_rates_dev"):
        assert callable(getattr(lib, name))
    assert _ffi.GJ_VERSION == 150
    for name in ("excise_chirp", "excise_chirp_dev", "chirp_rates_dev"):
        assert callable(getattr(gpsjam.Device, name))
    assert mitigate.CleanedSwept._fields == mitigate.Cleaned._fields + ("rates", "sweep_hz_per_s", "swept")
    assert mitigate.Cleaned._fields == ("capture", "records", "threshold", "floor_from", "removed_share")
    # q0 = round(sweep nfft^2 / fs^2): one unit at 1024 points is 4 MHz/s, at 256 points 64 MHz/s
    assert mitigate.sweep_rate_units(xr.E2E_SWEEP, 1024, xr.FS) == xr.E2E_Q == 1002
    assert mitigate.sweep_rate_units(-xr.E2E_SWEEP, 1024, xr.FS) == -1002
    assert mitigate.sweep_rate_units(63 * 64e6, 1024, xr.FS) == 1008 and mitigate.sweep_rate_units(1.0e9, 256, xr.FS) == 16


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("nfft", [16, 64, 1024])
def test_zero_rates_and_whole_periods_are_the_plain_excisor(nfft):
    raw = xr.parity_capture(nfft)[:2 * (1 + 9 * nfft)]
    want = er.excise(raw, xr.parity_threshold(nfft), nfft, 1)
    nf = want.records.size
    for q in (0, 2 * nfft * nfft, -4 * nfft * nfft):
        got = xr.excise_chirp(raw, xr.parity_threshold(nfft), np.full(nf, q), nfft, 1)
        assert np.array_equal(got.out, want.out) and got.records.tobytes() == want.records.tobytes(), (nfft, q)
        assert np.array_equal(got.value, want.value)
    assert want.records["n_excised"].sum() > 0
    # 2 N^2 + 3 is the rate 3, to the bit; the complex64 factors are exactly (1, 0) at rate 0
    assert np.array_equal(xr.factors(2 * nfft * nfft + 3, nfft), xr.factors(3, nfft))
    assert np.array_equal(xr.factors(2 * nfft * nfft + 3, nfft, True), xr.factors(3, nfft, True))
    assert np.all(xr.factors(0, nfft, True) == 1.0) and np.all(xr.factors(-2 * nfft * nfft, nfft, True) == 1.0)


@pytest.mark.parametrize("nfft", xr.NFFT)
def test_all_ones_mask_returns_the_input_whatever_the_rates(nfft):
    raw = xr.parity_capture(nfft)
    for offset, scale in xr.CONVENTIONS:
        for first, n in ((0, 7 * nfft), (1, 5 * nfft + nfft // 2 + 3)):
            nf = er.frames_loop(n, nfft)
            for single in (False, True):
                ex = xr.excise_chirp(raw[:2 * (first + n)], np.full(nfft, np.inf), xr.parity_rates(nfft, nf), nfft, first, n,
                                     offset, scale, single)
                assert np.array_equal(ex.out, raw[2 * first:2 * (first + n)]), (nfft, offset, first, single)
                assert not ex.records["n_excised"].any() and not ex.records["removed"].any()
                assert np.min(er.tie_distance(ex.value)) > 0.49


@pytest.mark.parametrize("nfft", [64, 1024, 4096])
def test_translation_by_whole_hops_with_the_rates_moved_along(nfft):
    raw, h, first = xr.parity_capture(nfft), nfft // 2, xr.PARITY_FIRST
    long = xr.parity_reference(nfft)
    rates, nf = xr.parity_rates(nfft), long.records.size
    for k in (1, 3):
        sh = xr.excise_chirp(raw, xr.parity_threshold(nfft), rates[k:], nfft, first + k * h, xr.PARITY_SAMPLES - first - k * h)
        assert sh.records.tobytes() == long.records[k:].tobytes()
        assert sh.out[nfft:(nf - k) * nfft].tobytes() == long.out[(k + 1) * nfft:nf * nfft].tobytes()
    # a frame's result depends on its own rate: another rate on ONE frame changes that frame's record and no other
    other = rates.copy()
    other[5] += 7
    alt = xr.excise_chirp(raw, xr.parity_threshold(nfft), other, nfft, first)
    same = np.ones(nf, bool)
    same[5] = False
    assert alt.records[same].tobytes() == long.records[same].tobytes() and alt.records[5] != long.records[5]


def test_rate_picker_restatement_multiplies_in_float32():
    rec = np.zeros(8, gpsjam.CHIRP_DTYPE)
    minc = 0.1
    # a total whose product with 0.1 in float64, rounded once, is not the float32 product of the float32 values
    odd = next(t for t in range(3, 1000) if np.float32(0.1 * t) != np.float32(minc) * np.float32(t))
    total = np.array([1.0, 3.0, 0.0, 7.0, np.nan, 1e30, odd, 5.0], np.float32)
    need = np.float32(minc) * total
    rec["total"] = total
    rec["peak"] = need
    rec["peak"][1] = np.nextafter(need[1], np.float32(0))           # one ulp short
    rec["peak"][6] = np.float32(0.1 * odd)                            # the float64 product, rounded
    rec["rate_index"] = [0, 1, 2, 3, 4, 5, 6, 2 ** 31 - 1]
    got = xr.chirp_rates(rec, -5, 3, minc)
    assert got.dtype == np.int32
    wrap = ((-5 + (2 ** 31 - 1) * 3) & 0xFFFFFFFF)
    wrap = wrap - (1 << 32) if wrap >= 1 << 31 else wrap
    on6 = bool(rec["peak"][6] >= need[6])
    assert got.tolist() == [-5, 0, 0, 4, 0, 10, 13 if on6 else 0, wrap]
    assert rec["peak"][6] != need[6], "the case must tell a float64 product from the float32 one"


# ------------------------------------------------------------------------------------------------ GPU inputs
def test_gpu_inputs_keep_clear_of_ties():
    """tests/excise_chirp/test_round6_gpu.py holds the GPU to the restatement's mask on EVERY bin, to its bytes wherever the
    float64 value is further than TIE_BAND from a half-integer, and to exact rates from the picker.  That is fair only if
    no P_f[k] lies within NEAR_TIE of its threshold, no frame's peak / total within NEAR_TIE of MIN_CONCENTRATION, and few
    values lie in the band: at most TIE_SHARE_CAP."""
    assert xr.E32_CHIRP >= xr.E32_CHIRP_MEASURED and xr.TIE_BAND == 8 * xr.E32_CHIRP and xr.TIE_SHARE_CAP == 4 * xr.TIE_BAND
    assert xr.TIE_SHARE_CAP < 2e-3
    share, margin, conc, e32 = {}, {}, {}, 0.0
    for nfft in xr.NFFT:
        rates = xr.parity_rates(nfft)
        cyc = set(xr.rate_cycle(nfft))
        assert set(rates.tolist()) == cyc and len(cyc) == 8 and np.all(rates[1:] != rates[:-1])
        assert {0, xr.PARITY_Q[nfft], -xr.PARITY_Q[nfft], 1, -1, nfft * nfft // 2, -(nfft * nfft // 2), 2 * nfft * nfft + 3} == cyc
        for offset, scale in xr.CONVENTIONS:
            ref = xr.parity_reference(nfft, offset, scale)
            share[(nfft, offset)] = float(np.mean(er.tie_distance(ref.value) <= xr.TIE_BAND))
            margin[(nfft, offset)] = er.threshold_margin(ref.power, xr.parity_threshold(nfft, scale))
            by_rate = {q: int(ref.records["n_excised"][rates == q].sum()) for q in cyc}
            assert by_rate[xr.PARITY_Q[nfft]] > 0 and by_rate[0] > 0, "the de-chirped line and the plain tone must both be cut"
        conc[nfft] = xr.concentration_margin(xr.parity_scan(nfft).records)
    for nfft in xr.NFFT:                                             # the complex64 restatement, re-measured in full
        for offset, scale in xr.CONVENTIONS:
            a, b = xr.parity_reference(nfft, offset, scale), xr.parity_reference(nfft, offset, scale, single=True)
            e32 = max(e32, float(np.max(np.abs(a.value - b.value))))
    print(f"largest tie-band share {max(share.values()):.2e} (cap {xr.TIE_SHARE_CAP:.2e}), smallest threshold margin "
          f"{min(margin.values()):.2e}, smallest concentration margin {min(conc.values()):.2e}, E32 here {e32:.2e}")
    assert e32 <= xr.E32_CHIRP
    assert max(share.values()) <= xr.TIE_SHARE_CAP, share
    assert min(margin.values()) >= xr.NEAR_TIE, margin
    assert min(conc.values()) >= xr.NEAR_TIE, conc


@pytest.mark.parametrize("nfft", xr.REMOVAL_NFFT)
def test_restated_removal_is_complete_in_the_chirp_domain_only(nfft):
    raw, thr = xr.removal_capture(nfft), xr.removal_threshold(nfft)
    nf = er.frames_loop(raw.size // 2, nfft)
    assert nf == xr.REMOVAL_FRAMES and xr.REMOVAL_Q[nfft] % 2 == 0
    swept = xr.excise_chirp(raw, thr, np.full(nf, xr.REMOVAL_Q[nfft]), nfft)
    plain = er.excise(raw, thr, nfft)
    body, pbody = swept.out[swept.lo:swept.hi], plain.out[plain.lo:plain.hi]
    assert np.all(swept.records["n_excised"] == 3) and np.all((body == 127) | (body == 128))
    # what is left is the quantiser's error: |y| < 1 with room for the GPU's 1e-4, and the line far from the threshold
    assert np.max(np.abs(swept.value - 127.5)) < 0.75 and er.threshold_margin(swept.power, thr) > 0.9
    assert np.mean((pbody == 127) | (pbody == 128)) < 0.5


# ------------------------------------------------------------------------------------------------ the Python layers
class HostLib(host_lib.HostLib):
    """The library's entry points that Device.excise_chirp and mitigate.clean_swept reach, computed by the restatements
    on host memory (tests/host_lib.py)."""

    log_malloc = False       # ``calls`` holds the kernel calls alone

    def gj_chirp_dev(self, ctx, d_iq, nbytes, first, nfft, hop, n_frames, guard, rate_first, rate_step, n_rates, d_out, d_peaks):
        self.calls.append(("chirp", first, nfft, hop, n_frames, rate_first, rate_step, n_rates))
        scan = cr.chirp_scan(self.view(d_iq, nbytes), nfft, hop, (rate_first, rate_step, n_rates), first, n_frames, guard)
        rec = self.view(d_out, n_frames, gpsjam.CHIRP_DTYPE)
        for key in ("total", "peak", "second", "peak_bin", "rate_index"):
            rec[key] = scan.records[key]
        return 0

    def gj_chirp_rates_dev(self, ctx, d_scan, n_frames, rate_first, rate_step, minc, d_rate):
        self.calls.append(("rates", n_frames, rate_first, rate_step, minc))
        self.view(d_rate, n_frames, np.int32)[:] = xr.chirp_rates(self.view(d_scan, n_frames, gpsjam.CHIRP_DTYPE), rate_first,
                                                                  rate_step, minc)
        return 0

    def gj_excise_chirp_dev(self, ctx, d_iq, nbytes, first, n_samples, nfft, d_rate, d_thr, d_out, d_frames):
        nf = er.frames_loop(n_samples, nfft)
        rates = self.view(d_rate, nf, np.int32).copy()
        self.calls.append(("excise_chirp", first, n_samples, nfft, rates))
        ex = xr.excise_chirp(self.view(d_iq, nbytes), self.view(d_thr, nfft, np.float32), rates, nfft, first, n_samples)
        self.view(d_out, 2 * n_samples)[:] = ex.out
        if d_frames:
            rec = self.view(d_frames, nf, gpsjam.EXCISE_DTYPE)
            for key in ("total", "removed", "n_excised"):
                rec[key] = ex.records[key]
        return 0


@pytest.fixture
def host_dev():
    dev = host_lib.host_device(HostLib())
    yield dev
    dev._ctx = None            # a Capture that outlives the test frees nothing


def test_device_excise_chirp_on_the_host_double(host_dev):
    nfft = 64
    raw = xr.parity_capture(nfft)[:2 * (1 + 20 * nfft)]
    nf = gpsjam.excise_frames(raw.size // 2 - 1, nfft)
    rates, thr = xr.parity_rates(nfft, nf), xr.parity_threshold(nfft)
    want = xr.excise_chirp(raw, thr, rates, nfft, 1)
    cleaned, rec = host_dev.excise_chirp(raw, thr, rates, nfft=nfft, first_sample=1)
    assert isinstance(cleaned, gpsjam.Capture) and cleaned.nbytes == raw.size - 2 and rec.dtype == gpsjam.EXCISE_DTYPE
    assert np.array_equal(HostLib.view(cleaned.ptr, cleaned.nbytes), want.out)
    assert np.array_equal(rec["n_excised"], want.records["n_excised"]) and host_dev.kernel_calls == {"excise_chirp": 1}
    cleaned.free()
    # rates as a list, and resident: a device buffer is taken as it is, whatever its length
    d_rate = gpsjam.DevBuf(host_dev, 4 * nf).upload(rates)
    again, rec2 = host_dev.excise_chirp(raw, thr, d_rate, nfft=nfft, first_sample=1)
    assert np.array_equal(HostLib.view(again.ptr, again.nbytes), want.out) and rec2.tobytes() == rec.tobytes()
    again.free()
    d_rate.free()
    for bad in (rates[:-1], np.append(rates, 0)):
        with pytest.raises(ValueError, match="rates holds"):
            host_dev.excise_chirp(raw, thr, bad, nfft=nfft, first_sample=1)
    with pytest.raises(TypeError):
        host_dev.excise_chirp(raw, thr, rates.astype(np.float64), nfft=nfft, first_sample=1)
    with pytest.raises(ValueError, match="threshold holds"):
        host_dev.excise_chirp(raw, thr[:-1], rates, nfft=nfft, first_sample=1)
    assert host_dev.kernel_calls == {"excise_chirp": 2}, "a refused call counts nothing"


def test_device_excise_chirp_refusals_and_buffers(host_dev):
    nfft = 64
    raw = xr.parity_capture(nfft)[:2 * (1 + 20 * nfft)]
    n = raw.size // 2 - 1
    nf = gpsjam.excise_frames(n, nfft)
    rates, thr, lib = xr.parity_rates(nfft, nf), xr.parity_threshold(nfft), host_dev._lib
    lib.log_malloc = True
    call = lambda thr, rates: (lambda s: host_dev.excise_chirp(s, thr, rates, nfft=nfft, first_sample=1))
    host_lib.check_freed(host_dev, raw, call(thr, rates))
    host_lib.check_refused(host_dev, raw, call(thr[:-1], rates), ValueError, "threshold holds 63 values, nfft is 64")
    assert not host_lib.mallocs(lib), "the thresholds are checked in front of their upload"
    for bad in (rates[:-1], np.append(rates, 0)):
        host_lib.check_refused(host_dev, raw, call(thr, bad), ValueError,
                               f"rates holds {bad.size} values, the range has {nf} frames of 64 points")
    host_lib.check_refused(host_dev, raw, call(thr, rates.astype(np.float64)), TypeError, "rates must be integers")
    assert host_lib.mallocs(lib) == [4 * nfft] * 6, "the thresholds were on the device by then, and are freed"
    assert host_dev.kernel_calls == {}
    # the buffers of a call that goes through: thresholds, rates, output, records; all but the output are freed
    for k, (source, held) in enumerate(host_lib.sources(host_dev, raw), 1):
        lib.calls.clear()
        uploads = gpsjam.Capture.uploads
        cleaned, rec = call(thr, rates.tolist())(source)
        assert gpsjam.Capture.uploads == uploads + (source is raw), "host bytes are uploaded once; the cleaned capture is no upload"
        assert host_lib.mallocs(lib) == [4 * nfft, 4 * nf, 2 * n, 16 * nf] and rec.size == nf and cleaned.nbytes == 2 * n
        assert set(lib.mem) == held | {cleaned.ptr} and host_dev.kernel_calls == {"excise_chirp": k}
        cleaned.free()
    # what the library refuses: everything is allocated by then, and freed
    lib.calls.clear()
    lib.refuse("gj_excise_chirp_dev")
    host_lib.check_refused(host_dev, raw, call(thr, rates), gpsjam.GpsJamError, host_lib.REFUSED_TEXT, counted="excise_chirp")
    assert host_lib.mallocs(lib) == [4 * nfft, 4 * nf, 2 * n, 16 * nf] * 2
    # a range shorter than a frame has no frame: no rate is wanted, and the buffers are never empty
    lib.calls.clear()
    host_lib.check_refused(host_dev, raw, lambda s: host_dev.excise_chirp(s, thr, [], nfft=nfft, n_samples=nfft - 1), gpsjam.GpsJamError,
                           host_lib.REFUSED_TEXT, counted="excise_chirp")
    assert host_lib.mallocs(lib) == [4 * nfft, 4, 2 * (nfft - 1), 16] * 2 and host_dev.kernel_calls == {"excise_chirp": 6}


def test_clean_swept_on_the_host_double(host_dev, monkeypatch):
    nfft = 256
    q = 12
    sweep = q * (xr.FS / nfft) ** 2
    n = 40 * nfft
    rng = np.random.default_rng(9)
    import ridge_restatement as rr
    z = rr._noise(rng, n, 6.25).astype(np.complex128)
    z[n // 2:] += 50.0 * np.exp(1j * np.pi * q * (np.arange(n - n // 2) / nfft) ** 2)
    raw = rr.quantise(z)
    thr = er.parity_threshold(nfft)
    lib = host_dev._lib
    res = mitigate.clean_swept(host_dev, raw, nfft=nfft, sweep_hz_per_s=sweep * 1.004, rate_span=3, threshold=thr)
    try:
        nf = gpsjam.excise_frames(n, nfft)
        kinds = [c[0] for c in lib.calls]
        assert kinds == ["chirp", "rates", "excise_chirp"] and host_dev.kernel_calls == {"excise_chirp": 1}
        assert lib.calls[0][1:] == (0, nfft, nfft // 2, nf, q - 3, 1, 7), "the grid is q0 - span .. q0 + span at hop nfft / 2"
        assert lib.calls[1][1:4] == (nf, q - 3, 1) and lib.calls[1][4] == pytest.approx(0.1)
        assert isinstance(res, mitigate.CleanedSwept) and res.swept and res.floor_from == "given"
        assert res.sweep_hz_per_s == sweep * 1.004 and res.rates.dtype == np.int32 and res.rates.size == nf == res.records.size
        assert np.array_equal(res.rates, lib.calls[2][4])
        half = nf // 2
        assert not res.rates[:half - 2].any() and np.all(res.rates[half + 1:] == q)
        want = xr.excise_chirp(raw, thr, res.rates, nfft)
        assert np.array_equal(HostLib.view(res.capture.ptr, res.capture.nbytes), want.out)
        assert 0.5 < res.removed_share < 1.0
    finally:
        res.capture.free()
    assert not lib.mem, "every buffer but the result is freed"

    # not a chirp: exactly what clean does, and no call of the chirp-domain excisor
    lib.calls.clear()
    seen = {}

    def fake_characterise(dev, capture, fs=2.048e6, nfft=256, max_sweep_hz_per_s=4.096e9, **onset_args):
        seen["characterise"] = dict(fs=fs, max_sweep_hz_per_s=max_sweep_hz_per_s, **onset_args)
        return classify.Interference("cw", 10.0, 1e5, None, None, None, {})

    def fake_clean(dev, capture, nfft=1024, rise_db=12.0, fs=2.048e6, threshold=None, **onset_args):
        seen["clean"] = dict(nfft=nfft, rise_db=rise_db, fs=fs, threshold=threshold, **onset_args)
        return mitigate.Cleaned("the capture", np.zeros(5, gpsjam.EXCISE_DTYPE), "thr", "quiet part", 0.25)

    monkeypatch.setattr(classify, "characterise_swept", fake_characterise)
    monkeypatch.setattr(mitigate, "clean", fake_clean)
    res = mitigate.clean_swept(host_dev, raw, nfft=512, rise_db=9.0, fs=1.0e6, max_sweep_hz_per_s=2e9, window=500)
    assert seen["characterise"] == dict(fs=1.0e6, max_sweep_hz_per_s=2e9, window=500)
    assert seen["clean"] == dict(nfft=512, rise_db=9.0, fs=1.0e6, threshold=None, window=500)
    assert res[:5] == ("the capture", res.records, "thr", "quiet part", 0.25) and res.records.size == 5
    assert not res.swept and res.sweep_hz_per_s is None and res.rates.dtype == np.int32 and not res.rates.any() and res.rates.size == 5
    assert not lib.calls and not lib.mem


# ------------------------------------------------------------------------------------------------ end to end
def test_end_to_end_on_the_cpu_gives_the_gpu_tests_tolerances():
    """The restated chain on xr.e2e_capture(): the rate as characterise_swept reports it (the nearest integer at 256 points),
    the search over q0 +- RATE_SPAN at 1024 points, the picker at MIN_CONCENTRATION, the excisor; C/N0 by the oracle's
    acquisition.  Shows that the defaults 8 and 0.1 hold here, and re-measures E2E_CPU_LOSS_DB and E2E_CPU_GAP_DB."""
    from oracle import gpsjam_oracle as orc
    jammed, free = xr.e2e_capture(True), xr.e2e_capture(False)
    assert np.array_equal(free, er.e2e_capture(None))
    nfft, lead = xr.E2E_NFFT, er.E2E_LEAD
    at256 = xr.E2E_SWEEP / (xr.FS / 256) ** 2
    assert abs(at256 - np.floor(at256) - 0.5) >= 0.125 and abs(xr.E2E_SWEEP - 4e9) < 1e8
    # the search at 256 points over the jammed part: the median rate is the nearest integer
    s256 = cr.chirp_scan(jammed, 256, 128, (-66, 1, 133), lead, (er.E2E_AFTER - 256) // 128 + 1)
    median = float(np.median(-66 + s256.records["rate_index"]))
    assert median == round(at256) == 63
    q0 = mitigate.sweep_rate_units(median * (xr.FS / 256) ** 2, nfft, xr.FS)
    assert abs(q0 - xr.E2E_Q) <= xr.RATE_SPAN, "a rate span of 8 at 1024 points is half a unit at 256 points"
    nf = er.frames_loop(jammed.size // 2, nfft)
    scan = cr.chirp_scan(jammed, nfft, nfft // 2, (q0 - xr.RATE_SPAN, 1, 2 * xr.RATE_SPAN + 1), 0, nf)
    rates = xr.chirp_rates(scan.records, q0 - xr.RATE_SPAN, 1, xr.MIN_CONCENTRATION)
    conc = scan.records["peak"] / scan.records["total"]
    quiet, on = lead // (nfft // 2) - 1, lead // (nfft // 2)       # frames that end in front of the onset; first frame behind it
    print(f"q0 {q0}; concentration: lead-in at most {conc[:quiet].max():.3f}, jammed at least {conc[on:].min():.3f}; "
          f"rates {rates[on:].min()} .. {rates[on:].max()}")
    assert not rates[:quiet].any() and np.all(rates[on:] != 0) and np.all(np.abs(rates[on:] - xr.E2E_Q) <= 2)
    assert conc[:quiet].max() < 0.5 * xr.MIN_CONCENTRATION and conc[on:].min() > 1.5 * xr.MIN_CONCENTRATION
    thr = xr.e2e_flat_threshold()
    swept, plain = xr.excise_chirp(jammed, thr, rates, nfft), er.excise(jammed, thr, nfft)
    cn0 = {}
    for name, raw in (("free", free), ("swept", swept.out), ("plain", plain.out)):
        res = [orc.acq_search(raw, lead, prn)[0] for prn, *_ in er.E2E_SATS]
        cn0[name] = np.array([r["cn0"] for r in res])
        print(name, " ".join(f"{r['cn0']:.2f}{'' if r['acquired'] else '(not acquired)'}" for r in res))
        if name != "plain":
            assert all(r["acquired"] for r in res)
    loss, gap = cn0["free"] - cn0["swept"], cn0["swept"] - cn0["plain"]
    print(f"loss against jammer-free {np.round(loss, 2)} dB, advantage over the plain excisor {np.round(gap, 2)} dB")
    assert loss.max() <= xr.E2E_CPU_LOSS_DB + 0.005 and gap.min() >= xr.E2E_CPU_GAP_DB - 0.005
    assert xr.E2E_CN0_TOL_DB == 2.0 * xr.E2E_CPU_LOSS_DB and xr.E2E_MIN_GAP_DB == 0.5 * xr.E2E_CPU_GAP_DB
