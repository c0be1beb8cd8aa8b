"""CPU side of the frequency-domain excisor (gj_excise_dev, gpsjam/mitigate.py): the frame arithmetic of the C-ABI, the
record layout, the float64 restatement the GPU tests compare with (tests/excise_restatement.py) checked against the
definition's own consequences, the floor arithmetic of mitigate, and the two conditions on the GPU tests' inputs:
few excised components inside the rounding-tie band, and no bin power near its threshold.  No GPU call is made."""
import ctypes as C

import numpy as np
import pytest

import excise_restatement as er
import gpsjam
import host_lib
import ridge_restatement as rr
from gpsjam import _ffi, mitigate


# ------------------------------------------------------------------------------------------------ C-ABI, host side
def test_excise_frames_matches_the_loop_at_every_boundary():
    lib = _ffi.load()
    for nfft in (16, 32, 256, 4096):
        h = nfft // 2
        lengths = {0, 1, nfft - 1, nfft, nfft + 1, nfft + h - 1, nfft + h, nfft + h + 1, nfft + 5 * h - 1, nfft + 5 * h,
                   nfft + 9 * h + 1, 40961}
        for n in sorted(lengths):
            want = er.frames_loop(n, nfft)
            assert lib.gj_excise_frames(n, nfft) == want == gpsjam.excise_frames(n, nfft), (n, nfft)
            if want:
                # what the kernel's edge copy relies on: the tail behind the last whole hop is h .. 2h - 1 samples
                assert h <= n - want * h < 2 * h
    assert lib.gj_excise_frames(1 << 20, 0) == 0
    assert lib.gj_excise_frames(1 << 20, -16) == 0
    assert lib.gj_excise_frames(2 ** 64 - 1, 16) == (2 ** 64 - 1 - 16) // 8 + 1
    assert gpsjam.excise_frames(-1, 16) == 0


def test_record_layout_and_python_interface():
    assert C.sizeof(_ffi.ExciseFrame) == 16 == gpsjam.EXCISE_DTYPE.itemsize
    assert [getattr(_ffi.ExciseFrame, k).offset for k in ("total", "removed", "n_excised", "reserved")] == [0, 4, 8, 12]
    assert [gpsjam.EXCISE_DTYPE.fields[k][1] for k in ("total", "removed", "n_excised", "reserved")] == [0, 4, 8, 12]
    assert len(_ffi.SIGNATURES["gj_excise_dev"][1]) == 9 and len(_ffi.SIGNATURES["gj_excise_frames"][1]) == 2
    assert _ffi.GJ_VERSION == 150
    for name in ("excise", "excise_dev"):
        assert callable(getattr(gpsjam.Device, name))
    assert callable(gpsjam.Capture.from_device)
    for name in ("floor_from_psd", "thresholds", "clean", "main"):
        assert callable(getattr(mitigate, name))
    assert mitigate.Cleaned._fields == ("capture", "records", "threshold", "floor_from", "removed_share")


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("nfft", er.NFFT)
def test_restatement_identity_is_byte_exact(nfft):
    raw = er.parity_capture()
    for offset, scale in er.CONVENTIONS:
        for first, n in ((0, None), (1, 5 * nfft + nfft // 2 + 3)):
            for thr in (np.full(nfft, np.inf), np.full(nfft, np.nan)):
                ex = er.excise(raw[:2 * (first + 9 * nfft)], thr, nfft, first, n, offset, scale)
                want = raw[2 * first:2 * (first + (n if n else 9 * nfft))]
                assert np.array_equal(ex.out, want)
                assert not ex.records["n_excised"].any() and not ex.records["removed"].any()
                # periodic Hann at hop N/2 sums to one: the values are the input's, far from any rounding tie
                assert np.min(er.tie_distance(ex.value)) > 0.49


@pytest.mark.parametrize("nfft", [16, 64, 1024])
def test_restatement_notch_takes_a_tone_on_a_bin_and_leaves_the_noise(nfft):
    n, b = 12 * nfft, 3
    rng = np.random.default_rng(5)
    noise = rr._noise(rng, n, 4.0).astype(np.complex128)
    z = noise + rr.tone(n, b * er.FS / nfft, 60.0)
    thr = np.full(nfft, np.inf, np.float32)
    thr[[b - 1, b, b + 1]] = -1.0
    jam, ref = er.excise(rr.quantise(z), thr, nfft), er.excise(rr.quantise(noise), thr, nfft)
    assert np.all(jam.records["n_excised"] == 3)
    # a Hann-windowed tone on a bin lives in b - 1, b, b + 1 alone: what is left is the noise with the same notch
    # (the quantiser's error on noise + tone differs from its error on the noise: a few LSB, not the tone's 60)
    d = jam.value - ref.value
    assert np.sqrt(np.mean(d ** 2)) < 1.0 and np.max(np.abs(d)) < 4.0
    assert np.sqrt(np.mean((jam.value - 127.5) ** 2)) < 1.3 * 4.0
    np.testing.assert_allclose(jam.records["removed"] / jam.records["total"], 1.0, atol=0.05)


@pytest.mark.parametrize("nfft", [16, 256, 4096])
def test_restatement_all_bins_notched_gives_the_offset(nfft):
    raw = er.parity_capture()[:2 * 8 * nfft + 2 * 5]
    for offset, scale in er.CONVENTIONS:
        ex = er.excise(raw, np.full(nfft, -1.0), nfft, 1, None, offset, scale)
        assert np.all(ex.records["n_excised"] == nfft)
        np.testing.assert_allclose(ex.records["removed"], ex.records["total"], rtol=1e-12)
        assert np.all(ex.out[ex.lo:ex.hi] == int(np.rint(np.float32(offset))))     # 127.5 -> 128 (half to even), 128 -> 128
        src = raw[2:]
        assert np.array_equal(ex.out[:ex.lo], src[:ex.lo]) and np.array_equal(ex.out[ex.hi:], src[ex.hi:]) and ex.out.size == src.size


def test_restatement_clamps():
    for nfft in er.CLAMP_NFFT:
        ex = er.excise(er.clamp_capture(), er.clamp_threshold(nfft), nfft)
        assert ex.value.max() > 255.0 + 20.0 and ex.value.min() < -20.0          # the 4/pi fundamental overshoots
        body = ex.out[ex.lo:ex.hi]
        assert body.max() == 255 and body.min() == 0
        assert np.all(body[ex.value > 255.5] == 255) and np.all(body[ex.value < -0.5] == 0)


# ------------------------------------------------------------------------------------------------ mitigate's floor
@pytest.mark.parametrize("nfft", [64, 1024])
def test_floor_from_psd_matches_the_restatement_on_white_noise(nfft):
    """K2's row is mean |FFT(w (x - mean))|^2 / (fs sum w^2) on normalised samples; floor_from_psd must give back the
    restatement's mean P on every bin the mean removal does not touch, and patch the three it does."""
    from oracle import gpsjam_oracle as orc
    sigma, scale = 10.0, 1.0 / 127.5
    rng = np.random.default_rng(8)
    raw = rr.quantise(rr._noise(rng, 400 * nfft, sigma))
    ex = er.excise(raw, np.full(nfft, np.inf), nfft)
    mean_p = ex.power.mean(axis=0)
    z = (er.unpack_lsb(raw) * scale).astype(np.complex64)
    psd = orc.welch_twosided_c64(z, er.FS, nfft)
    floor = mitigate.floor_from_psd(psd, er.FS, nfft)
    keep = np.ones(nfft, bool)
    keep[[0, 1, nfft - 1]] = False
    # the same segments but for each one's mean, which moves a bin outside 0 and +-1 by nothing
    np.testing.assert_allclose(floor[keep], mean_p[keep], rtol=1e-4)
    assert floor[0] == floor[1] == floor[nfft - 1] == max(floor[2], floor[nfft - 2])
    assert abs(np.median(floor) / er.noise_floor(nfft, sigma, scale) - 1.0) < 0.1
    # several rows are averaged
    two = mitigate.floor_from_psd(np.stack([psd, 3.0 * psd]), er.FS, nfft)
    np.testing.assert_allclose(two, 2.0 * floor, rtol=1e-6)
    assert mitigate.hann_power(nfft) == pytest.approx(3.0 * nfft / 8.0, rel=1e-12)


# ------------------------------------------------------------------------------------------------ GPU inputs
def test_gpu_inputs_keep_clear_of_rounding_ties_and_of_their_thresholds():
    """tests/excise/test_round6_gpu.py holds the GPU to the restatement's bytes wherever the float64 value is further
    than TIE_BAND from a half-integer, and to the restatement's mask on EVERY bin.  That is fair only if few values lie
    in the band (at most 1 %) and no P_f[k] lies within NEAR_TIE of its threshold."""
    assert er.E32 >= er.E32_MEASURED and er.TIE_BAND == 8 * er.E32
    share, margin, e32 = {}, {}, 0.0
    for offset, scale in er.CONVENTIONS:
        for nfft in er.NFFT:
            ref = er.parity_reference(nfft, offset, scale)
            share[(nfft, offset)] = float(np.mean(er.tie_distance(ref.value) <= er.TIE_BAND))
            margin[(nfft, offset)] = er.threshold_margin(ref.power, er.parity_threshold(nfft, scale))
            assert ref.records["n_excised"].sum() > 0, "the parity input must excise something at every size"
    for nfft in (16, 1024, 4096):                                  # the complex64 restatement, re-measured where it is cheap
        a, b = er.parity_reference(nfft), er.parity_reference(nfft, single=True)
        e32 = max(e32, float(np.max(np.abs(a.value - b.value))))
    for nfft in er.CLAMP_NFFT:
        ref = er.excise(er.clamp_capture(), er.clamp_threshold(nfft), nfft)
        share[("clamp", nfft)] = float(np.mean(er.tie_distance(ref.value) <= er.TIE_BAND))
    print(f"largest tie-band share {max(share.values()):.2e}, smallest threshold margin {min(margin.values()):.2e}, E32 here {e32:.2e}")
    assert e32 <= er.E32
    assert max(share.values()) <= 0.01, share
    assert min(margin.values()) >= er.NEAR_TIE, margin


# ------------------------------------------------------------------------------------------------ the Python layers
class HostLib(host_lib.HostLib):
    """gj_excise_dev, which Device.excise and mitigate.clean reach, computed by the restatement on host memory
    (tests/host_lib.py)."""

    def gj_excise_dev(self, ctx, d_iq, nbytes, first, n_samples, nfft, d_thr, d_out, d_frames):
        self.calls.append(("excise", first, n_samples, nfft))
        ex = er.excise(self.view(d_iq, nbytes), self.view(d_thr, nfft, np.float32), nfft, first, n_samples)
        self.view(d_out, 2 * n_samples)[:] = ex.out
        if d_frames:
            rec = self.view(d_frames, ex.records.size, gpsjam.EXCISE_DTYPE)
            for key in ("total", "removed", "n_excised"):
                rec[key] = ex.records[key]
        return 0


@pytest.fixture
def host_dev():
    dev = host_lib.host_device(HostLib())
    yield dev
    dev._ctx = None            # a Capture that outlives the test frees nothing


W_NFFT, W_FIRST, W_SAMPLES = 16, 1, 10 * 16 + 5
W_FRAMES = er.frames_loop(W_SAMPLES, W_NFFT)                   # 19, and a tail of 13 samples
W_RAW = er.parity_capture()[:2 * (W_FIRST + W_SAMPLES)]


def w_threshold():
    thr = er.parity_threshold(W_NFFT)
    thr[3] = -1.0              # one bin goes whatever the frame holds
    return thr


def as_records(rec):
    out = np.zeros(rec.size, gpsjam.EXCISE_DTYPE)
    for key in ("total", "removed", "n_excised"):
        out[key] = rec[key]
    return out


def test_device_excise_on_the_host_double(host_dev):
    lib, thr = host_dev._lib, w_threshold()
    want = er.excise(W_RAW, thr, W_NFFT, W_FIRST)
    assert want.records.size == W_FRAMES == 19 == gpsjam.excise_frames(W_SAMPLES, W_NFFT) and np.all(want.records["n_excised"] >= 1)
    for n, (source, held) in enumerate(host_lib.sources(host_dev, W_RAW), 1):
        lib.calls.clear()
        uploads = gpsjam.Capture.uploads
        cleaned, rec = host_dev.excise(source, thr, nfft=W_NFFT, first_sample=W_FIRST)
        assert gpsjam.Capture.uploads == uploads + (source is W_RAW), "host bytes are uploaded once; the cleaned capture is no upload"
        assert isinstance(cleaned, gpsjam.Capture) and cleaned.nbytes == 2 * W_SAMPLES and rec.dtype == gpsjam.EXCISE_DTYPE
        assert np.array_equal(HostLib.view(cleaned.ptr, cleaned.nbytes), want.out) and rec.tobytes() == as_records(want.records).tobytes()
        assert host_lib.mallocs(lib) == [4 * W_NFFT, 2 * W_SAMPLES, 16 * W_FRAMES], "the thresholds, the output, the records"
        assert lib.calls[-1] == ("excise", W_FIRST, W_SAMPLES, W_NFFT) and host_dev.kernel_calls == {"excise": n}
        assert set(lib.mem) == held | {cleaned.ptr}, "every buffer but the result is freed"
        cleaned.free()
    # thresholds that are on the device already are taken as they are; a given range
    d_thr = gpsjam.DevBuf(host_dev, 4 * W_NFFT).upload(thr)
    lib.calls.clear()
    part, rec = host_dev.excise(W_RAW, d_thr, nfft=W_NFFT, n_samples=64)
    assert lib.calls == [("malloc", 128), ("malloc", 16 * 7), ("excise", 0, 64, W_NFFT)] and part.nbytes == 128 and rec.size == 7
    assert np.array_equal(HostLib.view(part.ptr, 128), er.excise(W_RAW, thr, W_NFFT, 0, 64).out)
    assert set(lib.mem) == {d_thr.ptr, part.ptr} and host_dev.kernel_calls == {"excise": 3}
    part.free()
    d_thr.free()
    assert not lib.mem


def test_device_excise_refusals(host_dev):
    lib, thr = host_dev._lib, w_threshold()
    host_lib.check_freed(host_dev, W_RAW, lambda cap: host_dev.excise(cap, thr, nfft=W_NFFT))
    for bad in (thr[:-1], np.append(thr, 0.0)):
        host_lib.check_refused(host_dev, W_RAW, lambda s: host_dev.excise(s, bad, nfft=W_NFFT), ValueError,
                               f"threshold holds {bad.size} values, nfft is 16")
    assert not host_lib.mallocs(lib) and host_dev.kernel_calls == {}
    # a range shorter than a frame is the library's to refuse: the output and the records are allocated, never empty, and freed
    lib.refuse("gj_excise_dev")
    host_lib.check_refused(host_dev, W_RAW, lambda s: host_dev.excise(s, thr, nfft=W_NFFT, first_sample=W_FIRST + W_SAMPLES),
                           gpsjam.GpsJamError, host_lib.REFUSED_TEXT, counted="excise")
    assert host_lib.mallocs(lib) == [4 * W_NFFT, 1, 16] * 2 and host_dev.kernel_calls == {"excise": 2}


def test_clean_with_a_given_threshold_on_the_host_double(host_dev):
    lib, thr = host_dev._lib, w_threshold()
    want = er.excise(W_RAW, thr, W_NFFT)
    for source, held in host_lib.sources(host_dev, W_RAW):
        res = mitigate.clean(host_dev, source, nfft=W_NFFT, threshold=thr.astype(np.float64))
        assert isinstance(res, mitigate.Cleaned) and res.floor_from == "given" and res.threshold.dtype == np.float32
        assert np.array_equal(res.threshold, thr) and res.records.tobytes() == as_records(want.records).tobytes()
        assert np.array_equal(HostLib.view(res.capture.ptr, res.capture.nbytes), want.out)
        total = float(res.records["total"].astype(np.float64).sum())
        assert res.removed_share == float(res.records["removed"].astype(np.float64).sum()) / total and 0.0 < res.removed_share < 1.0
        assert set(lib.mem) == held | {res.capture.ptr}
        res.capture.free()
    assert host_dev.kernel_calls == {"excise": 2}
    host_lib.check_refused(host_dev, W_RAW[:2 * (W_NFFT - 1)], lambda s: mitigate.clean(host_dev, s, nfft=W_NFFT, threshold=thr),
                           ValueError, "the capture holds 15 samples, fewer than one frame of 16")
