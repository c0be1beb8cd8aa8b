"""Inputs at the edge of the uint8 range -- what a receiver next to a strong jammer records (a saturated ADC: runs of
0 and 255), constant bytes, the Nyquist pattern at full scale, uniform bytes over the whole range, one impulse -- through
K1-K5 against the oracle.  Tolerances as everywhere (module docstring of test_gpu_parity.py)."""
import numpy as np
import pytest

from oracle import gpsjam_oracle as orc

pytestmark = pytest.mark.gpu

N = 300000   # samples


def rel_err(got, want, floor=1e-12):
    keep = want > floor
    return float(np.max(np.abs(got[keep] - want[keep]) / want[keep])) if keep.any() else 0.0


def _interleave(i, q):
    raw = np.empty(2 * i.size, np.uint8)
    raw[0::2], raw[1::2] = i, q
    return raw


def extreme_captures():
    rng = np.random.RandomState(11)
    t = np.arange(N)
    out = {}
    out["constant 255"] = np.full(2 * N, 255, np.uint8)
    out["constant 0"] = np.zeros(2 * N, np.uint8)
    out["constant 128/127"] = _interleave(np.full(N, 128, np.uint8), np.full(N, 127, np.uint8))
    out["nyquist full scale"] = _interleave(np.where(t & 1, 255, 0).astype(np.uint8), np.where(t & 1, 0, 255).astype(np.uint8))
    out["uniform bytes"] = rng.randint(0, 256, 2 * N).astype(np.uint8)
    sat = 400.0 * np.exp(2j * np.pi * 0.031 * t) + rng.normal(0, 30, N) + 1j * rng.normal(0, 30, N)   # clips hard
    out["saturated tone"] = _interleave((np.clip(np.rint(sat.real), -128, 127) + 128).astype(np.uint8),
                                        (np.clip(np.rint(sat.imag), -128, 127) + 128).astype(np.uint8))
    quiet = (np.clip(np.rint(rng.normal(0, 2.0, 2 * N)), -128, 127) + 128).astype(np.uint8)
    burst = quiet.copy()
    burst[2 * 220000:] = np.where(rng.randint(0, 2, 2 * (N - 220000)) == 1, 255, 0)        # rail to rail after 220000
    out["quiet then rail to rail"] = burst
    imp = np.full(2 * N, 128, np.uint8)
    imp[2 * 123457] = 255
    out["one impulse"] = imp
    return out


CAPTURES = extreme_captures()


@pytest.mark.parametrize("name", list(CAPTURES))
def test_extreme_k1_power_map(dev, name):
    raw = CAPTURES[name]
    for chunk_bytes in (65536, 131072):
        pm = dev.chunk_power(raw, chunk_bytes=chunk_bytes)
        np.testing.assert_allclose(pm, orc.chunk_power(raw, chunk_bytes), rtol=1e-6)


@pytest.mark.parametrize("name", list(CAPTURES))
@pytest.mark.parametrize("nperseg", [256, 4096])
def test_extreme_k2_welch(dev, name, nperseg):
    raw = CAPTURES[name]
    psd, _ = dev.welch(raw, chunk_samples=100000, nperseg=nperseg, want_db=False)
    lin, _, _ = orc.widmo_waterfall(raw, nperseg=nperseg, chunk_samples=100000)
    assert psd.shape == lin.shape and np.all(np.isfinite(psd)) and np.all(psd >= 0)
    # relative to each row's own peak for the bins the reference leaves at rounding-noise level (a constant capture is
    # all such bins: scipy's detrend leaves ~1e-17, the frequency-domain detrend ~1e-13 of a full-scale bin)
    scale = lin.max(axis=1, keepdims=True)
    big = lin > 1e-6 * np.maximum(scale, 1e-30)
    if big.any():
        assert float(np.max(np.abs(psd[big] - lin[big]) / lin[big])) < 1e-4, name
    full_scale = 1.0 / (2.048e6 * 0.375 * nperseg) * nperseg ** 2 * 2.0           # PSD of a full-scale tone, one bin
    # every bin, the rounding-noise ones included: off by less than 2e-5 of the row's peak (1e-12 of full scale for a
    # capture whose true spectrum is empty)
    assert float(np.max(np.abs(psd - lin))) < 2e-5 * max(float(scale.max()), 5e-8 * full_scale), name


@pytest.mark.parametrize("name", list(CAPTURES))
def test_extreme_k3_amp_stats(dev, name):
    raw = CAPTURES[name]
    for thr in (0.0, 0.5, 1.2, 1.5):
        st = dev.amp_stats(raw, thr)
        k, avg = orc.rssi_amp_stats(raw, thr)
        if k is None:
            assert st.first_index == -1 and st.count == 0, (name, thr)
        else:
            assert st.first_index == k and st.count == N - k, (name, thr)
            np.testing.assert_allclose(st.mean, avg, rtol=1e-6)


@pytest.mark.parametrize("name", list(CAPTURES))
def test_extreme_k4_onset(dev, name):
    raw = CAPTURES[name]
    z = orc.tdoa_unpack(raw)
    for noise, window, factor in ((200000, 1000, 50.0), (1000, 64, 3.0)):
        got = dev.onset(raw, noise, window, factor)
        assert got.start_index == orc.tdoa_onset(z, noise, window, factor), (name, noise, window, got.margin)


@pytest.mark.parametrize("name", list(CAPTURES))
def test_extreme_k5_lags(dev, name):
    raw = CAPTURES[name]
    n = 50000
    a = raw[2 * 200000:2 * (200000 + n)]
    b = raw[2 * (200000 - 17):2 * (200000 - 17 + n)]          # the same signal 17 samples later
    lags, peaks, margins = dev.xcorr_lags([a, b], [(0, 1), (1, 0)], want_margins=True)
    want01, pk01 = orc.xcorr_lag(orc.tdoa_unpack(b), orc.tdoa_unpack(a))
    want10, _ = orc.xcorr_lag(orc.tdoa_unpack(a), orc.tdoa_unpack(b))
    # constant / periodic captures: the correlation is a triangle, the runner-up sits (N-1)/N below the peak
    assert lags[0] == want01 and lags[1] == want10, (name, lags, margins)
    if margins[0] > 1e-3:
        assert want01 == 17 and want10 == -17
        np.testing.assert_allclose(peaks[0], pk01, rtol=1e-4)
    else:
        np.testing.assert_allclose(margins, 1.0 / n, rtol=0.02)


@pytest.mark.parametrize("name", list(CAPTURES))
def test_extreme_fused_scan(dev, name):
    """The one-pass scan of the pipeline (gj_stream_scan_dev) on the same captures: power map, amplitude statistics and
    onset as from K1 / K3 / K4 alone and as the oracle has them."""
    raw = CAPTURES[name]
    nbytes, chunk = raw.size, 65536
    buf = dev.alloc(nbytes).upload(raw)
    nch = dev.chunk_count(nbytes, chunk)
    z = orc.tdoa_unpack(raw)
    for thr, (noise, window, factor) in ((0.0, (200000, 1000, 50.0)), (1.2, (1000, 64, 3.0))):
        d_pow, d_amp, d_on = dev.alloc(4 * nch), dev.alloc(32), dev.alloc(32)
        dev.stream_scan_dev(buf, nbytes, chunk, d_pow, thr, d_amp, noise, window, factor, d_on)
        dev.synchronize()
        amp = np.frombuffer(d_amp.download(np.uint8).tobytes(), dtype=[("i", "<i8"), ("c", "<u8"), ("s", "<f8"),
                                                                       ("m", "<f4"), ("r", "<f4")])[0]
        np.testing.assert_allclose(d_pow.download(np.float32, nch), orc.chunk_power(raw, chunk), rtol=1e-6)
        k, avg = orc.rssi_amp_stats(raw, thr)
        if k is None:
            assert amp["i"] == -1 and amp["c"] == 0, (name, thr)
        else:
            assert amp["i"] == k and amp["c"] == N - k, (name, thr)
            np.testing.assert_allclose(amp["m"], avg, rtol=1e-6)
        assert int(d_on.download(np.int64, 1)[0]) == orc.tdoa_onset(z, noise, window, factor), (name, noise, window)
        for b in (d_pow, d_amp, d_on):
            b.free()
    buf.free()


# ---------------------------------------------------------------------------------------------------------------------
# The same captures at the ENDS of the unpack range.  gj_set_unpack takes any offset that is a multiple of 0.5 in
# [0, 255]; e = (2I - o2)^2 + (2Q - o2)^2 reaches 2 * 510^2 = 520 200 at offsets 0 and 255 against 130 050 at 127.5, so
# every integer accumulator of K1, K3, K4, the fused scan and the blanker is at its largest here.  Yardstick: exact
# integer arithmetic in numpy int64 (tests/exact_restatement.py with o2, tests/blank_restatement.py with offset).
# ---------------------------------------------------------------------------------------------------------------------
import contextlib

import blank_restatement as br
import exact_restatement as ex
from gpu_lib import run_blank

END_OFFSETS = (0.0, 0.5, 254.5, 255.0)
E_MAX = 2 * 510 ** 2                       # 520 200
HEAD = 1 << 16                             # samples kept from the front of a capture
RAIL_AT, IMPULSE_AT = 220000, 123457       # extreme_captures()


@contextlib.contextmanager
def unpack_offset(dev, offset):
    """offset with scale 1/127.5 for the body, the default convention afterwards; yields o2 = 2 * offset."""
    try:
        dev.set_unpack(offset, 1.0 / 127.5)
        yield int(round(2 * offset))
    finally:
        dev.set_unpack()
    assert dev.get_unpack() == (127.5, 1.0 / 127.5)


def cut(name):
    """The first 2^16 samples and, where the capture has one, a window around its feature: 100 003 samples (ragged) of
    the stationary captures, 2^16 + 49 152 with the rail-to-rail part from 81 920 on, 2^16 + 8193 with the impulse at
    the odd sample 69 633."""
    raw = CAPTURES[name]
    if name == "quiet then rail to rail":
        return np.concatenate([raw[:2 * HEAD], raw[2 * (RAIL_AT - 16384):2 * (RAIL_AT + 32768)]])
    if name == "one impulse":
        return np.concatenate([raw[:2 * HEAD], raw[2 * (IMPULSE_AT - 4097):2 * (IMPULSE_AT + 4096)]])
    return raw[:2 * 100003]


def quiet_then(byte):
    """2^15 quiet samples, then a constant byte: 255 is the loudest there is under offsets 0 and 0.5 and silence under
    255; 0 the other way round."""
    quiet = CAPTURES["quiet then rail to rail"][:2 * (1 << 15)]
    return np.concatenate([quiet, np.full(2 * 40000, byte, np.uint8)])


@pytest.mark.parametrize("offset", END_OFFSETS)
@pytest.mark.parametrize("name", list(CAPTURES))
def test_end_offsets_k1_power_map(dev, name, offset):
    raw = cut(name)
    with unpack_offset(dev, offset) as o2:
        for chunk_bytes in (65536, 131072, 1000):          # one tile per chunk, the atomics path, ragged chunks
            pm = dev.chunk_power(raw, chunk_bytes=chunk_bytes, eps=0.0)
            np.testing.assert_array_equal(pm, ex.chunk_power(raw, chunk_bytes, eps=0.0, o2=o2), err_msg=f"{name} {offset} {chunk_bytes}")


@pytest.mark.parametrize("offset", END_OFFSETS)
@pytest.mark.parametrize("name", list(CAPTURES))
def test_end_offsets_k3_amp_stats(dev, name, offset):
    raw = cut(name)
    n = raw.size // 2
    with unpack_offset(dev, offset) as o2:
        v = 2.0 * raw.astype(np.float64) - o2
        amp = np.sqrt(v[0::2] ** 2 + v[1::2] ** 2) * (0.5 / 127.5)           # plain float64
        for thr in (0.0, 1.5):
            st = dev.amp_stats(raw, thr)
            hits = np.flatnonzero(amp > thr)
            # an integer m = 255^2 thr^2 would be a tie; 146 306.25 is none, and sqrt(m) / 255 clears 1.5 by 4e-6 at
            # the nearest integers, 30 float32 ulps: the float32 restatement must agree with float64 before the GPU is asked
            assert ex.amp_stats(raw, thr, o2)["first"] == (int(hits[0]) if hits.size else -1)
            if hits.size == 0:
                assert st.first_index == -1 and st.count == 0, (name, offset, thr)
            else:
                k = int(hits[0])
                assert st.first_index == k and st.count == n - k, (name, offset, thr, st.first_index, k)
                np.testing.assert_allclose(st.mean, amp[k:].mean(), rtol=1e-6)


K4_NOISE = 20000
K4_FACTORS = (1.5, 3.9)    # 3.9: under offset 0 only a window almost full of 255s crosses (130 050 / 32 768 = 3.97)


def _k4_captures():
    return {"quiet then rail to rail": cut("quiet then rail to rail"), "quiet then 255": quiet_then(255), "quiet then 0": quiet_then(0)}


@pytest.mark.parametrize("offset", END_OFFSETS)
@pytest.mark.parametrize("window", [64, 1000, 8192])
@pytest.mark.parametrize("name", ["quiet then rail to rail", "quiet then 255", "quiet then 0"])
def test_end_offsets_k4_onset_and_fused_scan(dev, name, window, offset):
    raw = _k4_captures()[name]
    nbytes, chunk = raw.size, 65536
    nch = dev.chunk_count(nbytes, chunk)
    buf = dev.alloc(nbytes).upload(raw)
    d_pow, d_amp, d_on = dev.alloc(4 * nch), dev.alloc(32), dev.alloc(32)
    try:
        with unpack_offset(dev, offset) as o2:
            if window == 8192 and (offset, name) in ((0.0, "quiet then 255"), (255.0, "quiet then 0")):
                # the screening bound of a 512-sample block spans 17 blocks: past 2^32 here, while the exact window sum
                # still fits -- the case a 32-bit bound gets wrong
                assert 17 * 512 * int(ex.msq(raw, o2).max()) > 2 ** 32 > 8192 * int(ex.msq(raw, o2).max())
            for factor in K4_FACTORS:
                want = ex.onset(raw, K4_NOISE, window, factor, o2)
                got = dev.onset(raw, K4_NOISE, window, factor)
                what = (name, window, offset, factor)
                print(f"{what}: start {got.start_index} (exact {want['start']}), noise {got.noise_power!r}, threshold {got.threshold!r}")
                assert got.start_index == want["start"], (what, got.start_index, want["start"])
                assert np.float32(got.noise_power) == want["noise"] and np.float32(got.threshold) == want["thr"], what
                dev.stream_scan_dev(buf, nbytes, chunk, d_pow, 0.0, d_amp, K4_NOISE, window, factor, d_on, eps=0.0)
                dev.synchronize()
                on = np.frombuffer(d_on.download(np.uint8).tobytes(), dtype=[("start", "<i8"), ("noise", "<f4"), ("thr", "<f4"),
                                                                             ("hit", "<f4"), ("before", "<f4"), ("guard", "<i8")])[0]
                assert on["start"] == want["start"], (what, "fused", int(on["start"]), want["start"])
                assert on["noise"] == want["noise"] and on["thr"] == want["thr"], (what, "fused")
                np.testing.assert_array_equal(d_pow.download(np.float32, nch), ex.chunk_power(raw, chunk, eps=0.0, o2=o2))
    finally:
        for b in (buf, d_pow, d_amp, d_on):
            b.free()


def test_end_offsets_k4_cases_cross_where_they_are_meant_to():
    """No kernel runs here: what the K4 cases above exercise.  Under offsets 0 and 0.5 both captures cross at factor 1.5, and at
    3.9 'quiet then 255' crosses with a window that is almost full -- the crossing lies in a block whose 17-block bound
    is past 2^32 at window 8192 and offset 0."""
    caps = _k4_captures()
    for offset in (0.0, 0.5):
        o2 = int(2 * offset)
        for window in (64, 1000, 8192):
            assert ex.onset(caps["quiet then rail to rail"], K4_NOISE, window, 1.5, o2)["start"] > 0
            assert ex.onset(caps["quiet then 255"], K4_NOISE, window, 1.5, o2)["start"] > 0
            assert ex.onset(caps["quiet then 255"], K4_NOISE, window, 3.9, o2)["start"] > 0
    window = 8192
    for name, o2 in (("quiet then 255", 0), ("quiet then 0", 510)):
        raw = caps[name]
        m = ex.msq(raw, o2)
        i0 = ex.onset(raw, K4_NOISE, window, 3.9, o2)["start"] - window // 2
        blk = i0 // 512
        assert i0 > 0 and int(m[512 * blk:512 * (blk + 17)].sum()) > 2 ** 32 > int(m[i0:i0 + window].sum())


BLANK_CAPTURES = ("constant 255", "constant 0", "uniform bytes", "quiet then rail to rail")
BLANK_RANGES = ((br.PARITY_FIRST, br.PARITY_SAMPLES), (0, 8192))       # the parity range; exactly one tile
BLANK_PASS = 12288                                                      # samples of P one pass of the kernel holds


def _blank_capture(name):
    """2^14 samples: the head of the capture; of 'quiet then rail to rail' the 2^14 around the step (at 8192)."""
    raw = CAPTURES[name]
    return raw[2 * (RAIL_AT - 8192):2 * (RAIL_AT + 8192)] if name == "quiet then rail to rail" else raw[:2 << 14]


@pytest.mark.parametrize("window,guard", [(1, 0), (16, 8), (1024, 1024)])
@pytest.mark.parametrize("name", BLANK_CAPTURES)
def test_end_offsets_blanker(dev, name, window, guard):
    raw = _blank_capture(name)
    constant = name.startswith("constant")
    with dev.capture(raw) as c:
        for offset in END_OFFSETS + (127.5,):
            with unpack_offset(dev, offset) as o2:
                for first, n in BLANK_RANGES:
                    e = ex.msq(raw[2 * first:2 * (first + n)], o2)
                    e_max = int(e.max())
                    loudest = (name, offset) in (("constant 255", 0.0), ("constant 0", 255.0))
                    if loudest:
                        assert e_max == E_MAX
                        if n >= BLANK_PASS:       # the regime where the kernel's 32-bit prefix sum P wraps
                            assert int(e[:BLANK_PASS].sum()) > 2 ** 32
                    at = np.float32(e_max / 4.0)
                    assert float(at) * 4.0 == e_max                       # exact in float32
                    thresholds = [0.0, float(at), np.inf] + ([float(np.nextafter(at, np.float32(0)))] if e_max else [])
                    for thr in thresholds:
                        want = br.blank(raw, thr, window, guard, first, n, offset)
                        got, rec = run_blank(dev, c, c.nbytes, first, n, window, guard, thr)
                        br.compare(got, rec, want, (name, window, guard, offset, first, n, thr))
                        if loudest:
                            assert int(want.records["total"].max()) == 4096 * E_MAX < 2 ** 32
                        if constant and e_max and thr == float(at):       # S = T in the interior, and the comparison is strict
                            assert not want.blanked[window:n - window].any()
                        if constant and e_max and 0.0 < thr < float(at):  # one ulp below: the whole interior
                            assert want.blanked[window:n - window].all()


@pytest.mark.parametrize("offset", [0.0, 255.0])
@pytest.mark.parametrize("nperseg", [256, 4096])
def test_end_offsets_k2_welch(dev, nperseg, offset):
    """One case to rule out a packed-int16 surprise: uniform bytes, against the oracle's Welch on (u - offset) * scale in
    float64.  1e-4 relative on the bins above 1e-6 of the row's peak, as everywhere."""
    raw = cut("uniform bytes")[:2 * 100000]
    with unpack_offset(dev, offset):
        psd, _ = dev.welch(raw, chunk_samples=100000, nperseg=nperseg, want_db=False)
    u = (raw.astype(np.float64) - offset) / 127.5
    z = u[0::2] + 1j * u[1::2]
    lin = np.fft.fftshift(orc.welch_twosided_c64(z - z.mean(), 2.048e6, nperseg))[None, :]
    assert psd.shape == lin.shape and np.all(np.isfinite(psd)) and np.all(psd >= 0)
    big = lin > 1e-6 * lin.max()
    err = float(np.max(np.abs(psd[big] - lin[big]) / lin[big]))
    print(f"welch {nperseg} at offset {offset}: {int(big.sum())} bins, largest relative error {err:.2e}")
    assert big.sum() >= nperseg - 1 and err < 1e-4


def test_end_offsets_k5_lag(dev):
    """A 17-sample shift of uniform bytes under offset 0, where every sample carries a DC of 127.5 (1 + j): the lag is
    the float64 restatement's, 17."""
    raw = CAPTURES["uniform bytes"]
    n = 50000
    a, b = raw[2 * 20000:2 * (20000 + n)], raw[2 * (20000 - 17):2 * (20000 - 17 + n)]
    with unpack_offset(dev, 0.0):
        lags, _ = dev.xcorr_lags([a, b], [(0, 1), (1, 0)])
    za, zb = (x[0::2].astype(np.float64) + 1j * x[1::2].astype(np.float64) for x in (a, b))
    assert ex.xcorr_f64(zb, za)[0] == 17 and ex.xcorr_f64(za, zb)[0] == -17
    assert lags.tolist() == [17, -17], lags
