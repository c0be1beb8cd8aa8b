"""The short-time spectral ridge (gj_ridge_dev, include/gpsjam.h) restated in float64 numpy, and the inputs of the ridge
tests.  Not a test module: tests/test_ridge_host.py and tests/test_ridge_gpu.py import it.

    x[t]   = ((I_t - offset) + j (Q_t - offset)) * scale
    w[n]   = 0.5 - 0.5 cos(2 pi n / N)
    X_f    = np.fft.fft(w * x[s_f : s_f + N]),   s_f = first_sample + f * hop
    P_f[k] = |X_f[k]|^2

Every input is made here in numpy from a seed and quantised to uint8 the way the reference's mixer does
(simulate/frontend/add_jammer_and_mix.py:170-177: float32, AWGN of sigma 6.25 LSB by default, clip to [-128, 127],
truncate to int16, + 128).
"""
import functools

import numpy as np

RECORD64 = np.dtype([("total", np.float64), ("peak", np.float64), ("second", np.float64), ("peak_bin", np.int32)])

FS = 2.048e6
NOISE_SIGMA = 6.25          # add_jammer_and_mix.py:202
TONE_HZ = 200e3
CHIRP_BW_HZ, CHIRP_PERIOD_S = 1e6, 20e-3
CHIRP_RATE = CHIRP_BW_HZ / CHIRP_PERIOD_S          # 5e7 Hz/s
PRF_HZ, DUTY = 1000.0, 0.5
BROADBAND_SIGMA = 30.0
CASES = ("none", "cw", "chirp", "pulsed", "broadband")
CLASSIFIER_SAMPLES = 1 << 18
# seeds chosen so that no frame of any capture has a near-tied peak (tests/test_ridge_host.py asserts it)
CLASSIFIER_SEED = {"none": 107, "cw": 204, "chirp": 302, "pulsed": 419, "broadband": 125}
PARITY_SAMPLES = 1 << 17
PARITY_SEED = 3
# a multiple of fs/16 plus a fifth of a 4096-point bin: near a bin centre at every size (a tone half way between two
# bins would make near ties of its two bins the rule), on none of them exactly
PARITY_TONE_HZ = -384e3 + 100.0


def hann(n):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / n)


def unpack(raw, offset=127.5, scale=1.0 / 127.5):
    u = np.asarray(raw, np.uint8).astype(np.float64)
    n = u.size // 2
    return ((u[0:2 * n:2] - offset) + 1j * (u[1:2 * n:2] - offset)) * scale


def frames_that_fit(nbytes, first_sample, nfft, hop):
    """gj_ridge_frames as the loop it abbreviates."""
    if nfft < 1 or hop < 1:
        return 0
    n, s, total = 0, first_sample, nbytes // 2
    while s + nfft <= total:
        n += 1
        s += hop
    return n


def ridge(raw, nfft, hop, first_sample=0, n_frames=None, guard=2, offset=127.5, scale=1.0 / 127.5):
    """(records[n_frames] of RECORD64, margin[n_frames]); margin = 1 - (largest P at any other bin) / peak
    (1 for a frame without power)."""
    return ridge_of(unpack(raw, offset, scale), nfft, hop, first_sample, n_frames, guard)


def ridge_of(x, nfft, hop, first_sample=0, n_frames=None, guard=2):
    """The same on complex samples that are already unpacked."""
    x = np.asarray(x, np.complex128)
    if n_frames is None:
        n_frames = (x.size - first_sample - nfft) // hop + 1 if x.size - first_sample >= nfft else 0
    starts = first_sample + hop * np.arange(n_frames, dtype=np.int64)
    assert n_frames > 0 and starts[-1] + nfft <= x.size
    rec = np.zeros(n_frames, RECORD64)
    margin = np.ones(n_frames)
    w = hann(nfft)
    k = np.arange(nfft)
    for lo in range(0, n_frames, 4096):                   # blocks of frames: bounded memory at 16 points
        st = starts[lo:lo + 4096]
        p = np.abs(np.fft.fft(x[st[:, None] + k[None, :]] * w[None, :], axis=1)) ** 2
        pb = np.argmax(p, axis=1)                          # first maximum = smallest k
        rows = np.arange(st.size)
        peak = p[rows, pb]
        d = np.abs(k[None, :] - pb[:, None])
        d = np.minimum(d, nfft - d)
        second = np.where(d > guard, p, 0.0).max(axis=1)
        others = np.where(d > 0, p, -1.0).max(axis=1)
        r = rec[lo:lo + 4096]
        r["total"], r["peak"], r["second"], r["peak_bin"] = p.sum(axis=1), peak, second, pb
        margin[lo:lo + 4096] = np.where(peak > 0, 1.0 - others / np.where(peak > 0, peak, 1.0), 1.0)
    return rec, margin


# ---------------------------------------------------------------------------------------------------- inputs
def quantise(z):
    """Complex LSB-valued samples -> interleaved uint8, as add_jammer_and_mix.py:175-177."""
    f = np.empty(2 * z.size, np.float32)
    f[0::2], f[1::2] = z.real, z.imag
    f = np.clip(f, -128.0, 127.0)
    return (f.astype(np.int16) + 128).astype(np.uint8)


def _noise(rng, n, sigma):
    return rng.normal(0.0, sigma, n).astype(np.float32) + 1j * rng.normal(0.0, sigma, n).astype(np.float32)


def tone(n, freq_hz, amp, fs=FS):
    return amp * np.exp(2j * np.pi * freq_hz * np.arange(n) / fs)


def chirp(n, amp, fs=FS):
    """Saw-tooth VCO as chirpJammer.py's, -BW/2 .. +BW/2 once per period."""
    t = np.arange(n) / fs
    f = -0.5 * CHIRP_BW_HZ + CHIRP_BW_HZ * ((t / CHIRP_PERIOD_S) % 1.0)
    return amp * np.exp(2j * np.pi * np.cumsum(f) / fs)


def pulsed(n, amp, fs=FS):
    """A carrier at 0 Hz gated by a square wave, as pulsedJammer.py's."""
    t = np.arange(n) / fs
    return amp * (((t * PRF_HZ) % 1.0) < DUTY).astype(np.float64) * np.exp(0.25j * np.pi)


@functools.lru_cache(maxsize=None)
def classifier_capture(case):
    """2^18 samples: the first half noise, the second half noise plus the case's interferer.  Read-only uint8."""
    assert case in CASES
    rng = np.random.default_rng(CLASSIFIER_SEED[case])
    n, h = CLASSIFIER_SAMPLES, CLASSIFIER_SAMPLES // 2
    z = _noise(rng, n, NOISE_SIGMA).astype(np.complex128)
    if case == "cw":
        z[h:] += tone(h, TONE_HZ, 40.0)
    elif case == "chirp":
        z[h:] += chirp(h, 40.0)
    elif case == "pulsed":
        z[h:] += pulsed(h, 40.0)
    elif case == "broadband":
        z[h:] += _noise(rng, h, BROADBAND_SIGMA)
    raw = quantise(z)
    raw.setflags(write=False)
    return raw


@functools.lru_cache(maxsize=None)
def parity_capture():
    """2^17 samples of noise plus a tone plus a short strong burst.  Read-only uint8."""
    rng = np.random.default_rng(PARITY_SEED)
    n = PARITY_SAMPLES
    z = _noise(rng, n, NOISE_SIGMA).astype(np.complex128) + tone(n, PARITY_TONE_HZ, 25.0)
    z[70000:70900] += _noise(rng, 900, 40.0)
    raw = quantise(z)
    raw.setflags(write=False)
    return raw


# classifier tolerances (the issue's table): one bin, one lag of the 16-frame period, 0.05 of duty, 0.5 dB
FREQ_TOL_HZ = FS / 256
PRF_REL_TOL = 1.0 / 16.0
DUTY_TOL = 0.05
JNR_TOL_DB = 0.5
BROADBAND_JNR_DB = 10.0 * np.log10((BROADBAND_SIGMA ** 2 + NOISE_SIGMA ** 2) / NOISE_SIGMA ** 2)
# The sweep-rate estimator's own error on the float64 records of classifier_capture("chirp"), measured on the CPU:
# 49 998 878 Hz/s against 5e7, a relative error of 2.25e-5 (a least-squares line through some 320 frames per sweep
# averages the bin quantisation away).  The tolerance is twice that; 5 % would be the most an estimator may need.
CHIRP_REL_ERR_MEASURED = 2.25e-5
CHIRP_REL_TOL = 2.0 * CHIRP_REL_ERR_MEASURED
NEAR_TIE = 1e-4             # no frame of any GPU input may have a smaller margin
ONSET_ARGS = dict(noise_samples=65536, window=1000, factor=4.0)   # K4 for the end-to-end test: the interferers are 13-14 dB up


def check_interference(case, res):
    """The expected kind and parameters of one classifier case, with the tolerances above."""
    assert res.kind == case, (case, res)
    if case == "none":
        assert res.jnr_db is None and res.freq_hz is None and res.sweep_hz_per_s is None and res.prf_hz is None and res.duty is None
        return
    assert res.jnr_db is not None and np.isfinite(res.jnr_db)
    if case == "cw":
        assert abs(res.freq_hz - TONE_HZ) <= FREQ_TOL_HZ, res
        assert res.sweep_hz_per_s is None and res.prf_hz is None and res.duty is None
    elif case == "chirp":
        print(f"chirp: {res.sweep_hz_per_s:.1f} Hz/s, relative error {abs(res.sweep_hz_per_s / CHIRP_RATE - 1.0):.3e} (tolerance {CHIRP_REL_TOL:.3e})")
        assert CHIRP_REL_TOL <= 0.05
        assert abs(res.sweep_hz_per_s / CHIRP_RATE - 1.0) <= CHIRP_REL_TOL, res     # measured 2.25e-5 on the CPU
        assert res.freq_hz is None and res.prf_hz is None and res.duty is None
    elif case == "pulsed":
        assert abs(res.prf_hz / PRF_HZ - 1.0) <= PRF_REL_TOL, res
        assert abs(res.duty - DUTY) <= DUTY_TOL, res
        assert res.sweep_hz_per_s is None
    elif case == "broadband":
        print(f"broadband: jnr {res.jnr_db:.3f} dB against {BROADBAND_JNR_DB:.3f}")
        assert abs(res.jnr_db - BROADBAND_JNR_DB) <= JNR_TOL_DB, res
        assert res.freq_hz is None and res.sweep_hz_per_s is None and res.prf_hz is None and res.duty is None


PARITY_NFFT = (16, 32, 64, 128, 256, 512, 1024, 2048, 4096)


def parity_hops(nfft):
    return (nfft // 2, nfft // 2 + 37)


@functools.lru_cache(maxsize=None)
def parity_reference(nfft, hop, first_sample, guard, offset=127.5, scale=1.0 / 127.5):
    """The restatement of parity_capture() at one geometry, computed once and shared."""
    rec, margin = ridge(parity_capture(), nfft, hop, first_sample, None, guard, offset, scale)
    rec.setflags(write=False)
    margin.setflags(write=False)
    return rec, margin


RTOL = 1e-5                 # the project's figure for a K2 PSD value summed in another order (tests/test_gpu_parity.py)


def compare(got, want, what):
    assert got.size == want.size, what
    np.testing.assert_array_equal(got["peak_bin"], want["peak_bin"], err_msg=str(what))
    for key in ("total", "peak"):
        err = np.max(np.abs(got[key] - want[key]) / want[key])
        assert err <= RTOL, (what, key, err)
    err = np.max(np.abs(got["second"] - want["second"]) / want["peak"])
    assert err <= RTOL, (what, "second", err)
