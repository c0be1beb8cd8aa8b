"""Spectral kurtosis (gj_sk_dev, include/gpsjam.h) restated in float64 numpy, and the inputs and constants of the
spectral-kurtosis tests.  Not a test module: tests/test_skurt_host.py and tests/skurt/test_round6_gpu.py import it.

    x[t]     = (I_t - offset) + j (Q_t - offset)
    X_f      = fft(w * x[s_f : s_f + N]),  s_f = first_sample + f hop,  w the periodic Hann window
    P_f[k]   = |X_f[k]|^2 * scale^2
    S1[r][k] = sum_m P_{rM+m}[k]      S2[r][k] = sum_m P_{rM+m}[k]^2
    SK[r][k] = (M+1)/(M-1) * (M S2 / S1^2 - 1),  NaN where S1 == 0

Every input is built from the generators of tests/ridge_restatement.py (the reference simulator's interferers over
noise of sigma 6.25 LSB, quantised as its mixer does) plus a pulse train with a duty parameter.
"""
import functools

import numpy as np

import gpsjam
import ridge_restatement as rr

FS = rr.FS
NFFT = rr.PARITY_NFFT                       # 16 .. 4096
MAX_RUN = 16                                # frames per block of the kernel (stft_rows.h kRowMaxRun)

# ---------------------------------------------------------------------------------------------------- detection cases
DETECT_SAMPLES = 1 << 19
DETECT_NFFT = DETECT_HOP = DETECT_M = 256   # 8 rows
SIGMAS = 4.0
TONE_AMP = 2.0                              # +0.23 dB over noise of sigma 6.25 LSB
PULSE_AMP, PULSE_DUTY, PULSE_HZ = 6.0, 0.10, -300e3      # +0.21 dB
CHIRP_AMP = 3.0                             # +0.50 dB
TONE_BIN = 25                               # TONE_HZ / (FS / 256)
PULSE_BINS = (216, 221)                     # -300 kHz lies between bins 218 and 219
CASES = ("noise", "tone", "pulse", "chirp")
# seeds chosen so that no cell's SK of any case lies within EDGE of a band edge (tests/test_skurt_host.py asserts it)
DETECT_SEED = {"noise": 4, "tone": 10, "pulse": 4, "chirp": 7}
EDGE = 1e-3
EXCISE_AMPS = (2.0, 10.0, 40.0)             # a tone present from the first sample
EXCISE_SEED = 11


def pulse_train(n, amp, freq_hz, duty, prf_hz=rr.PRF_HZ, fs=FS):
    """A carrier at freq_hz gated by a rectangular wave of the given duty (pulsedJammer.py's with a duty parameter)."""
    t = np.arange(n) / fs
    return amp * (((t * prf_hz) % 1.0) < duty) * np.exp(2j * np.pi * freq_hz * t)


def _interferer(case, n):
    if case == "tone":
        return rr.tone(n, rr.TONE_HZ, TONE_AMP)
    if case == "pulse":
        return pulse_train(n, PULSE_AMP, PULSE_HZ, PULSE_DUTY)
    if case == "chirp":
        return rr.chirp(n, CHIRP_AMP)
    assert case == "noise"
    return 0.0


@functools.lru_cache(maxsize=None)
def detect_capture(case, with_interferer=True):
    """2^19 samples: noise of sigma 6.25 LSB plus the case's interferer, on from the first sample.  Read-only uint8.
    with_interferer=False: the same noise alone (the power an interferer is measured against)."""
    assert case in CASES
    rng = np.random.default_rng(DETECT_SEED[case])
    z = rr._noise(rng, DETECT_SAMPLES, rr.NOISE_SIGMA).astype(np.complex128)
    if with_interferer:
        z = z + _interferer(case, DETECT_SAMPLES)
    raw = rr.quantise(z)
    raw.setflags(write=False)
    return raw


@functools.lru_cache(maxsize=None)
def excise_capture(amp):
    """2^19 samples of noise with a tone of `amp` LSB at TONE_HZ from the first sample on.  Read-only uint8."""
    rng = np.random.default_rng(EXCISE_SEED)
    z = rr._noise(rng, DETECT_SAMPLES, rr.NOISE_SIGMA).astype(np.complex128) + rr.tone(DETECT_SAMPLES, rr.TONE_HZ, amp)
    raw = rr.quantise(z)
    raw.setflags(write=False)
    return raw


def power_db(raw, against):
    """10 log10 of the ratio of the two captures' mean |x|^2, from the bytes."""
    a, b = rr.unpack(raw, 127.5, 1.0), rr.unpack(against, 127.5, 1.0)
    return 10.0 * np.log10(np.mean(np.abs(a) ** 2) / np.mean(np.abs(b) ** 2))


# ---------------------------------------------------------------------------------------------------- the definition
def rows_that_fit(nbytes, first_sample, nfft, hop, frames_per_row):
    """gj_sk_rows as the loop it abbreviates: rows whose last frame still ends inside the capture."""
    if nfft < 1 or hop < 1 or frames_per_row < 1:
        return 0
    rows, total = 0, nbytes // 2
    while first_sample + ((rows + 1) * frames_per_row - 1) * hop + nfft <= total:
        rows += 1
    return rows


def frame_powers(raw, nfft, hop, first_sample, n_frames, offset=127.5, scale=1.0 / 127.5):
    """P[n_frames][nfft] in float64."""
    x = rr.unpack(raw, offset, 1.0)
    starts = first_sample + hop * np.arange(n_frames, dtype=np.int64)
    assert n_frames > 0 and starts[-1] + nfft <= x.size
    w = rr.hann(nfft)
    k = np.arange(nfft)
    p = np.empty((n_frames, nfft))
    for lo in range(0, n_frames, 8192):                    # blocks of frames: bounded memory at 16 points
        st = starts[lo:lo + 8192]
        p[lo:lo + 8192] = np.abs(np.fft.fft(x[st[:, None] + k[None, :]] * w[None, :], axis=1)) ** 2
    return p * (scale * scale)


def estimate(s1, s2, m):
    """The estimator in float64; NaN where S1 == 0."""
    s1, s2, m = np.asarray(s1, np.float64), np.asarray(s2, np.float64), float(m)
    with np.errstate(divide="ignore", invalid="ignore"):
        sk = (m + 1.0) / (m - 1.0) * (m * s2 / (s1 * s1) - 1.0)
    return np.where(s1 == 0, np.nan, sk)


def sums_of(p, frames_per_row, n_rows=None):
    """(S1, S2, SK)[n_rows][nfft] from frame powers."""
    if n_rows is None:
        n_rows = p.shape[0] // frames_per_row
    assert 1 <= n_rows and n_rows * frames_per_row <= p.shape[0]
    q = p[:n_rows * frames_per_row].reshape(n_rows, frames_per_row, p.shape[1])
    s1, s2 = q.sum(axis=1), (q * q).sum(axis=1)
    return s1, s2, estimate(s1, s2, frames_per_row)


def sk(raw, nfft, hop, frames_per_row, first_sample=0, n_rows=None, offset=127.5, scale=1.0 / 127.5):
    """The definition on the bytes `raw`: (S1, S2, SK), float64[n_rows][nfft]."""
    if n_rows is None:
        n_rows = rows_that_fit(np.asarray(raw).size, first_sample, nfft, hop, frames_per_row)
    return sums_of(frame_powers(raw, nfft, hop, first_sample, n_rows * frames_per_row, offset, scale), frames_per_row, n_rows)


def as_result(s1, s2, skv, nfft, hop, frames_per_row, first_sample=0):
    """The restatement's arrays as the object Device.spectral_kurtosis returns."""
    return gpsjam.SpectralKurtosis(s1, s2, skv, nfft, hop, frames_per_row, first_sample)


@functools.lru_cache(maxsize=None)
def detect_reference(case):
    """The restatement of detect_capture(case) at the detection geometry, as a SpectralKurtosis of float64 origin."""
    s1, s2, skv = sk(detect_capture(case), DETECT_NFFT, DETECT_HOP, DETECT_M)
    return as_result(s1, s2, skv, DETECT_NFFT, DETECT_HOP, DETECT_M), skv


def edge_distance(skv, frames_per_row, sigmas=SIGMAS):
    """Smallest distance of any finite cell to either band edge."""
    from gpsjam import kurtosis
    lo, hi = kurtosis.band(frames_per_row, sigmas)
    v = skv[np.isfinite(skv)]
    return float(min(np.min(np.abs(v - lo)), np.min(np.abs(v - hi))))


# ---------------------------------------------------------------------------------------------------- GPU parity
PARITY_M = (2, 5, 17)
BOUNDARY_NFFT = (64, 1024, 4096)
BOUNDARY_HOP = 293                           # 3 rows of 130 frames of 4096 points fit 2^17 samples
BOUNDARY_M = tuple(sorted({2, 3, 15, 16, 17, 31, 33, 63, 65, 130, MAX_RUN - 1, MAX_RUN + 1, 2 * MAX_RUN + 3}))
S1_TOL, S2_TOL = 1e-5, 2e-5                  # of the row's largest reference value


def parity_hops(nfft):
    return (nfft, nfft // 2 + 37)


@functools.lru_cache(maxsize=None)
def parity_powers(nfft, hop, first_sample, offset=127.5, scale=1.0 / 127.5):
    """Frame powers of rr.parity_capture() at one geometry, every frame that fits; computed once and shared."""
    raw = rr.parity_capture()
    p = frame_powers(raw, nfft, hop, first_sample, rr.frames_that_fit(raw.size, first_sample, nfft, hop), offset, scale)
    p.setflags(write=False)
    return p


worst = {"s1": 0.0, "s2": 0.0, "sk_ulp": 0.0}   # largest errors seen, relative to the tolerance's own reference


def check_sk(s1, s2, skv, m, what):
    """d_sk against the formula in float64 on the float32 sums the call wrote."""
    want = estimate(s1, s2, m)
    dead = s1 == 0
    assert np.array_equal(np.isnan(skv), dead), (what, "NaN exactly where S1 == 0")
    live = ~dead
    if live.any():
        w32 = want[live].astype(np.float32)
        ulps = np.abs(skv[live].astype(np.float64) - want[live]) / np.spacing(np.abs(w32)).astype(np.float64)
        worst["sk_ulp"] = max(worst["sk_ulp"], float(ulps.max()))
        assert ulps.max() <= 2.0, (what, float(ulps.max()))


def compare(got, p, m, n_rows, what):
    """GPU sums against the restatement's, from frame powers p."""
    r1, r2, _ = sums_of(p, m, n_rows)
    s1, s2, skv = got
    assert s1.shape == r1.shape, what
    e1 = float(np.max(np.abs(s1 - r1) / r1.max(axis=1, keepdims=True)))
    e2 = float(np.max(np.abs(s2 - r2) / r2.max(axis=1, keepdims=True)))
    worst["s1"], worst["s2"] = max(worst["s1"], e1), max(worst["s2"], e2)
    assert e1 <= S1_TOL, (what, "S1", e1)
    assert e2 <= S2_TOL, (what, "S2", e2)
    if skv is not None:
        check_sk(s1, s2, skv, m, what)
