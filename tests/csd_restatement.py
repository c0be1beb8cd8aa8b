"""Cross-spectral density and coherence of a capture pair (gj_csd_dev, include/gpsjam.h) restated in float64 numpy, and
the inputs and constants of its tests.  Not a test module: tests/test_csd_host.py and tests/csd/test_round6_gpu.py
import it.

    x_a[t]    = (I - offset) + j (Q - offset) of capture a at sample first_a + t          likewise x_b
    A_f       = fft(w * x_a[s_f : s_f + N]),  s_f = f hop,  w the periodic Hann window      B_f likewise
    Saa[r][k] = scale^2 sum_m |A_{rM+m}[k]|^2      Sbb likewise      Sab[r][k] = scale^2 sum_m B[k] conj(A[k])
    MSC[r][k] = |Sab|^2 / (Saa Sbb),  NaN where Saa Sbb == 0

Sign: b delayed by D samples gives arg Sab[k] = -2 pi k D / N.

Every input is built from the generators of tests/ridge_restatement.py (noise of sigma 6.25 LSB, quantised as the
reference's mixer does) plus band-limited Gaussian noise: white noise through a brick-wall filter, delayed by a phase
ramp on its whole-record FFT (a circular delay: the few samples that wrap are 1e-5 of the record).
"""
import functools

import numpy as np

import gpsjam
import ridge_restatement as rr
import skurt_restatement as sr

FS = rr.FS
NFFT = rr.PARITY_NFFT                       # 16 .. 4096
MAX_RUN = sr.MAX_RUN                        # frame pairs per block of the kernel (stft_rows.h kRowMaxRun)
S1_TOL = sr.S1_TOL                          # the project's tolerance for these very sums


# ---------------------------------------------------------------------------------------------------- inputs
def band_noise(rng, n, sigma, lo_hz, hi_hz, fs=FS):
    """(spectrum of) complex white Gaussian noise of `sigma` LSB per component, kept inside lo_hz .. hi_hz only."""
    z = rng.normal(0.0, sigma, n) + 1j * rng.normal(0.0, sigma, n)
    f = np.fft.fftfreq(n, 1.0 / fs)
    return np.fft.fft(z) * ((f >= lo_hz) & (f <= hi_hz))


def delayed(spectrum, delay, fs=FS):
    """The signal of `spectrum` delayed by `delay` samples (fractional, circular)."""
    f = np.fft.fftfreq(spectrum.size)
    return np.fft.ifft(spectrum * np.exp(-2j * np.pi * f * delay))


def _readonly(z):
    raw = rr.quantise(z)
    raw.setflags(write=False)
    return raw


# the parity pair: 2^17 samples; b holds a's wide-band source 2.5 samples later, each has its own noise, both the tone
PARITY_SAMPLES = rr.PARITY_SAMPLES
PARITY_SEED = 21
PARITY_SOURCE_SIGMA = 9.0
PARITY_DELAY = 2.5
PARITY_FIRST_A, PARITY_FIRST_B = 1, 4


@functools.lru_cache(maxsize=None)
def parity_pair():
    rng = np.random.default_rng(PARITY_SEED)
    n = PARITY_SAMPLES
    src = band_noise(rng, n, PARITY_SOURCE_SIGMA, -0.5 * FS, 0.5 * FS)
    tone = rr.tone(n, rr.PARITY_TONE_HZ, 25.0)
    a = delayed(src, 0.0) + rr._noise(rng, n, rr.NOISE_SIGMA) + tone
    b = delayed(src, PARITY_DELAY) + rr._noise(rng, n, rr.NOISE_SIGMA) + tone
    return _readonly(a), _readonly(b)


# the detection cases: 2^20 samples each
DETECT_SAMPLES = 1 << 20
DETECT_NFFT = DETECT_HOP = 256
CASES = ("noise", "subnoise", "two")
DETECT_M = {"noise": 1024, "subnoise": 4096, "two": 1024}
P_FA = 1e-6
EDGE = 1e-3                                 # no off-DC cell's MSC lies within this, relatively, of the threshold
SUB_BAND_HZ = (100e3, 400e3)
SUB_DB = -10.0                              # the jammer's density inside its band against the receiver noise's
SUB_DELAY = 0.4
SUB_BINS_INSIDE = (14, 48)                  # every one flagged: the 35 interior bins of 12.5 .. 50
SUB_BINS_OUTSIDE = (12, 50)                 # none flagged outside these
TWO_SIGMA = (20.0, 12.0)
TWO_DELAY = (3.25, -5.5)
TWO_BAND_HZ = ((100e3, 600e3), (-700e3, -200e3))
TWO_CORR_SAMPLES = 50000
# (source, noise of a, noise of b); chosen so that EDGE holds (tests/test_csd_host.py asserts it).  The noise pair also so
# that the ONE cell in a thousand which the threshold of p_fa 1e-3 lets through is there: of five pairs tried three had
# none, two had one, as a Poisson count of mean 1 does (the counts at 1e-2 and 1e-1, which the test holds as well, were
# 6..12 of 10 and 95..106 of 101 for all five)
DETECT_SEED = {"noise": (0, 1, 2), "subnoise": (7, 8, 9), "two": (46, 47, 48)}


@functools.lru_cache(maxsize=None)
def detect_pair(case, with_interferer=True):
    """(a, b), read-only uint8: independent noise of sigma 6.25 LSB in each plus the case's common source.
    with_interferer=False: the same noise alone (the power an interferer is measured against)."""
    assert case in CASES
    n = DETECT_SAMPLES
    s0, sa, sb = DETECT_SEED[case]
    za = rr._noise(np.random.default_rng(sa), n, rr.NOISE_SIGMA).astype(np.complex128)
    zb = rr._noise(np.random.default_rng(sb), n, rr.NOISE_SIGMA).astype(np.complex128)
    if with_interferer and case != "noise":
        rng = np.random.default_rng(s0)
        if case == "subnoise":
            src = band_noise(rng, n, rr.NOISE_SIGMA * 10.0 ** (SUB_DB / 20.0), *SUB_BAND_HZ)
            za, zb = za + delayed(src, 0.0), zb + delayed(src, SUB_DELAY)
        else:
            for sigma, delay, band in zip(TWO_SIGMA, TWO_DELAY, TWO_BAND_HZ):
                src = band_noise(rng, n, sigma, *band)
                za, zb = za + delayed(src, 0.0), zb + delayed(src, delay)
    return _readonly(za), _readonly(zb)


# ---------------------------------------------------------------------------------------------------- the definition
def rows_that_fit(nbytes_a, first_a, nbytes_b, first_b, nfft, hop, frames_per_row):
    """gj_csd_rows: rows whose last frame still ends inside BOTH captures, the fewer of what each holds on its own."""
    return min(sr.rows_that_fit(nbytes_a, first_a, nfft, hop, frames_per_row),
               sr.rows_that_fit(nbytes_b, first_b, nfft, hop, frames_per_row))


def frame_spectra(raw, nfft, hop, first, f0, n_frames, offset=127.5):
    """X[n_frames][nfft] in float64, LSB units, of frames f0 .. f0 + n_frames - 1."""
    x = rr.unpack(raw, offset, 1.0)
    starts = first + hop * np.arange(f0, f0 + n_frames, dtype=np.int64)
    assert n_frames > 0 and starts[-1] + nfft <= x.size
    return np.fft.fft(x[starts[:, None] + np.arange(nfft)[None, :]] * rr.hann(nfft)[None, :], axis=1)


def coherence(saa, sbb, sab):
    """|Sab|^2 / (Saa Sbb) in float64; NaN where Saa Sbb == 0."""
    saa, sbb, sab = np.asarray(saa, np.float64), np.asarray(sbb, np.float64), np.asarray(sab, np.complex128)
    den = saa * sbb
    with np.errstate(divide="ignore", invalid="ignore"):
        v = (sab.real * sab.real + sab.imag * sab.imag) / den
    return np.where(den == 0, np.nan, v)


def sums_of(a, b, frames_per_row, n_rows=None, scale=1.0 / 127.5):
    """(Saa, Sbb, Sab, MSC)[n_rows][nfft] from the frame spectra of both."""
    if n_rows is None:
        n_rows = a.shape[0] // frames_per_row
    assert 1 <= n_rows and n_rows * frames_per_row <= a.shape[0] and a.shape == b.shape
    shape = (n_rows, frames_per_row, a.shape[1])
    qa, qb = a[:n_rows * frames_per_row].reshape(shape), b[:n_rows * frames_per_row].reshape(shape)
    s2 = scale * scale
    saa, sbb, sab = (np.abs(qa) ** 2).sum(axis=1) * s2, (np.abs(qb) ** 2).sum(axis=1) * s2, (qb * np.conj(qa)).sum(axis=1) * s2
    return saa, sbb, sab, coherence(saa, sbb, sab)


def csd(raw_a, raw_b, nfft, hop, frames_per_row, first_a=0, first_b=0, n_rows=None, offset=127.5, scale=1.0 / 127.5):
    """The definition on the bytes of the pair: (Saa, Sbb, Sab, MSC), float64 / complex128 [n_rows][nfft].  Evaluated in
    pieces of whole rows: bounded memory at 16 points."""
    if n_rows is None:
        n_rows = rows_that_fit(np.asarray(raw_a).size, first_a, np.asarray(raw_b).size, first_b, nfft, hop, frames_per_row)
    assert n_rows >= 1
    per = max(1, 8192 // frames_per_row)
    out = []
    for r in range(0, n_rows, per):
        k = min(per, n_rows - r)
        a = frame_spectra(raw_a, nfft, hop, first_a, r * frames_per_row, k * frames_per_row, offset)
        b = frame_spectra(raw_b, nfft, hop, first_b, r * frames_per_row, k * frames_per_row, offset)
        out.append(sums_of(a, b, frames_per_row, k, scale))
    return tuple(np.concatenate([o[i] for o in out]) for i in range(4))


def as_result(saa, sbb, sab, msc, nfft, hop, frames_per_row, first_a=0, first_b=0):
    """The restatement's arrays as the object Device.cross_spectrum returns."""
    return gpsjam.CrossSpectrum(saa, sbb, sab, msc, nfft, hop, frames_per_row, first_a, first_b)


@functools.lru_cache(maxsize=None)
def detect_reference(case, frames_per_row=None):
    """The restatement of detect_pair(case) at the detection geometry: (CrossSpectrum of float64 origin, MSC float64)."""
    m = DETECT_M[case] if frames_per_row is None else frames_per_row
    a, b = detect_pair(case)
    saa, sbb, sab, msc = csd(a, b, DETECT_NFFT, DETECT_HOP, m)
    return as_result(saa, sbb, sab, msc, DETECT_NFFT, DETECT_HOP, m), msc


def off_dc(nfft, dc_guard=1):
    """bool[nfft]: the bins the detector may flag."""
    k = np.arange(nfft)
    return np.abs(np.where(k >= nfft // 2, k - nfft, k)) > dc_guard


def edge_distance(msc, frames_per_row, p_fa=P_FA, dc_guard=1):
    """Smallest relative distance of any finite off-DC cell to the threshold."""
    from gpsjam import coherence as co
    thr = co.threshold(frames_per_row, p_fa)
    v = msc[:, off_dc(msc.shape[1], dc_guard)]
    v = v[np.isfinite(v)]
    return float(np.min(np.abs(v / thr - 1.0)))


def full_band_lag(a, b, n=TWO_CORR_SAMPLES):
    """argmax |correlate(x_b, x_a, 'full')| of the first n samples, positive when b is delayed (K5's convention)."""
    xa, xb = rr.unpack(a[:2 * n]), rr.unpack(b[:2 * n])
    size = 1 << int(np.ceil(np.log2(2 * n)))
    c = np.fft.ifft(np.fft.fft(xb, size) * np.conj(np.fft.fft(xa, size)))
    k = int(np.argmax(np.abs(c)))
    return k if k < size // 2 else k - size


power_db = sr.power_db


# ---------------------------------------------------------------------------------------------------- GPU parity
PARITY_M = sr.PARITY_M                      # (2, 5, 17)
BOUNDARY_NFFT = sr.BOUNDARY_NFFT
BOUNDARY_HOP = sr.BOUNDARY_HOP
BOUNDARY_M = sr.BOUNDARY_M
parity_hops = sr.parity_hops                # nfft and nfft / 2 + 37


@functools.lru_cache(maxsize=None)
def parity_spectra(nfft, hop, first_a=PARITY_FIRST_A, first_b=PARITY_FIRST_B, offset=127.5):
    """Frame spectra (A, B) of parity_pair() at one geometry, every frame pair that fits; computed once and shared."""
    a, b = parity_pair()
    n = rows_that_fit(a.size, first_a, b.size, first_b, nfft, hop, 1)
    sa, sb = frame_spectra(a, nfft, hop, first_a, 0, n, offset), frame_spectra(b, nfft, hop, first_b, 0, n, offset)
    sa.setflags(write=False)
    sb.setflags(write=False)
    return sa, sb


worst = {"saa": 0.0, "sbb": 0.0, "sab": 0.0, "msc_ulp": 0.0}   # largest errors seen, relative to the tolerance's own reference


def check_msc(saa, sbb, sab, msc, what):
    """d_msc against the formula in float64 on the float32 values the call wrote."""
    want = coherence(saa, sbb, sab)
    dead = saa.astype(np.float64) * sbb.astype(np.float64) == 0
    assert np.array_equal(np.isnan(msc), dead), (what, "NaN exactly where Saa * Sbb == 0")
    live = ~dead
    if live.any():
        w32 = want[live].astype(np.float32)
        ulps = np.abs(msc[live].astype(np.float64) - want[live]) / np.spacing(np.abs(w32)).astype(np.float64)
        worst["msc_ulp"] = max(worst["msc_ulp"], float(ulps.max()))
        assert ulps.max() <= 2.0, (what, float(ulps.max()))


def compare(got, ref, what):
    """GPU sums against the restatement's (Saa, Sbb, Sab, MSC) of float64."""
    saa, sbb, sab, msc = got
    raa, rbb, rab, _ = ref
    assert saa.shape == raa.shape == sbb.shape == sab.shape, what
    ma, mb = raa.max(axis=1, keepdims=True), rbb.max(axis=1, keepdims=True)
    ea, eb = float(np.max(np.abs(saa - raa) / ma)), float(np.max(np.abs(sbb - rbb) / mb))
    cross = np.sqrt(ma * mb)
    eab = float(max(np.max(np.abs(sab.real - rab.real) / cross), np.max(np.abs(sab.imag - rab.imag) / cross)))
    worst["saa"], worst["sbb"], worst["sab"] = max(worst["saa"], ea), max(worst["sbb"], eb), max(worst["sab"], eab)
    assert ea <= S1_TOL, (what, "Saa", ea)
    assert eb <= S1_TOL, (what, "Sbb", eb)
    assert eab <= S1_TOL, (what, "Sab", eab)
    if msc is not None:
        check_msc(saa, sbb, sab, msc, what)
