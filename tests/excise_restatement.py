"""The frequency-domain excisor (gj_excise_dev, include/gpsjam.h) restated in float64 numpy, the same computation in
complex64, and the inputs and constants of the excision tests.  Not a test module: tests/test_excise_host.py and
tests/excise/test_round6_gpu.py import it.

    x[t]   = (I_t - offset) + j (Q_t - offset)
    X_f    = fft(w * x[s_f : s_f + N]),  s_f = first_sample + f N/2,  w the periodic Hann window
    P_f[k] = |X_f[k]|^2 * scale^2
    y_f    = ifft(X_f where P_f <= thr else 0)
    y[t]   = y_{f-1}[t - s_{f-1}] + y_f[t - s_f];  u = clip(rint(float32(y + offset)), 0, 255) on samples [N/2, F N/2)
"""
import functools

import numpy as np
import scipy.fft

import ridge_restatement as rr

RECORD64 = np.dtype([("total", np.float64), ("removed", np.float64), ("n_excised", np.int32), ("reserved", np.int32)])

FS = rr.FS
NFFT = rr.PARITY_NFFT                       # 16 .. 4096
CONVENTIONS = ((127.5, 1.0 / 127.5), (128.0, 1.0 / 128.0))
NEAR_TIE = rr.NEAR_TIE                      # no P_f[k] of a GPU input may lie within 1e-4 relative of its threshold
PARITY_SAMPLES = 1 << 15                    # 4096 points still get 15 frames
PARITY_FIRST = 1                            # odd on purpose
PARITY_SIGMA = rr.NOISE_SIGMA               # 6.25 LSB
PARITY_TONE_HZ, PARITY_TONE_AMP = rr.PARITY_TONE_HZ, 60.0
PARITY_CHIRP_AMP = 40.0
PARITY_RISE = 16.0                          # flat threshold: 16 x the nominal noise floor (12 dB)
# chosen so that the restatement alone keeps every P_f[k] of every parity input NEAR_TIE away from its threshold
# (tests/test_excise_host.py asserts it and prints the smallest margin)
PARITY_SEED = 662
# Largest |y_complex64 - y_float64| over the parity inputs (every size, both conventions), measured on the CPU with
# scipy.fft on complex64 input: E32_MEASURED.  A transform with other radices and twiddles than pocketfft errs against
# float64 by a like amount; the factor 8 covers the sum of both and the final + offset.
E32_MEASURED = 2.7499702639488532e-05     # 1.2e-5 at 16 points .. 2.7e-5 at 2048 points
E32 = 2.75e-5
TIE_BAND = 8 * E32


def hann(n):
    return rr.hann(n)


def unpack_lsb(raw, offset=127.5):
    u = np.asarray(raw, np.uint8).astype(np.float64)
    n = u.size // 2
    return (u[0:2 * n:2] - offset) + 1j * (u[1:2 * n:2] - offset)


def frames_loop(n_samples, nfft):
    """gj_excise_frames as the loop it abbreviates."""
    if nfft < 2:
        return 0
    f, s = 0, 0
    while s + nfft <= n_samples:
        f += 1
        s += nfft // 2
    return f


class Excised:
    """out: uint8[2 n_samples]; records: RECORD64[F]; value: float64[2 (F-1) N/2], y + offset of the excised range
    [N/2, F N/2) before rounding, interleaved like the bytes; power: P[F][N]."""

    def __init__(self, out, records, value, power, nfft):
        self.out, self.records, self.value, self.power, self.nfft = out, records, value, power, nfft

    @property
    def lo(self):
        return self.nfft                     # first excised byte (sample N/2)

    @property
    def hi(self):
        return self.records.size * self.nfft    # one past the last excised byte (sample F N/2)


def finish(Y, src, thr, nfft, offset, scale, rechirp=None):
    """What the excisors and the cancellers do alike behind their spectra Y[F][nfft] (complex64 or complex128; the inverse
    keeps that precision): the powers, the mask against `thr` (None: +inf), the inverse, the overlap-add and the bytes
    over a copy of `src`, the bytes of the range.  `rechirp`: factors[F][nfft] that every frame is multiplied with between
    the inverse and the overlap-add, in Y's precision.  Returns (P, cut, sums, value, out); sums = (total, removed,
    n_excised) per frame, for the caller's own record type."""
    h = nfft // 2
    thr = np.full(nfft, np.inf) if thr is None else np.asarray(thr, np.float32).astype(np.float64)
    P = (np.abs(Y.astype(np.complex128)) ** 2) * (scale * scale)
    with np.errstate(invalid="ignore"):
        cut = P > thr[None, :]               # strict; False against NaN
    y = scipy.fft.ifft(np.where(cut, 0, Y).astype(Y.dtype), axis=1)
    if rechirp is not None:
        y = y * rechirp
    y = y.astype(np.complex128)
    t = (y[:-1, h:] + y[1:, :h]).reshape(-1)                     # samples [h, F h)
    value = np.empty(2 * t.size)
    value[0::2], value[1::2] = t.real + offset, t.imag + offset
    out = src.copy()
    out[2 * h:2 * h + value.size] = np.clip(np.rint(value.astype(np.float32)), 0, 255).astype(np.uint8)
    return P, cut, (P.sum(axis=1), np.where(cut, P, 0.0).sum(axis=1), cut.sum(axis=1)), value, out


def excise(raw, thr, nfft, first_sample=0, n_samples=None, offset=127.5, scale=1.0 / 127.5, single=False):
    """The definition on the bytes `raw`.  single=True: the transforms in complex64 (scipy.fft keeps the input's
    precision), everything else alike."""
    raw = np.asarray(raw, np.uint8)
    if n_samples is None:
        n_samples = raw.size // 2 - first_sample
    h = nfft // 2
    nf = frames_loop(n_samples, nfft)
    assert nf >= 1 and first_sample + n_samples <= raw.size // 2
    src = raw[2 * first_sample:2 * (first_sample + n_samples)]
    x = unpack_lsb(src, offset)
    idx = (h * np.arange(nf))[:, None] + np.arange(nfft)[None, :]
    seg = x[idx] * hann(nfft)[None, :]
    if single:
        seg = seg.astype(np.complex64)
    P, _, sums, value, out = finish(scipy.fft.fft(seg, axis=1), src, thr, nfft, offset, scale)
    rec = np.zeros(nf, RECORD64)
    rec["total"], rec["removed"], rec["n_excised"] = sums
    return Excised(out, rec, value, P, nfft)


def tie_distance(value):
    """Distance of every value to the nearest half-integer (where rint changes)."""
    return np.abs(value - np.floor(value) - 0.5)


def threshold_margin(power, thr):
    """Smallest |P / thr - 1| over the finite positive thresholds (inf where there are none)."""
    thr = np.asarray(thr, np.float32).astype(np.float64)
    ok = np.isfinite(thr) & (thr > 0)
    if not ok.any():
        return np.inf
    return float(np.min(np.abs(power[:, ok] / thr[None, ok] - 1.0)))


def noise_floor(nfft, sigma, scale):
    """E P[k] of complex Gaussian noise of `sigma` LSB per component: sum(w^2) * 2 sigma^2 * scale^2."""
    return float(np.sum(hann(nfft) ** 2) * 2.0 * sigma * sigma * scale * scale)


# ---------------------------------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def parity_capture():
    """2^15 samples: noise of sigma 6.25 LSB, a tone and a chirp of the simulator's shapes.  Read-only uint8."""
    rng = np.random.default_rng(PARITY_SEED)
    n = PARITY_SAMPLES
    z = rr._noise(rng, n, PARITY_SIGMA).astype(np.complex128) + rr.tone(n, PARITY_TONE_HZ, PARITY_TONE_AMP) + rr.chirp(n, PARITY_CHIRP_AMP)
    raw = rr.quantise(z)
    raw.setflags(write=False)
    return raw


def parity_threshold(nfft, scale=1.0 / 127.5):
    return np.full(nfft, PARITY_RISE * noise_floor(nfft, PARITY_SIGMA, scale), np.float32)


@functools.lru_cache(maxsize=None)
def parity_reference(nfft, offset=127.5, scale=1.0 / 127.5, single=False):
    """The restatement of parity_capture() from PARITY_FIRST to the end, computed once and shared."""
    return excise(parity_capture(), parity_threshold(nfft, scale), nfft, PARITY_FIRST, None, offset, scale, single)


CLAMP_SAMPLES = 1 << 13
CLAMP_PERIOD = 64             # samples per period of the square wave: bin N / 64 at every size from 64 points on
CLAMP_NFFT = (64, 1024, 4096)


@functools.lru_cache(maxsize=None)
def clamp_capture():
    """A 127-LSB square wave on both components (what a clipped strong tone looks like) plus 1 LSB of noise."""
    rng = np.random.default_rng(11)
    n = CLAMP_SAMPLES
    sq = np.where((np.arange(n) % CLAMP_PERIOD) < CLAMP_PERIOD // 2, 127.0, -127.0)
    z = sq + 1j * np.roll(sq, CLAMP_PERIOD // 4) + rr._noise(rng, n, 1.0)
    raw = rr.quantise(z)
    raw.setflags(write=False)
    return raw


def clamp_threshold(nfft):
    """Negative (always excised) on every bin but the fundamental's +-(N / 64) with a neighbour on each side, and bin 0:
    what remains is the fundamental of 4 / pi * 127 LSB, which overshoots the uint8 range."""
    thr = np.full(nfft, -1.0, np.float32)
    b = nfft // CLAMP_PERIOD
    for k in (0, b - 1, b, b + 1, nfft - b - 1, nfft - b, nfft - b + 1):
        thr[k % nfft] = np.inf
    return thr


# end to end: three C/A signals under a tone that is switched on after a quiet lead-in
E2E_SATS = ((3, 1400.0, 517, 3.0), (17, -3000.0, 1201, 3.0), (25, 5230.0, 88, 3.0))   # prn, doppler, code delay, amplitude
E2E_SIGMA = 10.0
E2E_TONE_HZ, E2E_TONE_AMP = 137e3, 60.0
E2E_LEAD = 1 << 17            # quiet samples in front of the tone: K4's noise estimate and the floor
E2E_AFTER = 1 << 15           # 16 ms after the onset: one acquisition at intg 10 (11 * 2048 samples)
E2E_ONSET_ARGS = dict(noise_samples=65536, window=1000, factor=4.0)
E2E_NFFT, E2E_RISE_DB = 1024, 12.0
E2E_CN0_TOL_DB = 1.0          # twice the 0.5 dB the CPU prototype lost


@functools.lru_cache(maxsize=None)
def e2e_capture(jammer="tone"):
    """uint8 I/Q of E2E_LEAD + E2E_AFTER samples: C/A signals + noise (+ the jammer from sample E2E_LEAD on) + 128, as
    the acquisition tests build theirs.  jammer: "tone", "chirp" or None."""
    from gpsjam import gnss
    n = E2E_LEAD + E2E_AFTER
    rng = np.random.default_rng(4)
    k = np.arange(n)
    z = rng.normal(0, E2E_SIGMA, n) + 1j * rng.normal(0, E2E_SIGMA, n)
    for prn, dop, delay, amp in E2E_SATS:
        chip = ((k - delay) * 1.023e6 / FS) % 1023
        z += amp * gnss.ca_code(prn)[chip.astype(np.int64)] * np.exp(-2j * np.pi * dop * (k / FS))
    if jammer == "tone":
        z[E2E_LEAD:] += rr.tone(E2E_AFTER, E2E_TONE_HZ, E2E_TONE_AMP)
    elif jammer == "chirp":
        z[E2E_LEAD:] += rr.chirp(E2E_AFTER, E2E_TONE_AMP)
    else:
        assert jammer is None
    iq = np.empty(2 * n, np.float64)
    iq[0::2], iq[1::2] = z.real, z.imag
    raw = (np.clip(np.round(iq), -128, 127) + 128).astype(np.uint8)
    raw.setflags(write=False)
    return raw


RTOL = 1e-5                                     # of total: the project's figure for a K2 value summed in another order


def compare(got, rec, want, what):
    """GPU bytes and records against an Excised."""
    assert rec.size == want.records.size and got.size == want.out.size, what
    np.testing.assert_array_equal(rec["n_excised"], want.records["n_excised"], err_msg=str(what))
    assert not rec["reserved"].any()
    tot = want.records["total"]
    for key in ("total", "removed"):
        err = float(np.max(np.abs(rec[key] - want.records[key]) / tot))
        assert err <= RTOL, (what, key, err)
    assert np.array_equal(got[:want.lo], want.out[:want.lo]) and np.array_equal(got[want.hi:], want.out[want.hi:]), (what, "edges")
    body, ref = got[want.lo:want.hi].astype(np.int16), want.out[want.lo:want.hi].astype(np.int16)
    clear = tie_distance(want.value) > TIE_BAND
    diff = np.abs(body - ref)
    print(f"{what}: {int(np.sum(diff != 0))} of {diff.size} bytes differ, {int(np.sum(~clear))} lie in the tie band")
    assert not diff[clear].any(), (what, int(np.sum(diff[clear] != 0)), "bytes differ outside the tie band")
    assert diff.max(initial=0) <= 1, (what, int(diff.max()))
