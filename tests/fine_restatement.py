"""The exact lag-window correlation (gj_xcorr_fine_dev, include/gpsjam.h) restated in numpy int64, and the inputs and
constants of the fine-TDOA tests.  Not a test module: tests/test_fine_host.py and tests/fine/test_round6_gpu.py import it.

    u = 2 byte - o2 for I and Q, o2 = 2 offset;  xa[t], xb[t] = samples first_a + t, first_b + t;  zero outside 0 .. n-1
    C4[k].re = sum_t uI_b[t+k] uI_a[t] + uQ_b[t+k] uQ_a[t]
    C4[k].im = sum_t uQ_b[t+k] uI_a[t] - uI_b[t+k] uQ_a[t]            k = lag_center - R .. lag_center + R
    blocks[m] = the same over t in [4096 m, 4096 (m + 1)) alone;  total = sum of the blocks

Everything is exact: the GPU is held to every bit of every total and every record.  The estimator (gpsjam/tdoa.py) is
NOT restated: the tests feed it these integers.
"""
import functools

import numpy as np

import blank_restatement as br
import gpsjam
import ridge_restatement as rr

BLOCK = 4096
MAX_HALF = 32
FS = rr.FS
CONVENTIONS = br.CONVENTIONS                # (127.5, 1/127.5): o2 odd;  (128, 1/128): o2 even
BLOCK_BOUND = 4096 * 2 * 510 ** 2           # 2 130 739 200 < 2^31: offsets 0 and 255
# (byte of a, byte of b, offset) -> real part of one full block's record at lag 0; the imaginary part is 0
EXTREME_CASES = {(255, 255, 0): BLOCK_BOUND, (0, 255, 255): 0, (0, 0, 255): BLOCK_BOUND, (0, 255, 127.5): -4096 * 2 * 255 ** 2}


class Fine:
    """total: int64[2R+1][2]; blocks: int64[ceil(n / 4096)][2R+1][2] (every value fits int32); lags: int64[2R+1]."""

    def __init__(self, total, blocks, lags, n_samples):
        self.total, self.blocks, self.lags, self.n_samples = total, blocks, lags, n_samples

    def corr(self, want_blocks=False):
        """What Device.xcorr_fine makes of these integers."""
        c = (self.total[:, 0] + 1j * self.total[:, 1]) / 4.0
        b = (self.blocks[..., 0] + 1j * self.blocks[..., 1]) / 4.0 if want_blocks else None
        return gpsjam.FineCorr(self.lags.copy(), c, b, self.n_samples)


def unpack2(raw, first, n, offset):
    o2 = int(round(2 * offset))
    assert o2 == 2 * offset
    src = np.asarray(raw, np.uint8)[2 * first:2 * (first + n)]
    assert src.size == 2 * n, "the range runs past the capture"
    return 2 * src[0::2].astype(np.int64) - o2, 2 * src[1::2].astype(np.int64) - o2


def fine(raw_a, raw_b, lag_center=0, half_width=16, first_a=0, first_b=0, n_samples=None, offset=127.5):
    """The definition on the bytes of the two captures."""
    if n_samples is None:
        n_samples = min(np.asarray(raw_a).size // 2 - first_a, np.asarray(raw_b).size // 2 - first_b)
    n, R, c = int(n_samples), int(half_width), int(lag_center)
    assert n >= 1 and 0 <= R <= MAX_HALF
    ai, aq = unpack2(raw_a, first_a, n, offset)
    bi, bq = unpack2(raw_b, first_b, n, offset)
    starts = np.arange(0, n, BLOCK)
    lags = np.arange(c - R, c + R + 1, dtype=np.int64)
    blocks = np.zeros((starts.size, lags.size, 2), np.int64)
    for j, k in enumerate(lags.tolist()):
        lo, hi = max(0, -k), min(n, n - k)
        if hi <= lo:
            continue
        re, im = np.zeros(n, np.int64), np.zeros(n, np.int64)
        re[lo:hi] = bi[lo + k:hi + k] * ai[lo:hi] + bq[lo + k:hi + k] * aq[lo:hi]
        im[lo:hi] = bq[lo + k:hi + k] * ai[lo:hi] - bi[lo + k:hi + k] * aq[lo:hi]
        blocks[:, j, 0], blocks[:, j, 1] = np.add.reduceat(re, starts), np.add.reduceat(im, starts)
    assert np.abs(blocks).max() <= BLOCK_BOUND
    return Fine(blocks.sum(axis=0), blocks, lags, n)


# ---------------------------------------------------------------------------------------------------- parity input
PARITY_FIRST_A, PARITY_FIRST_B = 5, 11      # odd on purpose, and different
PARITY_SAMPLES = br.PARITY_SAMPLES          # three whole record blocks and a ragged one: two tiles of the kernel
PARITY_TAIL = 64                            # samples behind the ranges: loud, and never to be read
PARITY_HALVES = (0, 1, 16, 32)
# a block seam of b (-4099), the last lag with an overlap (n - 1) and none at all (n + 40)
PARITY_CENTRES = (0, 1, -1, 37, -4099, PARITY_SAMPLES - 1, PARITY_SAMPLES + 40)
PARITY_DELAY = 3                            # b is a delayed by this many samples, under noise of its own
PARITY_SEED = 917


@functools.lru_cache(maxsize=None)
def parity_captures():
    """Two captures of PARITY_FIRST_x + PARITY_SAMPLES + PARITY_TAIL samples each: one 40-LSB noise source seen through
    two receivers with their own noise, b three samples late, the four corners of the byte range among the samples, and
    everything outside the ranges as loud as bytes get.  Read-only uint8."""
    rng = np.random.default_rng(PARITY_SEED)
    n = PARITY_SAMPLES
    z = rr._noise(rng, n + 64, 40.0 / np.sqrt(2.0)).astype(np.complex128)
    out = []
    for first, shift in ((PARITY_FIRST_A, 0), (PARITY_FIRST_B, PARITY_DELAY)):
        body = rr.quantise(z[32 - shift:32 - shift + n] * np.exp(0.4j * shift) + rr._noise(rng, n, rr.NOISE_SIGMA))
        raw = np.full(2 * (first + n + PARITY_TAIL), 255, np.uint8)
        raw[1:2 * first:2] = 0
        raw[2 * first:2 * (first + n)] = body
        for at, i, q in br.PARITY_EXTREMES:
            raw[2 * (first + at + shift):2 * (first + at + shift) + 2] = (i, q)
        raw.setflags(write=False)
        out.append(raw)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def parity_reference(lag_center, half_width, offset=127.5, n_samples=PARITY_SAMPLES):
    """The restatement of the parity ranges, computed once and shared."""
    a, b = parity_captures()
    return fine(a, b, lag_center, half_width, PARITY_FIRST_A, PARITY_FIRST_B, n_samples, offset)


# ---------------------------------------------------------------------------------------------------- end to end
E2E_JAMMER_LSB, E2E_NOISE_LSB = 40.0, 6.0    # rms |z| of the jammer; sigma per component of each receiver's own noise
E2E_PHASE = 0.7                              # constant phase of receiver b against a, radians
E2E_DELAYS = (3.0, 3.1, 3.25, 3.37, 3.5, 3.63, 3.9, -2.3)
E2E_SIZES = (4096, 50000)                    # 50 000: the reference's CORRELATION_SLICE_SIZE
E2E_BANDS = ("full", "half")
E2E_HALF = 16
E2E_SEED = 2024
E2E_OFFSET_HZ = 60.0
# The worst |lag - truth| over E2E_DELAYS, measured on the CPU with this restatement and gpsjam.tdoa.fine_lag at its
# defaults (tests/test_fine_host.py re-measures every figure to within 10 % and prints it), in samples; the tolerance
# of the CPU and GPU tests is twice that: the factor covers another seed, not another definition.
E2E_CPU_ERROR_MEASURED = {(4096, "full"): 0.0053, (4096, "half"): 0.0062, (50000, "full"): 0.00126, (50000, "half"): 0.0046}
E2E_TOL = {key: 2.0 * v for key, v in E2E_CPU_ERROR_MEASURED.items()}


def e2e_centre(delay):
    """The integer lag the window is centred on: the nearest one, as K5 finds it."""
    return int(np.floor(delay + 0.5))


@functools.lru_cache(maxsize=None)
def e2e_pair(n, band, delay, offset_hz=0.0, carrier=False):
    """(raw_a, raw_b): one Gaussian jammer over the full band or its inner half (a carrier at fs / 16 if asked for) seen
    by two receivers with independent noise; b is late by `delay` samples (a phase ramp over the spectrum of a longer
    stretch, cut from its middle), turned by E2E_PHASE and, if asked for, by offset_hz; both quantised around 127.5."""
    rng = np.random.default_rng(E2E_SEED + n + int(round(1000 * delay)) + (7 if band == "half" else 0))
    pad = 64
    m = n + 2 * pad
    s = E2E_JAMMER_LSB / np.sqrt(2.0)
    z = rng.normal(0.0, s, m) + 1j * rng.normal(0.0, s, m)
    f = np.fft.fftfreq(m)
    Z = np.fft.fft(z)
    if band == "half":
        Z = np.where(np.abs(f) < 0.25, Z * np.sqrt(2.0), 0.0)
    if carrier:
        Z = np.fft.fft(E2E_JAMMER_LSB * np.exp(2j * np.pi * np.arange(m) / 16.0))
    za = np.fft.ifft(Z)[pad:pad + n]
    zb = np.fft.ifft(Z * np.exp(-2j * np.pi * f * delay))[pad:pad + n] * np.exp(1j * E2E_PHASE)
    if offset_hz:
        zb = zb * np.exp(2j * np.pi * offset_hz * np.arange(n) / FS)
    out = []
    for zz in (za, zb):
        zz = zz + rng.normal(0.0, E2E_NOISE_LSB, n) + 1j * rng.normal(0.0, E2E_NOISE_LSB, n)
        iq = np.empty(2 * n, np.float64)
        iq[0::2], iq[1::2] = zz.real, zz.imag
        raw = np.clip(np.floor(iq + 128.0), 0, 255).astype(np.uint8)
        raw.setflags(write=False)
        out.append(raw)
    return tuple(out)
