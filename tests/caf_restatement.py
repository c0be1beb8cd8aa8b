"""The cross-ambiguity search of include/gpsjam.h (gj_xcorr_caf_dev), restated in numpy / scipy -- the yardstick of
tests/test_xcorr_caf_host.py and tests/xcorr_caf/.

Definition: L = the power of two >= 2n - 1, at least 65536.  For a pair (i, j) and an integer bin b

    x_j^(b)[t] = x_j[t] * exp(-2 pi i b t / L),   t = 0 .. n-1
    c_b        = scipy.signal.correlate(x_j^(b), x_i, 'full')          (skrypty/triangulateTDOA.py:86)

and the answer is the (b, m) with the largest |c_b[m]|; lag = m - (n - 1).  Ties: larger value, then the earlier bin,
then the smaller m (numpy.argmax).  x = (I - 127.5) + j(Q - 127.5).

Two evaluations:
* ``direct``: the words above taken literally -- rotate the unpacked slice in complex64, one scipy.signal.correlate per bin;
* ``sweep``:  float64, by the identity FFT_L(x_j^(b))[k] = Z_j[(k + b) mod L] (the slice is zero-padded to L, so the
  rotation is an exact shift of the spectrum): one forward transform per antenna, one inverse per bin.

Also here: the seeded test captures (a common wide-band source seen by receivers with their own delay and frequency
offset), shared by the CPU and the GPU tests."""
from typing import NamedTuple

import numpy as np
from scipy import signal

LAG_NEAR_TIE = 2e-5          # skrypty/triangulateTDOA.py
N_REF = 50000                # the reference's CORRELATION_SLICE_SIZE
BINS_REF = (-64, 129)        # bins -64 .. 64
#: (delay in samples, offset in bins) of antenna 1 against antenna 0
CASES = [(37, 21.0), (-5, 23.4), (12, -57.0), (3, 0.0)]
#: the same for a third antenna, per case (every pairwise offset stays inside BINS_REF and off the half bins)
THIRD = [(-11, -14.0), (9, -8.3), (-20, 6.0), (-7, 5.0)]


def fft_len(n: int) -> int:
    L = 65536
    while L < 2 * n - 1:
        L *= 2
    return L


def unpack(raw: np.ndarray) -> np.ndarray:
    raw = np.asarray(raw, np.uint8)
    return ((raw[0::2].astype(np.float32) - 127.5) + 1j * (raw[1::2].astype(np.float32) - 127.5)).astype(np.complex64)


def make_antennas(n, specs, seed, amplitude=30.0, sigma=6.25):
    """uint8 I/Q slices of n samples, one per (delay, offset_bins) of ``specs``: amplitude x a common unit-variance
    complex white Gaussian source delayed by `delay` samples and multiplied by exp(2 pi i offset t / L), + complex
    Gaussian noise (sigma per component), + 127.5, rounded and clipped."""
    rng = np.random.default_rng(seed)
    L = fft_len(n)
    pad = max(abs(int(d)) for d, _ in specs) + 1
    src = (rng.normal(size=n + 2 * pad) + 1j * rng.normal(size=n + 2 * pad)) / np.sqrt(2.0)
    t = np.arange(n)
    out = []
    for d, f in specs:
        z = amplitude * src[pad - int(d):pad - int(d) + n] * np.exp(2j * np.pi * float(f) * t / L)
        z = z + rng.normal(0, sigma, n) + 1j * rng.normal(0, sigma, n)
        iq = np.empty(2 * n)
        iq[0::2], iq[1::2] = z.real + 127.5, z.imag + 127.5
        out.append(np.clip(np.round(iq), 0, 255).astype(np.uint8))
    return out


class BinPeak(NamedTuple):
    lag: int
    peak: float
    margin: float     # 1 - (largest |c| at any other lag of this bin) / peak


def _pick(mag: np.ndarray, n: int) -> BinPeak:
    m = int(np.argmax(mag))
    peak = float(mag[m])
    other = float(max(mag[:m].max(initial=0.0), mag[m + 1:].max(initial=0.0)))
    return BinPeak(m - (n - 1), peak, 1.0 - other / peak if peak > 0 else 0.0)


def direct_bin(raw_j, raw_i, b: int) -> BinPeak:
    """One bin, the definition taken literally (complex64 operands, scipy.signal.correlate)."""
    xj, xi = unpack(raw_j), unpack(raw_i)
    n = xi.size
    rot = np.exp(-2j * np.pi * int(b) * np.arange(n) / fft_len(n))
    c = signal.correlate((xj * rot).astype(np.complex64), xi, mode="full")
    return _pick(np.abs(c), n)


def sweep(raw_j, raw_i, bin_first: int, n_bins: int):
    """Every bin of the range by spectrum shift in float64: a list of BinPeak."""
    xj, xi = unpack(raw_j).astype(np.complex128), unpack(raw_i).astype(np.complex128)
    n, L = xi.size, fft_len(xi.size)
    Zj, Zi = np.fft.fft(xj, L), np.fft.fft(xi, L)
    out = []
    for b in range(bin_first, bin_first + n_bins):
        c = np.fft.ifft(np.roll(Zj, -b) * np.conj(Zi))          # c[lag mod L] = sum_t x_j^(b)[t + lag] conj(x_i[t])
        out.append(_pick(np.abs(np.concatenate([c[L - (n - 1):], c[:n]])), n))
    return out


class Surface(NamedTuple):
    lag: int
    bin: int
    peak: float
    margin_lag: float
    margin_bin: float
    bins: list        # BinPeak per bin


def winner(bins, bin_first: int) -> Surface:
    """The pair's answer from its per-bin records: larger peak first, then the earlier bin."""
    peaks = np.array([r.peak for r in bins])
    k = int(np.argmax(peaks))
    others = np.delete(peaks, k)
    mb = 1.0 - float(others.max()) / peaks[k] if others.size and peaks[k] > 0 else (1.0 if peaks[k] > 0 else 0.0)
    return Surface(bins[k].lag, bin_first + k, float(peaks[k]), bins[k].margin, mb, list(bins))


def search(raw_j, raw_i, bin_first: int, n_bins: int) -> Surface:
    return winner(sweep(raw_j, raw_i, bin_first, n_bins), bin_first)


def search_direct(raw_j, raw_i, bin_first: int, n_bins: int) -> Surface:
    return winner([direct_bin(raw_j, raw_i, b) for b in range(bin_first, bin_first + n_bins)], bin_first)


def plain_lag(raw_j, raw_i) -> int:
    """The reference's call on the slices as they are (skrypty/triangulateTDOA.py:86-89)."""
    xj, xi = unpack(raw_j), unpack(raw_i)
    c = signal.correlate(xj, xi, mode="full")
    return int(np.argmax(np.abs(c))) - (xi.size - 1)


P3 = [(0, 1), (0, 2), (1, 2)]


P7 = P3 + [(1, 0), (2, 0), (0, 0), (2, 2)]     # more than 2 x antennas: K5's many-pair path
