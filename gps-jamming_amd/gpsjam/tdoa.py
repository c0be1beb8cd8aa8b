"""Fine TDOA: a sub-sample delay from the exact lag-window correlation (``Device.xcorr_fine``, gj_xcorr_fine_dev).

K5 answers with an integer lag, and one sample at 2.048 MHz is 146 m of path.  The GPU part here is the correlation at
the few dozen lags around that answer, summed over as many samples as the caller has: exact integers.  Everything in
this module is host float64 on those 2R + 1 complex numbers, a deterministic function of them.

The estimator is the lag-window (Blackman-Tukey) cross-spectrum: if b is a delayed by D samples, the correlation is
a's autocorrelation shifted to D, and its transform over the window is the jammer's spectrum times exp(-2 pi i f D).
The delay is the slope of that phase over the bins where the jammer has power -- whatever the spectrum's shape, which
is what biases a parabola through three points of |c| (by up to 0.23 sample on a flat-spectrum jammer, whose
correlation is a sinc).

Limits: a narrow-band jammer has few bins with power and so little slope to measure (a carrier
has none: its delay is its phase, modulo a period); receivers without a common sample clock drift, and a drift over the
integration time smears the peak; a frequency offset between the receivers is taken out per FINE_BLOCK samples (2 ms)
only, so ``offset_hz`` holds well under fs / (4 * 4096) = 125 Hz.
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional

import numpy as np

import gpsjam
from gpsjam import FINE_BLOCK, FineCorr, GJ_LAG_INVALID

__all__ = ["FineLag", "fine_lag", "refine", "series", "parabola_lag"]


class FineLag(NamedTuple):
    lag: float        # coarse + delta, samples; positive when b is delayed
    coarse: int       # the window's centre lag
    delta: float      # -slope / 2 pi of the cross-spectrum's phase
    phase: float      # the fitted line's value at f = 0, radians: the constant phase between the receivers
    spread: float     # |S|^2-weighted rms residual of the fit, radians
    ok: bool          # |delta| < 1 and at least 4 bins carried the fit


def _rotated_sum(corr: FineCorr, offset_hz: float, fs: float) -> np.ndarray:
    """The block records with the receivers' frequency offset taken out per block, summed."""
    if corr.blocks is None:
        raise ValueError("offset_hz needs the block records: Device.xcorr_fine(..., want_blocks=True)")
    nb = corr.blocks.shape[0]
    start = FINE_BLOCK * np.arange(nb, dtype=np.float64)
    stop = np.minimum(start + FINE_BLOCK, float(corr.n_samples))
    t_mid = 0.5 * (start + stop)
    rot = np.exp(-2j * np.pi * float(offset_hz) * t_mid / float(fs))
    return (corr.blocks * rot[:, None]).sum(axis=0)


def fine_lag(corr: FineCorr, offset_hz: float = 0.0, fs: float = 2.048e6, n_freqs: int = 64, band: float = 0.8,
             floor: float = 0.1) -> FineLag:
    """The delay of b against a from the 2R + 1 correlation values of ``corr``.

        w[k] = 0.5 + 0.5 cos(pi k / (R + 1)),  k = -R .. R            the lag window
        S[m] = sum_k w[k] c[k0 + k] exp(-2 pi i f_m k)                n_freqs frequencies over the inner `band` of fs
        a |S|^2-weighted least-squares line through the unwrapped phase of S over the contiguous run of bins around
        the strongest one with |S|^2 >= floor * max:  delta = -slope / 2 pi,  lag = k0 + delta

    ``offset_hz``: receiver b sees the source that much higher than receiver a; the block records are rotated back by
    exp(-2 pi i offset_hz t_mid / fs) before they are summed (needs ``want_blocks``; one phase per FINE_BLOCK samples,
    so |offset_hz| must stay well under fs / (4 * FINE_BLOCK) = 125 Hz)."""
    c = np.asarray(corr.c, np.complex128) if offset_hz == 0.0 else _rotated_sum(corr, offset_hz, fs)
    n_lags = c.size
    R = (n_lags - 1) // 2
    if n_lags != 2 * R + 1:
        raise ValueError("an odd number of lags is expected")
    k0 = int(corr.lags[R])
    k = np.arange(-R, R + 1, dtype=np.float64)
    w = 0.5 + 0.5 * np.cos(np.pi * k / (R + 1))
    f = np.linspace(-0.5 * band, 0.5 * band, int(n_freqs))
    S = np.exp(-2j * np.pi * np.outer(f, k)) @ (w * c)
    p = S.real ** 2 + S.imag ** 2
    top = int(np.argmax(p))
    if not np.isfinite(p).all() or p[top] <= 0.0:
        return FineLag(float(k0), k0, 0.0, 0.0, 0.0, False)
    keep = p >= floor * p[top]
    lo = hi = top
    while lo > 0 and keep[lo - 1]:
        lo -= 1
    while hi < p.size - 1 and keep[hi + 1]:
        hi += 1
    sel = slice(lo, hi + 1)
    fs_, ps, ph = f[sel], p[sel], np.unwrap(np.angle(S[sel]))
    if fs_.size < 2:
        return FineLag(float(k0), k0, 0.0, float(ph[0]), 0.0, False)
    sw = ps.sum()
    fm, pm = (ps * fs_).sum() / sw, (ps * ph).sum() / sw
    var = (ps * (fs_ - fm) ** 2).sum()
    slope = (ps * (fs_ - fm) * (ph - pm)).sum() / var
    intercept = pm - slope * fm
    resid = ph - (intercept + slope * fs_)
    spread = float(np.sqrt((ps * resid ** 2).sum() / sw))
    delta = float(-slope / (2.0 * np.pi))
    # the line's value at f = 0, brought back into (-pi, pi]: the unwrapping started at the run's first bin
    phase = float(np.angle(np.exp(1j * intercept)))
    ok = bool(abs(delta) < 1.0 and fs_.size >= 4)
    return FineLag(k0 + delta, k0, delta, phase, spread, ok)


def parabola_lag(corr: FineCorr) -> float:
    """The three-point parabola through |c| at the window's strongest lag: what ``fine_lag`` is measured against
    (tests/test_fine_host.py).  Biased by the correlation's shape; not used by the library."""
    mag = np.abs(np.asarray(corr.c))
    j = int(np.argmax(mag))
    if j == 0 or j == mag.size - 1:
        return float(corr.lags[j])
    den = mag[j - 1] - 2.0 * mag[j] + mag[j + 1]
    return float(corr.lags[j]) + (0.5 * (mag[j - 1] - mag[j + 1]) / den if den != 0.0 else 0.0)


def refine(dev, slice_b, slice_a, half_width: int = 16, offset_hz: float = 0.0, fs: float = 2.048e6, **estimator) -> Optional[FineLag]:
    """K5's integer lag of ``slice_b`` against ``slice_a`` (``Device.xcorr_lags``' convention: positive when b is
    delayed), the lag window centred there over the whole slices, and ``fine_lag`` on it.  The slices: equal-length
    host bytes (uploaded once each) or resident ``Capture``s.  None for a pair K5 calls invalid."""
    with dev._resident(slice_a) as cap_a, dev._resident(slice_b) as cap_b:
        n = min(cap_a.nsamples, cap_b.nsamples)
        lags, _ = dev.xcorr_lags_at([cap_a, cap_b], [0, 0], n, [(0, 1)])
        if int(lags[0]) == GJ_LAG_INVALID:
            return None
        corr = dev.xcorr_fine(cap_a, cap_b, lag_center=int(lags[0]), half_width=half_width, n_samples=n,
                              want_blocks=offset_hz != 0.0)
    return fine_lag(corr, offset_hz=offset_hz, fs=fs, **estimator)


def series(corr: FineCorr, blocks_per_point: int, **estimator) -> List[FineLag]:
    """The fine lag of every ``blocks_per_point`` consecutive block records (the last group may be shorter): how the
    delay moves over a capture.  Needs ``want_blocks``."""
    if corr.blocks is None:
        raise ValueError("series needs the block records: Device.xcorr_fine(..., want_blocks=True)")
    step = int(blocks_per_point)
    if step < 1:
        raise ValueError("blocks_per_point must be at least 1")
    out = []
    for m in range(0, corr.blocks.shape[0], step):
        part = corr.blocks[m:m + step]
        n = min(corr.n_samples - m * FINE_BLOCK, part.shape[0] * FINE_BLOCK)
        out.append(fine_lag(FineCorr(corr.lags, part.sum(axis=0), None, n), **estimator))
    return out
