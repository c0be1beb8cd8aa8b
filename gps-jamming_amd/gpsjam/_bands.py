"""Bins in ascending frequency and the contiguous runs of flagged ones: what ``kurtosis.bands``, ``coherence.bands`` and
``coherence.band_delay`` share.  Private to the package."""
import numpy as np


def signed_bins(nfft: int, k=None) -> np.ndarray:
    """The signed index of the FFT-order bins ``k`` (default: every bin): bins from nfft/2 on are negative frequencies."""
    k = np.arange(nfft) if k is None else k
    return np.where(k >= nfft // 2, k - nfft, k)


def shifted_order(nfft: int) -> np.ndarray:
    """The FFT-order bin at every position of the ascending-frequency (fftshift) order."""
    return np.fft.fftshift(np.arange(nfft))


def runs(kinds, cells, fs: float) -> list:
    """The runs of equal non-zero ``kinds`` (int[nfft] in FFT order, 0: not flagged), contiguous in ascending frequency and
    lowest first, as (kind, first_bin, last_bin, n_bins, freq_lo_hz, freq_hi_hz, median): FFT-order bins of the run's ends,
    outer edges of those bins, median of the finite ``cells[:, run]`` (else NaN).  The order's two ends are not joined."""
    n = len(kinds)
    order = shifted_order(n)
    kind, width, out = np.asarray(kinds, int)[order], float(fs) / n, []
    cuts = np.flatnonzero(np.diff(kind)) + 1                   # the shifted positions where the kind changes
    for at, end in zip(np.r_[0, cuts], np.r_[cuts, n] - 1):
        if kind[at]:
            run = cells[:, order[at:end + 1]].astype(np.float64)
            med = float(np.nanmedian(run)) if np.isfinite(run).any() else float("nan")
            out.append((int(kind[at]), int(order[at]), int(order[end]), int(end - at + 1),
                        float((at - n // 2 - 0.5) * width), float((end - n // 2 + 0.5) * width), med))
    return out
