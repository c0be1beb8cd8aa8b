"""Floor-free per-bin interference detection from the spectral kurtosis (``Device.spectral_kurtosis``, gj_sk_dev).

For every bin the estimator compares sum P^2 with (sum P)^2 over M short spectra (Nita & Gary).  Gaussian noise gives
SK = 1 whatever its level or the passband's shape, so no noise floor, no quiet part and no onset are needed; a steady
carrier pulls its bin toward 0, anything intermittent (pulses, a chirp that crosses the bin) pushes it above 1.  The
estimator integrates over M frames: a tone that no single frame's peak shows is still found.

Two blind spots are inherent: a Gaussian broadband jammer has SK = 1, and so has a pulse train of exactly 50 % duty
(pulsedJammer.py's default).  Both raise the power, which K1's threshold and ``classify`` see: this module complements
them, it does not replace them.

The sums behind SK also feed the excisor: S1 / M is the mean of the very P_f[k] that gj_excise_dev compares with its
threshold, so ``excision_threshold`` goes to ``mitigate.clean(..., threshold=...)`` as it is.

    python -m gpsjam.kurtosis IN.bin [--nfft N] [--frames-per-row M] [--sigmas S]

prints the flagged bands.

Nothing here computes on the CPU but the decisions on the rows x nfft sums.
"""
from __future__ import annotations

from typing import List, NamedTuple

import numpy as np

from . import SpectralKurtosis, _bands


class Detection(NamedTuple):
    """Per-bin flags in FFT order and the band (lo, hi) they were decided with."""
    steady: np.ndarray          # bool[nfft]: more than half of the rows lie below the band
    intermittent: np.ndarray    # bool[nfft]: more than half of the rows lie above it
    lo: float
    hi: float

    @property
    def flagged(self) -> np.ndarray:
        return self.steady | self.intermittent


class Band(NamedTuple):
    """A contiguous run of flagged bins of one kind.  first_bin .. last_bin are FFT-order indices of the run's ends in
    ascending frequency (across DC a run passes from nfft - 1 to 0; the band's two ends, nfft/2 - 1 and nfft/2, are never
    joined: a run through them comes back as two); the frequencies are the outer edges of those bins."""
    kind: str                   # "steady" or "intermittent"
    first_bin: int
    last_bin: int
    n_bins: int
    freq_lo_hz: float
    freq_hi_hz: float
    median_sk: float


class Scan(NamedTuple):
    result: SpectralKurtosis
    detection: Detection
    bands: List[Band]


def band(frames_per_row: int, sigmas: float = 4.0):
    """(lo, hi) = 1 -+ sigmas * 2 / sqrt(M): 2 / sqrt(M) is the estimator's standard deviation under Gaussian noise."""
    m = int(frames_per_row)
    if m < 2:
        raise ValueError("frames_per_row must be >= 2")
    half = float(sigmas) * 2.0 / np.sqrt(m)
    return 1.0 - half, 1.0 + half


def detect(result: SpectralKurtosis, sigmas: float = 4.0) -> Detection:
    """A bin is ``steady`` when more than half of the rows lie below the band and ``intermittent`` when more than half
    lie above it.  A NaN cell (a bin without power) never votes."""
    lo, hi = band(result.frames_per_row, sigmas)
    sk = result.sk.astype(np.float64)
    rows = sk.shape[0]
    with np.errstate(invalid="ignore"):
        below, above = np.sum(sk < lo, axis=0), np.sum(sk > hi, axis=0)
    return Detection(2 * below > rows, 2 * above > rows, lo, hi)


def bands(result: SpectralKurtosis, detection: Detection, fs: float = 2.048e6) -> List[Band]:
    """Contiguous flagged runs of one kind, in ascending frequency (fftshift order), with the median SK of their cells."""
    kinds = np.where(detection.steady, 1, np.where(detection.intermittent, 2, 0))
    return [Band("steady" if kind == 1 else "intermittent", *run) for kind, *run in _bands.runs(kinds, result.sk, fs)]


def excision_threshold(result: SpectralKurtosis, detection: Detection, rise_db: float = 12.0) -> np.ndarray:
    """float32[nfft] for gj_excise_dev (``mitigate.clean(..., threshold=...)``).  The per-bin floor is the mean of S1 / M
    over the cells whose SK lies inside the band; a bin without such a cell, and every ``intermittent`` bin, takes the
    median floor of the unflagged bins.  The threshold is that floor times 10^(rise_db / 10); ``steady`` bins get -1, a
    fixed notch.  ValueError when no bin is unflagged."""
    free = ~detection.flagged
    sk = result.sk.astype(np.float64)
    with np.errstate(invalid="ignore"):
        inside = (sk >= detection.lo) & (sk <= detection.hi)
    mean_p = result.s1.astype(np.float64) / result.frames_per_row
    n_in = inside.sum(axis=0)
    floor = np.where(n_in > 0, np.where(inside, mean_p, 0.0).sum(axis=0) / np.maximum(n_in, 1), np.nan)
    known = free & (n_in > 0)
    if not known.any():
        raise ValueError("no unflagged bin with a cell inside the band: nothing to take the noise floor from")
    flat = float(np.median(floor[known]))
    floor = np.where((n_in == 0) | detection.intermittent, flat, floor)
    thr = floor * 10.0 ** (float(rise_db) / 10.0)
    return np.where(detection.steady, -1.0, thr).astype(np.float32)


def scan(dev, capture, fs: float = 2.048e6, nfft: int = 256, frames_per_row: int = 256, sigmas: float = 4.0) -> Scan:
    """``dev.spectral_kurtosis`` at hop = nfft over the whole capture, ``detect`` and ``bands``."""
    result = dev.spectral_kurtosis(capture, nfft=nfft, frames_per_row=frames_per_row)
    detection = detect(result, sigmas)
    return Scan(result, detection, bands(result, detection, fs))


def main(argv=None) -> int:
    import argparse
    from . import Device
    ap = argparse.ArgumentParser(prog="python -m gpsjam.kurtosis", description="print the bands the spectral kurtosis flags")
    ap.add_argument("input")
    ap.add_argument("--nfft", type=int, default=256)
    ap.add_argument("--frames-per-row", type=int, default=256)
    ap.add_argument("--sigmas", type=float, default=4.0)
    ap.add_argument("--fs", type=float, default=2.048e6)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv)
    with Device(args.device) as dev:
        with dev.capture(args.input) as cap:
            res = scan(dev, cap, fs=args.fs, nfft=args.nfft, frames_per_row=args.frames_per_row, sigmas=args.sigmas)
    print(f"{args.input}: {len(res.result)} rows of {args.frames_per_row} frames of {args.nfft} points, band "
          f"{res.detection.lo:.3f} .. {res.detection.hi:.3f}, {len(res.bands)} flagged band(s)")
    for b in res.bands:
        print(f"  {b.kind:12s} {b.freq_lo_hz / 1e3:9.1f} .. {b.freq_hi_hz / 1e3:9.1f} kHz  bins {b.first_bin}..{b.last_bin} "
              f"({b.n_bins})  median SK {b.median_sk:.3f}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
