"""Which bins do two antennas share, and with what delay in each band: decisions on the cross-spectral density of a
capture pair (``Device.cross_spectrum``, gj_csd_dev).

Two receivers see the same jammer under independent noise.  Per bin the magnitude-squared coherence

    MSC = |Sab|^2 / (Saa Sbb),   Saa, Sbb, Sab summed over M frame pairs

is about 1 / M under noise alone and (rho / (1 + rho))^2 in a bin of jammer-to-noise ratio rho.  For Gaussian noise and
independent frames P(MSC > g) = (1 - g)^(M - 1) exactly (Carter), so the threshold for a per-bin false-alarm
probability needs no noise floor and no calibration -- floor-free as the spectral kurtosis is (``gpsjam.kurtosis``), and
sighted exactly where that one is blind: a Gaussian broadband jammer has SK = 1 but is coherent between the antennas,
also when it lies below each receiver's own noise.  Inside a coherent band the slope of Sab's phase is that band's own
delay, so two jammers at once give two delays where a full-band correlation (K5, ``gj_xcorr_fine_dev``) gives the
stronger one's.

Limits:
  * the receivers share a clock.  A frequency offset between them rotates Sab from frame to frame and averages it
    away; feeding a cross-ambiguity bin in is a later change;
  * the residual misalignment of the pair must be small against nfft (``scan`` takes an integer ``lag`` to align by);
  * both dongles have a DC spur, and two constants are perfectly coherent: bins within ``dc_guard`` of bin 0 are never
    flagged.

    python -m gpsjam.coherence A.bin B.bin [--nfft N] [--frames-per-row M] [--p-fa P] [--lag L|k5]

prints the coherent bands and their delays.

What is found can be taken out: ``cancel_weights`` turns the sums into the per-bin weights of the two-antenna canceller
(``Device.cancel``, gj_cancel_dev; ``gpsjam.mitigate.clean_spatial`` joins the two).  With a third antenna,
``spectral_matrix`` takes the sums of the three pairs and ``cancel_weights2`` solves the 2 x 2 system per cell for the
two weights of the three-antenna canceller (``Device.cancel2``, gj_cancel2_dev; ``gpsjam.mitigate.clean_spatial2``).

Nothing here computes on the CPU but the decisions on the rows x nfft numbers.
"""
from __future__ import annotations

import contextlib
from typing import List, NamedTuple, Optional

import numpy as np

from . import CrossSpectrum, _bands, csd_rows

K5_SAMPLES = 65536          # the slice ``scan(lag="k5")`` hands to K5


class Detection(NamedTuple):
    """Per-bin flags in FFT order and the threshold they were decided with."""
    flagged: np.ndarray         # bool[nfft]: more than half of the rows exceed the threshold
    threshold: float
    p_fa: float


class Band(NamedTuple):
    """A contiguous run of flagged bins.  first_bin .. last_bin are FFT-order indices of the run's ends in ascending
    frequency; the frequencies are the outer edges of those bins.  ``delay``: samples by which b lags a in this band
    (``band_delay``), None where it was not estimated."""
    first_bin: int
    last_bin: int
    n_bins: int
    freq_lo_hz: float
    freq_hi_hz: float
    median_msc: float
    delay: Optional[float] = None


class Scan(NamedTuple):
    result: CrossSpectrum
    detection: Detection
    bands: List[Band]
    lag: int                    # the integer lag the pair was aligned by


def threshold(frames_per_row: int, p_fa: float = 1e-6) -> float:
    """The MSC that noise exceeds with probability p_fa in one cell: 1 - p_fa^(1 / (M - 1)).  Exact for Gaussian noise
    and INDEPENDENT frames, that is hop >= nfft; overlapping frames are correlated and exceed it more often."""
    m = int(frames_per_row)
    if m < 2:
        raise ValueError("frames_per_row must be >= 2")
    if not 0.0 < float(p_fa) < 1.0:
        raise ValueError("p_fa must lie in (0, 1)")
    return 1.0 - float(p_fa) ** (1.0 / (m - 1))


def detect(result: CrossSpectrum, p_fa: float = 1e-6, dc_guard: int = 1) -> Detection:
    """A bin is flagged when more than half of the rows exceed ``threshold(M, p_fa)``.  A NaN cell (a bin without
    power) never votes.  Bins within ``dc_guard`` of bin 0 are never flagged (negative: none is exempt)."""
    thr = threshold(result.frames_per_row, p_fa)
    msc = result.msc.astype(np.float64)
    rows = msc.shape[0]
    with np.errstate(invalid="ignore"):
        above = np.sum(msc > thr, axis=0)
    flagged = 2 * above > rows
    flagged &= np.abs(_bands.signed_bins(result.nfft)) > int(dc_guard)
    return Detection(flagged, thr, float(p_fa))


def detect_cells(result: CrossSpectrum, p_fa: float = 1e-6, dc_guard: int = 1) -> Detection:
    """``detect`` without the vote: ``flagged`` is bool[n_rows][nfft], every cell decided on its own row's MSC.  What a
    jammer that is on in a few rows only needs; the false-alarm probability is then ``p_fa`` per cell, not per bin."""
    thr = threshold(result.frames_per_row, p_fa)
    with np.errstate(invalid="ignore"):
        flagged = result.msc.astype(np.float64) > thr
    flagged &= (np.abs(_bands.signed_bins(result.nfft)) > int(dc_guard))[None, :]
    return Detection(flagged, thr, float(p_fa))


def cancel_weights(result: CrossSpectrum, detection: Detection, per_row: bool = True) -> np.ndarray:
    """The per-bin MMSE weights of the two-antenna canceller, W = conj(Sab) / Sbb: the prediction of a's spectrum from
    b's that leaves the least power (``Device.cancel`` subtracts W B from A).  In the flagged bins only, exactly 0
    elsewhere -- the DC guard bins, which no detection flags, and cells with Sbb = 0 or a sum that is not finite.
    ``detection.flagged``: bool[nfft] (``detect``) or bool[n_rows][nfft] (``detect_cells``).
    per_row=True: complex64[n_rows][nfft], each row from its own sums.  per_row=False: complex64[nfft] from the
    row-summed sums, in the bins flagged in any row.  |W|^2 <= Saa / Sbb (Cauchy-Schwarz on the sums)."""
    flagged = np.asarray(detection.flagged, bool)
    sab, sbb = result.sab.astype(np.complex128), result.sbb.astype(np.float64)
    if flagged.shape not in ((result.nfft,), sab.shape):
        raise ValueError(f"flags of shape {flagged.shape} do not fit {sab.shape[0]} rows of {result.nfft} bins")
    if per_row:
        flagged = np.broadcast_to(flagged, sab.shape)
    else:
        sab, sbb = sab.sum(axis=0), sbb.sum(axis=0)
        flagged = flagged.any(axis=0) if flagged.ndim == 2 else flagged
    use = flagged & (sbb > 0) & np.isfinite(sbb) & np.isfinite(sab)
    w = np.zeros(sab.shape, np.complex128)
    w[use] = np.conj(sab[use]) / sbb[use]
    return w.astype(np.complex64)


class SpectralMatrix(NamedTuple):
    """The sums of a capture triple over the same rows (``spectral_matrix``): ``ab.sab`` = sum B conj(A), ``ac.sab`` =
    sum C conj(A), ``bc.sab`` = sum C conj(B); Saa = ``ab.saa``, Sbb = ``ab.sbb``, Scc = ``ac.sbb``."""
    ab: CrossSpectrum
    ac: CrossSpectrum
    bc: CrossSpectrum
    lags: tuple                 # the integer lags (b, c) the auxiliaries were aligned by


def spectral_matrix(dev, main, aux_b, aux_c, lags=(0, 0), nfft: int = 256, frames_per_row: int = 1024,
                    hop: Optional[int] = None) -> SpectralMatrix:
    """The per-bin 3 x 3 spectral matrix of a capture triple: three ``dev.cross_spectrum`` calls, (a,b), (a,c) and (b,c),
    over the same rows of the range all three captures hold.  ``lags``: the integer samples by which each auxiliary lags
    main, or "k5" for K5's integer lag of the first K5_SAMPLES samples of each pair; the triple is aligned by them first.
    Host bytes are uploaded once each.  Three pair calls cost six transforms per frame triple where three would do."""
    nfft, m = int(nfft), int(frames_per_row)
    hop = nfft if hop is None else int(hop)
    with contextlib.ExitStack() as temps:
        cap_a, cap_b, cap_c = dev._residents(temps, main, aux_b, aux_c)
        if isinstance(lags, str):
            if lags != "k5":
                raise ValueError(f'lags must be two integers or "k5", not {lags!r}')
            lag_b, lag_c = _k5_lag(dev, cap_a, cap_b), _k5_lag(dev, cap_a, cap_c)
        else:
            lag_b, lag_c = (int(v) for v in lags)
        first_a = max(0, -lag_b, -lag_c)
        first_b, first_c = first_a + lag_b, first_a + lag_c
        rows = min(csd_rows(cap_a.nbytes, first_a, cap_b.nbytes, first_b, nfft, hop, m),
                   csd_rows(cap_a.nbytes, first_a, cap_c.nbytes, first_c, nfft, hop, m))
        if rows == 0:
            none = np.empty((0, nfft), np.float32)
            return SpectralMatrix(CrossSpectrum(none, none, none, none, nfft, hop, m, first_a, first_b),
                                  CrossSpectrum(none, none, none, none, nfft, hop, m, first_a, first_c),
                                  CrossSpectrum(none, none, none, none, nfft, hop, m, first_b, first_c), (lag_b, lag_c))
        pair = lambda x, y, fx, fy: dev.cross_spectrum(x, y, nfft=nfft, hop=hop, frames_per_row=m, first_a=fx, first_b=fy,
                                                       n_rows=rows)
        return SpectralMatrix(pair(cap_a, cap_b, first_a, first_b), pair(cap_a, cap_c, first_a, first_c),
                              pair(cap_b, cap_c, first_b, first_c), (lag_b, lag_c))


def cancel_weights2(matrix: SpectralMatrix, flagged, loading: float = 1e-6) -> np.ndarray:
    """The per-cell MMSE weights of the three-antenna canceller (``Device.cancel2`` subtracts W1 B and W2 C from A):
    complex64[n_rows][2][nfft], W1 and W2 of every row, solved in float64 from the row's own sums

        W1 Sbb       + W2 Sbc = conj(Sab)
        W1 conj(Sbc) + W2 Scc = conj(Sac)            Sxy = sum Y conj(X)

    in the ``flagged`` cells (bool[n_rows][nfft] or bool[nfft]), exactly 0 elsewhere.  Where det = Sbb Scc - |Sbc|^2 is
    not finite or <= ``loading`` Sbb Scc -- the auxiliaries see the same thing, ``aux_c is aux_b`` included -- the cell
    falls back to the single weight conj(Sax) / Sxx of the auxiliary more coherent with a, the other weight exactly 0;
    where neither auxiliary is usable (Sxx = 0 or a sum that is not finite) both are 0."""
    ab, ac, bc = matrix.ab, matrix.ac, matrix.bc
    sab, sac, sbc = (r.sab.astype(np.complex128) for r in (ab, ac, bc))
    sbb, scc = ab.sbb.astype(np.float64), ac.sbb.astype(np.float64)
    flagged = np.asarray(flagged, bool)
    if flagged.shape not in ((ab.nfft,), sab.shape) or sac.shape != sab.shape or sbc.shape != sab.shape:
        raise ValueError(f"flags of shape {flagged.shape} do not fit {sab.shape[0]} rows of {ab.nfft} bins")
    flagged = np.broadcast_to(flagged, sab.shape)
    with np.errstate(all="ignore"):
        ok_b = (sbb > 0) & np.isfinite(sbb) & np.isfinite(sab)
        ok_c = (scc > 0) & np.isfinite(scc) & np.isfinite(sac)
        det = sbb * scc - (sbc.real * sbc.real + sbc.imag * sbc.imag)
        full = flagged & ok_b & ok_c & np.isfinite(det) & (det > float(loading) * sbb * scc)
        safe = np.where(full, det, 1.0)
        w1 = (np.conj(sab) * scc - np.conj(sac) * sbc) / safe
        w2 = (np.conj(sac) * sbb - np.conj(sab) * np.conj(sbc)) / safe
        # the fallback: the single auxiliary whose coherence with a is larger (|Sax|^2 / Sxx, Saa being common)
        cb = np.where(ok_b, (sab.real ** 2 + sab.imag ** 2) / np.where(ok_b, sbb, 1.0), -1.0)
        cc = np.where(ok_c, (sac.real ** 2 + sac.imag ** 2) / np.where(ok_c, scc, 1.0), -1.0)
        one_b = flagged & ~full & ok_b & (cb >= cc)
        one_c = flagged & ~full & ok_c & ~one_b
        s1 = np.conj(sab) / np.where(ok_b, sbb, 1.0)
        s2 = np.conj(sac) / np.where(ok_c, scc, 1.0)
    w = np.zeros((sab.shape[0], 2, ab.nfft), np.complex128)
    w[:, 0][full], w[:, 1][full] = w1[full], w2[full]
    w[:, 0][one_b] = s1[one_b]
    w[:, 1][one_c] = s2[one_c]
    return w.astype(np.complex64)


def bands(result: CrossSpectrum, detection: Detection, fs: float = 2.048e6) -> List[Band]:
    """Contiguous flagged runs in ascending frequency (fftshift order), with the median MSC of their cells."""
    return [Band(*run) for _, *run in _bands.runs(np.asarray(detection.flagged, bool), result.msc, fs)]


def band_delay(result: CrossSpectrum, band: Band, coarse_lag: int = 0) -> Optional[float]:
    """Samples by which b lags a inside ``band``, plus ``coarse_lag``: the |Sab|-weighted least-squares slope of the
    unwrapped phase of the row-summed Sab over the band's bins, D = -(nfft / 2 pi) d(arg Sab) / dk.  None for a band
    of fewer than 3 bins (a line through two points has no residual to average)."""
    if band.n_bins < 3:
        return None
    n, signed = result.nfft, _bands.signed_bins(result.nfft)
    at = int(signed[band.first_bin]) + n // 2                  # the band's place in ascending frequency
    bins = _bands.shifted_order(n)[at:at + band.n_bins]
    s = result.sab[:, bins].astype(np.complex128).sum(axis=0)
    w = np.abs(s)
    if not np.all(np.isfinite(w)) or w.sum() == 0:
        return None
    k = signed[bins].astype(np.float64)
    phase = np.unwrap(np.angle(s))
    km, pm = np.sum(w * k) / w.sum(), np.sum(w * phase) / w.sum()
    slope = np.sum(w * (k - km) * (phase - pm)) / np.sum(w * (k - km) ** 2)
    return float(-slope * n / (2.0 * np.pi) + coarse_lag)


def _k5_lag(dev, cap_a, cap_b) -> int:
    n = min(K5_SAMPLES, cap_a.nsamples, cap_b.nsamples)
    lags, _ = dev.xcorr_lags_at([cap_a, cap_b], [0, 0], n, [(0, 1)])
    return int(lags[0])


def scan(dev, a, b, lag=0, fs: float = 2.048e6, nfft: int = 256, frames_per_row: int = 1024, p_fa: float = 1e-6,
         dc_guard: int = 1, hop: Optional[int] = None) -> Scan:
    """``dev.cross_spectrum`` over the whole pair, ``detect``, ``bands``, and each band's delay.  The pair is aligned
    by the integer ``lag`` first (samples by which b lags a): a positive lag advances first_b, a negative one first_a.
    ``lag="k5"`` takes K5's integer lag of the first K5_SAMPLES samples."""
    with contextlib.ExitStack() as temps:
        cap_a, cap_b = dev._residents(temps, a, b)
        lag = _k5_lag(dev, cap_a, cap_b) if lag == "k5" else int(lag)
        result = dev.cross_spectrum(cap_a, cap_b, nfft=nfft, hop=hop, frames_per_row=frames_per_row,
                                    first_a=max(-lag, 0), first_b=max(lag, 0))
    detection = detect(result, p_fa, dc_guard)
    found = [bd._replace(delay=band_delay(result, bd, lag)) for bd in bands(result, detection, fs)]
    return Scan(result, detection, found, lag)


def main(argv=None) -> int:
    import argparse
    from . import Device
    ap = argparse.ArgumentParser(prog="python -m gpsjam.coherence", description="print the bands two captures share and their delays")
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--nfft", type=int, default=256)
    ap.add_argument("--frames-per-row", type=int, default=1024)
    ap.add_argument("--p-fa", type=float, default=1e-6)
    ap.add_argument("--lag", default="0", help="integer samples by which b lags a, or k5")
    ap.add_argument("--fs", type=float, default=2.048e6)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv)
    lag = "k5" if args.lag == "k5" else int(args.lag)
    with Device(args.device) as dev:
        with dev.capture(args.a) as cap_a, dev.capture(args.b) as cap_b:
            res = scan(dev, cap_a, cap_b, lag=lag, fs=args.fs, nfft=args.nfft, frames_per_row=args.frames_per_row, p_fa=args.p_fa)
    print(f"{args.a} / {args.b}: {len(res.result)} rows of {args.frames_per_row} frame pairs of {args.nfft} points, aligned by {res.lag}, "
          f"threshold {res.detection.threshold:.5f} (p_fa {args.p_fa:g}), {len(res.bands)} coherent band(s)")
    for bd in res.bands:
        delay = "       -" if bd.delay is None else f"{bd.delay:+8.3f}"
        print(f"  {bd.freq_lo_hz / 1e3:9.1f} .. {bd.freq_hi_hz / 1e3:9.1f} kHz  bins {bd.first_bin}..{bd.last_bin} ({bd.n_bins})  "
              f"median MSC {bd.median_msc:.3f}  delay {delay} samples")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
