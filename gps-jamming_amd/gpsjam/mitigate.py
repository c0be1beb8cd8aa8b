"""Interference mitigation: a cleaned capture out of a jammed one (``Device.excise``, gj_excise_dev).

The excisor takes out every bin of every short frame whose power exceeds a per-bin threshold.  This module builds the
threshold the way a receiver does -- the noise floor of the capture's quiet part, raised by ``rise_db`` -- and joins
the pieces: K4's onset (``Device.onset``) cuts the quiet part as ``classify.characterise`` does, K2 (``Device.welch_dev``)
measures its spectrum, the excisor cleans the whole capture.

    python -m gpsjam.mitigate IN.bin OUT.bin [--nfft N] [--rise-db D] [--swept]

writes the cleaned file, byte for byte as long as the input, for gnssdec.

A fast sweep crosses hundreds of bins inside one frame and escapes the per-bin mask.  ``clean_swept`` (``--swept``)
measures its rate (``classify.characterise_swept``), searches a few integer rates around it frame by frame
(gj_chirp_dev), and excises every frame behind the de-chirp of its own rate (gj_excise_chirp_dev).

Nothing here computes on the CPU but the threshold's arithmetic on one PSD row.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np

from . import Capture, excise_frames

QUIET_FRAMES_MIN = 8          # the quiet part must hold 8 nfft samples to supply the floor
WELCH_CHUNK = 2048000         # K2's row length while the floor is measured (one second at 2.048 MHz)


class Cleaned(NamedTuple):
    """Result of ``clean``: the cleaned range as a resident ``Capture`` (the caller frees it), one EXCISE_DTYPE record per
    frame, the threshold that was applied (float32[nfft], FFT order, the units of ``Device.ridge``), where the floor
    under it came from ("quiet part" or "flat median") and the share of the frames' power that was removed."""
    capture: Capture
    records: np.ndarray
    threshold: np.ndarray
    floor_from: str
    removed_share: float


def hann_power(nfft: int) -> float:
    """sum w^2 of the periodic Hann window: 3 N / 8."""
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(int(nfft)) / int(nfft))
    return float(np.sum(w * w))


def floor_from_psd(psd_row, fs: float, nfft: int) -> np.ndarray:
    """Per-bin noise floor in the excisor's P units from K2's PSD: ``psd * fs * sum(w^2)`` undoes K2's density scaling.
    ``psd_row``: K2's UNSHIFTED row(s) at nperseg = nfft; several rows are averaged.  K2 removes every segment's mean,
    which empties bin 0 and, through the window, bins +-1: those three take max(floor[2], floor[N-2])."""
    nfft = int(nfft)
    psd = np.asarray(psd_row, np.float64).reshape(-1, nfft)
    if psd.shape[0] == 0:
        raise ValueError("no PSD row")
    floor = psd.mean(axis=0) * float(fs) * hann_power(nfft)
    patch = max(floor[2], floor[nfft - 2])
    floor[[0, 1, nfft - 1]] = patch
    return floor


def _psd_rows(dev, cap: Capture, n_samples: int, nfft: int, fs: float) -> np.ndarray:
    """K2's unshifted rows of the first n_samples of a resident capture."""
    nbytes = 2 * int(n_samples)
    chunk = min(int(n_samples), WELCH_CHUNK)
    rows = dev.welch_rows(nbytes, chunk, nfft)
    dev.reserve(dev.welch_workspace(nbytes, chunk, nfft))
    d_psd = dev.alloc(4 * max(rows, 1) * nfft)
    try:
        dev.welch_dev(cap.ptr, nbytes, chunk, nfft, fs, d_psd, None, shift=False)
        return d_psd.download(np.float32, rows * nfft).reshape(rows, nfft)
    finally:
        d_psd.free()


def thresholds(dev, capture, nfft: int = 1024, rise_db: float = 12.0, fs: float = 2.048e6, **onset_args):
    """(threshold float32[nfft], floor_from): the per-bin floor times 10^(rise_db / 10).  The floor comes from the
    samples in front of K4's onset (``dev.onset(capture, **onset_args)``), cut as ``classify.characterise`` cuts
    them, when at least 8 nfft samples lie there ("quiet part"); otherwise it is flat, the median over bins of the
    whole capture's floor ("flat median").  A bin of Gaussian noise exceeds a 12-dB threshold with probability e^-16."""
    nfft = int(nfft)
    own = None if isinstance(capture, Capture) else Capture(dev, capture)
    cap = capture if own is None else own
    try:
        k = int(dev.onset(cap, **onset_args).start_index)
        if k >= QUIET_FRAMES_MIN * nfft:
            floor, floor_from = floor_from_psd(_psd_rows(dev, cap, k, nfft, fs), fs, nfft), "quiet part"
        else:
            whole = floor_from_psd(_psd_rows(dev, cap, cap.nsamples, nfft, fs), fs, nfft)
            floor, floor_from = np.full(nfft, np.median(whole)), "flat median"
    finally:
        if own is not None:
            own.free()
    return (floor * 10.0 ** (float(rise_db) / 10.0)).astype(np.float32), floor_from


def clean(dev, capture, nfft: int = 1024, rise_db: float = 12.0, fs: float = 2.048e6, threshold=None, **onset_args) -> Cleaned:
    """The whole capture excised at ``nfft`` points against ``thresholds(...)`` (or a given ``threshold``).
    ``capture``: a resident ``Capture`` or host bytes (uploaded once)."""
    own = None if isinstance(capture, Capture) else Capture(dev, capture)
    cap = capture if own is None else own
    try:
        if threshold is None:
            threshold, floor_from = thresholds(dev, cap, nfft, rise_db, fs, **onset_args)
        else:
            threshold, floor_from = np.ascontiguousarray(threshold, np.float32).reshape(-1), "given"
        if excise_frames(cap.nsamples, nfft) == 0:
            raise ValueError(f"the capture holds {cap.nsamples} samples, fewer than one frame of {int(nfft)}")
        cleaned, rec = dev.excise(cap, threshold, nfft=nfft)
    finally:
        if own is not None:
            own.free()
    total = float(rec["total"].astype(np.float64).sum())
    share = float(rec["removed"].astype(np.float64).sum()) / total if total > 0 else 0.0
    return Cleaned(cleaned, rec, threshold, floor_from, share)


class CleanedSwept(NamedTuple):
    """Result of ``clean_swept``: ``Cleaned``'s fields, the rate every frame was de-chirped with (int32[F], in units of
    fs^2 / nfft^2; 0 where the frame went through the plain mask), the sweep the rate grid was centred on (Hz/s, None
    without one) and whether the chirp-domain excisor ran at all (False: the result is ``clean``'s)."""
    capture: Capture
    records: np.ndarray
    threshold: np.ndarray
    floor_from: str
    removed_share: float
    rates: np.ndarray
    sweep_hz_per_s: Optional[float]
    swept: bool


def sweep_rate_units(sweep_hz_per_s: float, nfft: int, fs: float) -> int:
    """The integer rate nearest to a sweep at nfft points: round(sweep nfft^2 / fs^2)."""
    return int(round(float(sweep_hz_per_s) * float(nfft) ** 2 / float(fs) ** 2))


def clean_swept(dev, capture, nfft: int = 1024, rise_db: float = 12.0, fs: float = 2.048e6, sweep_hz_per_s=None,
                rate_span: int = 8, min_concentration: float = 0.1, threshold=None, **onset_args) -> CleanedSwept:
    """``clean`` for a fast sweep: every frame de-chirped by its own rate, masked, re-chirped (gj_excise_chirp_dev).

    ``sweep_hz_per_s`` None: ``classify.characterise_swept(dev, capture, fs=fs, **onset_args)`` measures it
    (``max_sweep_hz_per_s`` in ``onset_args`` goes to it and nowhere else); any kind but "chirp" is left to ``clean``,
    whose result comes back with ``swept`` False and all rates 0.  Otherwise q0 = round(sweep nfft^2 / fs^2), the
    chirp-rate search runs at hop nfft / 2 over the 2 rate_span + 1 integer rates around q0, gj_chirp_rates_dev keeps
    the best rate of every frame whose de-chirped peak holds at least ``min_concentration`` of its power (0 elsewhere:
    noise, the lead-in, the frame with the saw-tooth's fly-back) and the excisor takes the rates from the device:
    the host sees the records and, for the result, the rates.

    The threshold is FLAT: the median over bins of ``thresholds(...)``'s floor, times the rise.  A de-chirp smears the
    passband's shape over the bins, so a per-bin floor measured on plain frames does not apply behind it; for a capture
    whose floor varies much across the band the median is the best a flat value can do, and that limit stands.  A given ``threshold`` (nfft floats) is used as it is.
    The search refuses rates beyond nfft^2 / 2 in magnitude (GpsJamError, GJ_ERR_INVALID): |q0| + rate_span must stay inside."""
    from . import CHIRP_DTYPE, DevBuf, classify
    nfft, rate_span = int(nfft), int(rate_span)
    onset_only = {k: v for k, v in onset_args.items() if k != "max_sweep_hz_per_s"}
    own = None if isinstance(capture, Capture) else Capture(dev, capture)
    cap = capture if own is None else own
    d_scan = d_rate = None
    try:
        if sweep_hz_per_s is None:
            found = classify.characterise_swept(dev, cap, fs=fs, **onset_args)
            if found.kind != "chirp":
                res = clean(dev, cap, nfft, rise_db, fs, threshold, **onset_only)
                return CleanedSwept(*res, np.zeros(res.records.size, np.int32), None, False)
            sweep_hz_per_s = float(found.sweep_hz_per_s)
        sweep_hz_per_s = float(sweep_hz_per_s)
        if threshold is None:
            per_bin, floor_from = thresholds(dev, cap, nfft, rise_db, fs, **onset_only)
            threshold = np.full(nfft, np.median(per_bin), np.float32)
            floor_from = "flat median" if floor_from == "flat median" else "quiet part, flat median"
        else:
            threshold, floor_from = np.ascontiguousarray(threshold, np.float32).reshape(-1), "given"
        frames = excise_frames(cap.nsamples, nfft)
        if frames == 0:
            raise ValueError(f"the capture holds {cap.nsamples} samples, fewer than one frame of {nfft}")
        q0 = sweep_rate_units(sweep_hz_per_s, nfft, fs)
        first, n_rates = q0 - rate_span, 2 * rate_span + 1
        d_scan = DevBuf(dev, frames * CHIRP_DTYPE.itemsize)
        d_rate = DevBuf(dev, 4 * frames)
        dev.chirp_dev(cap, cap.nbytes, 0, nfft, nfft // 2, frames, 2, first, 1, n_rates, d_scan)
        dev.chirp_rates_dev(d_scan, frames, first, 1, min_concentration, d_rate)
        cleaned, rec = dev.excise_chirp(cap, threshold, d_rate, nfft=nfft)
        rates = d_rate.download(np.int32, frames)
    finally:
        for b in (d_scan, d_rate, own):
            if b is not None:
                b.free()
    total = float(rec["total"].astype(np.float64).sum())
    share = float(rec["removed"].astype(np.float64).sum()) / total if total > 0 else 0.0
    return CleanedSwept(cleaned, rec, threshold, floor_from, share, rates, sweep_hz_per_s, True)


def main(argv=None) -> int:
    import argparse
    from . import Device
    ap = argparse.ArgumentParser(prog="python -m gpsjam.mitigate", description="write a capture with the interference excised")
    ap.add_argument("input")
    ap.add_argument("output")
    ap.add_argument("--nfft", type=int, default=1024)
    ap.add_argument("--rise-db", type=float, default=12.0)
    ap.add_argument("--fs", type=float, default=2.048e6)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--swept", action="store_true", help="chirp-domain excision of a fast sweep (clean_swept)")
    args = ap.parse_args(argv)
    with Device(args.device) as dev:
        with dev.capture(args.input) as cap:
            res = (clean_swept if args.swept else clean)(dev, cap, nfft=args.nfft, rise_db=args.rise_db, fs=args.fs)
            try:
                res.capture.download().tofile(args.output)
            finally:
                res.capture.free()
    print(f"{args.output}: {res.records.size} frames of {args.nfft} points, floor from the {res.floor_from}, "
          f"{100.0 * res.removed_share:.2f} % of the power removed")
    if args.swept:
        print(f"chirp domain: {int(np.count_nonzero(res.rates))} frames de-chirped around {res.sweep_hz_per_s:.4g} Hz/s"
              if res.swept else "chirp domain: no fast sweep found, excised as plain frames")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
