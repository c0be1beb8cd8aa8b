"""Interference mitigation: a cleaned capture out of a jammed one (``Device.excise``, gj_excise_dev).

The excisor takes out every bin of every short frame whose power exceeds a per-bin threshold.  This module builds the
threshold the way a receiver does -- the noise floor of the capture's quiet part, raised by ``rise_db`` -- and joins
the pieces: K4's onset (``Device.onset``) cuts the quiet part as ``classify.characterise`` does, K2 (``Device.welch_dev``)
measures its spectrum, the excisor cleans the whole capture.

    python -m gpsjam.mitigate IN.bin OUT.bin [--nfft N] [--rise-db D] [--swept]
    python -m gpsjam.mitigate IN.bin OUT.bin --pulsed [--window W] [--guard G] [--rise-db D]
    python -m gpsjam.mitigate A.bin OUT.bin --spatial B.bin [--nfft N] [--frames-per-row M] [--p-fa P] [--lag L|k5]
    python -m gpsjam.mitigate A.bin OUT.bin --spatial B.bin --spatial2 C.bin [--lag L|k5] [--lag2 L|k5]
    python -m gpsjam.mitigate A.bin OUT.bin --spoofed B.bin [--peaks K] [--out-b OUT_B.bin] [--tracked]

writes the cleaned file, byte for byte as long as the input (``--spoofed``: as long as the range it cleans), for gnssdec.

A fast sweep crosses hundreds of bins inside one frame and escapes the per-bin mask.  ``clean_swept`` (``--swept``)
measures its rate (``classify.characterise_swept``), searches a few integer rates around it frame by frame
(gj_chirp_dev), and excises every frame behind the de-chirp of its own rate (gj_excise_chirp_dev).

A pulse train -- a gated carrier, gated noise, a sweep that crosses the band in a few samples -- is spread over every
bin of every frame it touches; the per-bin mask wipes those frames or lets the pulses through.  ``clean_pulsed``
(``--pulsed``) blanks in the time domain instead (``Device.blank``, gj_blank_dev): every sample near a short window
whose mean power exceeds the noise floor raised by ``rise_db`` goes to mid-level.

A Gaussian broadband jammer stands above the floor in every bin of its band, sweeps nowhere and has no pulses: none of
the three sees anything to cut.  With a second antenna it can be cancelled: ``clean_spatial`` (``--spatial``) finds the
bins the two captures share (``coherence.scan``, gj_csd_dev), builds the per-bin weights from the same sums
(``coherence.cancel_weights``) and subtracts the auxiliary antenna's weighted spectrum from the main one's
(``Device.cancel``, gj_cancel_dev).  One auxiliary antenna gives one null per bin: a satellite whose inter-antenna phase
is near the jammer's is attenuated with it, and the main antenna's receiver noise rises by up to 1 + |W|^2.

Two Gaussian jammers from different directions in one band leave a single auxiliary half blind: its one null fits one of
them.  With a third antenna ``clean_spatial2`` (``--spatial2``) takes the sums of the three pairs
(``coherence.spectral_matrix``), solves the 2 x 2 system per cell (``coherence.cancel_weights2``) and subtracts both
auxiliaries' weighted spectra (``Device.cancel2``, gj_cancel2_dev): two nulls per bin, the noise rising by up to
1 + |W1|^2 + |W2|^2.

A spoofer is no interference in any of these senses: its signals have the satellites' own codes.  With a second antenna
``spoof.scan_peaks`` tells them by their common direction, and ``clean_spoofed`` (``--spoofed``) takes them out of both
captures by successive interference cancellation: each counterfeit signal rebuilt from its correlator outputs
(``Device.corr_bank``, ``postcorr.amplitudes``) and subtracted (``Device.subtract``, gj_subtract_dev).  A plain
acquisition on the result locks onto the authentic signals.  That is open loop and covers a tenth of a second;
``--tracked`` follows each counterfeit signal with the tracking loops and cleans to the end of the capture
(``spoof.remove_tracked``, gj_subtract_track_dev).

Nothing here computes on the CPU but the threshold's arithmetic on one PSD row or one floor value, the weights'
on the rows x nfft sums, and the amplitudes' on a hundred prompts per signal.
"""
from __future__ import annotations

import contextlib
from typing import List, NamedTuple, Optional

import numpy as np

from . import Capture, _bands, excise_frames

FLOOR_CHUNK_BYTES = 128       # K1's chunk while clean_pulsed reads the floor off a capture without a quiet part: 64 samples
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
    with dev.alloc(4 * max(rows, 1) * nfft) as d_psd:
        dev.welch_dev(cap.ptr, nbytes, chunk, nfft, fs, d_psd, None, shift=False)
        return d_psd.download(np.float32, rows * nfft).reshape(rows, nfft)


def thresholds(dev, capture, nfft: int = 1024, rise_db: float = 12.0, fs: float = 2.048e6, **onset_args):
    """(threshold float32[nfft], floor_from): the per-bin floor times 10^(rise_db / 10).  The floor comes from the
    samples in front of K4's onset (``dev.onset(capture, **onset_args)``), cut as ``classify.characterise`` cuts
    them, when at least 8 nfft samples lie there ("quiet part"); otherwise it is flat, the median over bins of the
    whole capture's floor ("flat median").  A bin of Gaussian noise exceeds a 12-dB threshold with probability e^-16."""
    nfft = int(nfft)
    with dev._resident(capture) as cap:
        k = int(dev.onset(cap, **onset_args).start_index)
        if k >= QUIET_FRAMES_MIN * nfft:
            floor, floor_from = floor_from_psd(_psd_rows(dev, cap, k, nfft, fs), fs, nfft), "quiet part"
        else:
            whole = floor_from_psd(_psd_rows(dev, cap, cap.nsamples, nfft, fs), fs, nfft)
            floor, floor_from = np.full(nfft, np.median(whole)), "flat median"
    return (floor * 10.0 ** (float(rise_db) / 10.0)).astype(np.float32), floor_from


def _removed_share(rec) -> float:
    """The share of the frames' power that the excisor's records say was removed (0 for frames without power)."""
    total = float(rec["total"].astype(np.float64).sum())
    return float(rec["removed"].astype(np.float64).sum()) / total if total > 0 else 0.0


def clean(dev, capture, nfft: int = 1024, rise_db: float = 12.0, fs: float = 2.048e6, threshold=None, **onset_args) -> Cleaned:
    """The whole capture excised at ``nfft`` points against ``thresholds(...)`` (or a given ``threshold``).
    ``capture``: a resident ``Capture`` or host bytes (uploaded once)."""
    with dev._resident(capture) as cap:
        if threshold is None:
            threshold, floor_from = thresholds(dev, cap, nfft, rise_db, fs, **onset_args)
        else:
            threshold, floor_from = np.ascontiguousarray(threshold, np.float32).reshape(-1), "given"
        if excise_frames(cap.nsamples, nfft) == 0:
            raise ValueError(f"the capture holds {cap.nsamples} samples, fewer than one frame of {int(nfft)}")
        cleaned, rec = dev.excise(cap, threshold, nfft=nfft)
    return Cleaned(cleaned, rec, threshold, floor_from, _removed_share(rec))


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
    with dev._resident(capture) as cap:
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
        with DevBuf(dev, frames * CHIRP_DTYPE.itemsize) as d_scan, DevBuf(dev, 4 * frames) as d_rate:
            dev.chirp_dev(cap, cap.nbytes, 0, nfft, nfft // 2, frames, 2, first, 1, n_rates, d_scan)
            dev.chirp_rates_dev(d_scan, frames, first, 1, min_concentration, d_rate)
            cleaned, rec = dev.excise_chirp(cap, threshold, d_rate, nfft=nfft)
            rates = d_rate.download(np.int32, frames)
    return CleanedSwept(cleaned, rec, threshold, floor_from, _removed_share(rec), rates, sweep_hz_per_s, True)


class CleanedPulsed(NamedTuple):
    """Result of ``clean_pulsed``: the cleaned capture (resident; the caller frees it), one BLANK_DTYPE record per
    BLANK_BLOCK samples, the threshold that was applied (mean power per sample in LSB^2, as the float32 the library
    got), where the floor under it came from ("quiet part", "low percentile" or "given"), the share of the capture's
    power that was removed and the share of its samples that were blanked."""
    capture: Capture
    records: np.ndarray
    threshold: float
    floor_from: str
    removed_share: float
    blanked_share: float


def _floor_low_percentile(dev, cap: Capture, floor_pct: float) -> float:
    """``floor_pct``-th percentile of the mean power of the capture's whole 64-sample chunks: K1 (gj_chunk_power_dev)
    and gj_power_threshold_dev's baseline."""
    from . import DevBuf
    nbytes = cap.nbytes // FLOOR_CHUNK_BYTES * FLOOR_CHUNK_BYTES or cap.nbytes // 2 * 2
    n = dev.chunk_count(nbytes, FLOOR_CHUNK_BYTES)
    if n == 0:
        raise ValueError("the capture holds no sample")
    with DevBuf(dev, 4 * n) as d_power, DevBuf(dev, 12) as d_stats:
        dev.chunk_power_dev(cap, nbytes, FLOOR_CHUNK_BYTES, d_power, eps=0.0)
        dev.power_threshold_dev(d_power, n, d_stats, None, pct=float(floor_pct), rise_db=0.0)
        return float(d_stats.download(np.float32, 3)[0])


def clean_pulsed(dev, capture, window: int = 16, guard: int = 8, rise_db: float = 6.0, threshold=None,
                 floor_pct: float = 25.0, noise_samples: int = 200000, onset_window: int = 1000, **onset_args) -> CleanedPulsed:
    """The whole capture through the pulse blanker (``Device.blank``) at ``threshold`` = floor * 10^(rise_db / 10), a
    mean power per sample in LSB^2.  ``capture``: a resident ``Capture`` or host bytes (uploaded once).

    ``window`` and ``guard`` are the blanker's.  K4's own window, which ``clean`` and ``clean_swept`` take as ``window``
    among their ``onset_args``, is ``onset_window`` here; ``noise_samples`` is K4's, and ``onset_args`` holds its ``factor``.

    The floor is K4's ``noise_power`` when the onset ``dev.onset(capture, noise_samples, onset_window, **onset_args)`` lies
    behind the samples that estimate was taken from (``noise_samples``): "quiet part".  Otherwise -- no onset, or a jammer that is on from the
    start -- it is the ``floor_pct``-th percentile of the mean power of 64-sample chunks (K1 and
    gj_power_threshold_dev): "low percentile".  Between the pulses of a train the chunks see noise alone, and a low
    percentile of a chunk mean of noise reads the floor a few tenths of a dB low (215.75 against 227 LSB^2, -0.22 dB, at the 25th
    percentile on a 30 % train): the blanker then triggers slightly early, never late.  A given ``threshold`` is used as
    it is ("given")."""
    with dev._resident(capture) as cap:
        if threshold is not None:
            floor_from = "given"
        else:
            on = dev.onset(cap, noise_samples=int(noise_samples), window=int(onset_window), **onset_args)
            if int(on.start_index) >= int(noise_samples):
                floor, floor_from = float(on.noise_power), "quiet part"
            else:
                floor, floor_from = _floor_low_percentile(dev, cap, floor_pct), "low percentile"
            threshold = floor * 10.0 ** (float(rise_db) / 10.0)
        threshold = float(np.float32(threshold))
        cleaned, rec = dev.blank(cap, threshold, window=window, guard=guard)
    total = int(rec["total"].sum(dtype=np.uint64))
    removed = int(rec["removed"].sum(dtype=np.uint64))
    blanked = int(rec["n_blanked"].sum(dtype=np.int64))
    return CleanedPulsed(cleaned, rec, threshold, floor_from, removed / total if total else 0.0,
                         blanked / cleaned.nsamples if cleaned.nsamples else 0.0)


class CleanedSpatial(NamedTuple):
    """Result of ``clean_spatial``: the cleaned range of ``main`` as a resident ``Capture`` (the caller frees it), one
    CANCEL_DTYPE record per frame, the weights that were applied (complex64[n_sets][nfft], FFT order), the coherence
    scan they came from, the bands that were cancelled (flagged in any row), per band the measured suppression in dB,
    10 log10(sum total_in / sum total) over the frames whose weight set is not zero inside the band, and whether anything
    was cancelled at all (False: nothing coherent was flagged, ``capture`` is a copy of ``main``; ``note`` says so)."""
    capture: Capture
    records: np.ndarray
    weights: np.ndarray
    scan: object
    bands: List
    suppression_db: List[float]
    cancelled: bool
    note: str


def _copy_of_main(cancel, cap, n_aux: int, threshold, nfft: int, scan):
    """The fields the two spatial results share when nothing was flagged: zero weights of ``cancel``'s rank, ``cancel`` run
    with main in the place of every auxiliary, and the note that says so."""
    zero = np.zeros((1, nfft) if n_aux == 1 else (1, n_aux, nfft), np.complex64)
    cleaned, rec = cancel(*[cap] * (1 + n_aux), zero, threshold, nfft=nfft)
    return cleaned, rec, zero, scan, [], [], False, "nothing coherent was flagged: a copy of main"


def _suppression_db(rec, weights, frames_per_set: int, cancelled, nfft: int) -> List[float]:
    """Per cancelled band 10 log10(sum total_in / sum total) of the records ``rec`` over the frames whose weight set is
    not zero inside the band; NaN unless both sums are positive.  ``weights``: [n_sets][n_aux][nfft]."""
    sets = np.minimum(np.arange(rec.size) // frames_per_set, weights.shape[0] - 1)
    t_in, t_out = rec["total_in"].astype(np.float64), rec["total"].astype(np.float64)
    shifted = _bands.shifted_order(nfft)
    suppression = []
    for bd in cancelled:
        at = int(np.flatnonzero(shifted == bd.first_bin)[0])
        active = np.any(weights[:, :, shifted[at:at + bd.n_bins]] != 0, axis=(1, 2))[sets]
        num, den = t_in[active].sum(), t_out[active].sum()
        suppression.append(float(10.0 * np.log10(num / den)) if num > 0 and den > 0 else float("nan"))
    return suppression


def clean_spatial(dev, main, aux, nfft: int = 1024, frames_per_row: int = 256, p_fa: float = 1e-6, lag="k5",
                  threshold=None, fs: float = 2.048e6) -> CleanedSpatial:
    """``main`` with what it shares with ``aux`` cancelled bin by bin (gj_cancel_dev).  ``main`` and ``aux``: resident
    ``Capture``s or host bytes (uploaded once each) of two antennas on one clock.

    ``coherence.scan`` runs at hop = nfft over rows of ``frames_per_row`` frame pairs, aligned by ``lag`` (samples by
    which aux lags main, or "k5").  A cell -- one bin of one row -- whose coherence exceeds the threshold of ``p_fa``
    (``coherence.detect_cells``) gets the weight conj(Sab) / Sbb of its own row's sums, every other cell exactly 0, so a
    row without the jammer goes through untouched.  Row r covers the excisor frames [2 r M, 2 (r + 1) M) with
    M = frames_per_row: the canceller takes one weight set per row at ``frames_per_set`` = 2 M, and the frames behind
    the last whole row use the last set.  ``threshold``: the excisor's mask behind the cancellation, None for none.
    The result covers the aligned range: main from sample max(-lag, 0) on, as long as both captures hold samples.
    With nothing flagged the result is a copy of the whole of ``main`` and ``cancelled`` is False."""
    from . import coherence
    nfft, m = int(nfft), int(frames_per_row)
    with contextlib.ExitStack() as temps:
        cap_a, cap_b = dev._residents(temps, main, aux)
        if excise_frames(cap_a.nsamples, nfft) == 0:
            raise ValueError(f"the capture holds {cap_a.nsamples} samples, fewer than one frame of {nfft}")
        found = coherence.scan(dev, cap_a, cap_b, lag=lag, fs=fs, nfft=nfft, frames_per_row=m, p_fa=p_fa)
        cells = coherence.detect_cells(found.result, p_fa)
        if not cells.flagged.any():
            return CleanedSpatial(*_copy_of_main(dev.cancel, cap_a, 1, threshold, nfft, found))
        weights = coherence.cancel_weights(found.result, cells, per_row=True)
        cleaned, rec = dev.cancel(cap_a, cap_b, weights, threshold, nfft=nfft, first_a=found.result.first_a,
                                  first_b=found.result.first_b, frames_per_set=2 * m)
    union = coherence.Detection(cells.flagged.any(axis=0), cells.threshold, cells.p_fa)
    cancelled = coherence.bands(found.result, union, fs)
    suppression = _suppression_db(rec, weights[:, None], 2 * m, cancelled, nfft)
    return CleanedSpatial(cleaned, rec, weights, found, cancelled, suppression, True, "")


class CleanedSpatial2(NamedTuple):
    """Result of ``clean_spatial2``: ``CleanedSpatial``'s fields -- ``weights`` is complex64[n_sets][2][nfft], W1 and W2 of
    every set, ``scan`` the coherence scan of (main, aux_b) -- and the scans of (main, aux_c) and (aux_b, aux_c)."""
    capture: Capture
    records: np.ndarray
    weights: np.ndarray
    scan: object
    bands: List
    suppression_db: List[float]
    cancelled: bool
    note: str
    scan_c: object
    scan_bc: object


def clean_spatial2(dev, main, aux_b, aux_c, nfft: int = 1024, frames_per_row: int = 256, p_fa: float = 1e-6, lags="k5",
                   threshold=None, fs: float = 2.048e6) -> CleanedSpatial2:
    """``main`` with what it shares with ``aux_b`` and ``aux_c`` cancelled bin by bin (gj_cancel2_dev): ``clean_spatial``
    with two auxiliaries, step by step.  The three captures are resident ``Capture``s or host bytes (uploaded once each)
    of three antennas on one clock.

    ``coherence.spectral_matrix`` runs at hop = nfft over rows of ``frames_per_row`` frame triples, aligned by ``lags``
    (samples by which each auxiliary lags main, or "k5").  A cell is flagged when ``coherence.detect_cells`` flags it for
    (main, aux_b) or for (main, aux_c); a flagged cell gets the 2 x 2 solution of its own row's sums
    (``coherence.cancel_weights2``), every other cell exactly 0, so a row without a jammer goes through untouched.  One
    weight set per row at ``frames_per_set`` = 2 M as in ``clean_spatial``; ``threshold``: the excisor's mask behind the
    cancellation, None for none.  The result covers the aligned range: main from sample max(0, -lag_b, -lag_c) on, as long
    as all three captures hold samples.  With nothing flagged the result is a copy of the whole of ``main`` and
    ``cancelled`` is False."""
    from . import coherence
    nfft, m = int(nfft), int(frames_per_row)
    with contextlib.ExitStack() as temps:
        cap_a, cap_b, cap_c = dev._residents(temps, main, aux_b, aux_c)
        if excise_frames(cap_a.nsamples, nfft) == 0:
            raise ValueError(f"the capture holds {cap_a.nsamples} samples, fewer than one frame of {nfft}")
        mat = coherence.spectral_matrix(dev, cap_a, cap_b, cap_c, lags=lags, nfft=nfft, frames_per_row=m)
        scans = []
        for res, lag in zip(mat, (mat.lags[0], mat.lags[1], mat.lags[1] - mat.lags[0])):
            det = coherence.detect(res, p_fa)
            found = [bd._replace(delay=coherence.band_delay(res, bd, lag)) for bd in coherence.bands(res, det, fs)]
            scans.append(coherence.Scan(res, det, found, lag))
        cells_b, cells_c = coherence.detect_cells(mat.ab, p_fa), coherence.detect_cells(mat.ac, p_fa)
        flagged = cells_b.flagged | cells_c.flagged
        if not flagged.any():
            return CleanedSpatial2(*_copy_of_main(dev.cancel2, cap_a, 2, threshold, nfft, scans[0]), scans[1], scans[2])
        weights = coherence.cancel_weights2(mat, flagged)
        cleaned, rec = dev.cancel2(cap_a, cap_b, cap_c, weights, threshold, nfft=nfft, first_a=mat.ab.first_a,
                                   first_b=mat.ab.first_b, first_c=mat.ac.first_b, frames_per_set=2 * m)
    union = coherence.Detection(flagged.any(axis=0), cells_b.threshold, cells_b.p_fa)
    msc = np.fmax(mat.ab.msc, mat.ac.msc)                     # a band's median MSC: the better auxiliary's, cell by cell
    cancelled = [coherence.Band(*run) for _, *run in _bands.runs(union.flagged, msc, fs)]
    suppression = _suppression_db(rec, weights, 2 * m, cancelled, nfft)
    return CleanedSpatial2(cleaned, rec, weights, scans[0], cancelled, suppression, True, "", scans[1], scans[2])


class CleanedSpoofed(NamedTuple):
    """Result of ``clean_spoofed``: the cleaned ranges of both antennas as resident ``Capture``s of their own (the caller
    frees them), the ``spoof.PeakSpoofReport`` they were cleaned by, one ``spoof.Removal`` per counterfeit signal and
    antenna, and the SUB_DTYPE records of both subtractions.  ``report.spoofed`` False or None: nothing was removed, the
    ranges are byte for byte the input's and the removal lists are empty."""
    capture_a: Capture
    capture_b: Capture
    report: object
    removals_a: List
    removals_b: List
    records_a: np.ndarray
    records_b: np.ndarray


def clean_spoofed(dev, a, b, k: int = 2, search=None, tol: float = 0.15, min_common: int = 4, pfa: float = 1e-3,
                  first_sample: int = 0, duration_s: float = 0.1, dither: bool = True, tracked: bool = False) -> CleanedSpoofed:
    """Two antennas on one clock with the counterfeit signals taken out.  ``spoof.scan_peaks`` (``k`` peaks per PRN) names
    the counterfeit candidates: the ones that share one inter-antenna phase.  When it says ``spoofed``, ``spoof.remove``
    takes them out of ``a`` -- re-observed, one amplitude per code period from the correlator bank, replicas subtracted
    by gj_subtract_dev -- and out of ``b`` with the SAME channels and b's own amplitudes.  What is left holds the
    authentic signals: a plain acquisition on it finds them, and ``spoof.scan`` on the cleaned pair measures their
    phases.  ``a`` and ``b``: resident ``Capture``s or host bytes (uploaded once each); ``search``: as in
    ``spoof.scan``.  The result covers samples first_sample .. + duration_s (``spoof.remove`` states why no more).
    ``tracked``: the candidates are found on those ``duration_s`` as before and then taken out from ``first_sample`` to
    the END of each capture by ``spoof.remove_tracked``: each antenna follows them through tracking loops of its own and
    subtracts with the NCOs those loops had (gj_subtract_track_dev).  ``spoof.remove_tracked`` states the limits: samples
    in front of a signal's first epoch and behind its last whole one keep it, an epoch with a bit flip inside it is
    under-subtracted, and one complex dimension of noise per epoch and signal goes out with the signal."""
    from . import gnss, spoof
    own = search is None
    if own:
        search = gnss.AcqSearch(dev)
    try:
        with dev._resident(a) as cap_a, dev._resident(b) as cap_b:
            report = spoof.scan_peaks(dev, cap_a, cap_b, search, k, tol, min_common, pfa, first_sample, duration_s)
            fakes = report.counterfeit if report.spoofed else []
            if tracked:
                out_a = spoof.remove_tracked(dev, cap_a, fakes, search, first_sample, dither=dither)
            else:
                out_a = spoof.remove(dev, cap_a, fakes, search, first_sample, duration_s, dither)
            try:
                if tracked:
                    out_b = spoof.remove_tracked(dev, cap_b, fakes, search, first_sample, dither=dither)
                else:
                    out_b = spoof.remove(dev, cap_b, fakes, search, first_sample, duration_s, dither, observations=out_a.observations)
            except BaseException:
                out_a.capture.free()
                raise
    finally:
        if own:
            search.close()
    return CleanedSpoofed(out_a.capture, out_b.capture, report, out_a.removals, out_b.removals, out_a.records, out_b.records)


def _write(capture: Capture, path) -> None:
    """A result's capture written to ``path`` and freed, whatever the writing does."""
    try:
        capture.download().tofile(path)
    finally:
        capture.free()


def _print_bands(res) -> None:
    """One line per cancelled band of a spatial result, with the suppression measured in it."""
    for bd, db in zip(res.bands, res.suppression_db):
        print(f"  {bd.freq_lo_hz / 1e3:9.1f} .. {bd.freq_hi_hz / 1e3:9.1f} kHz  ({bd.n_bins} bins)  median MSC {bd.median_msc:.3f}  "
              f"suppression {db:.1f} dB")


def main(argv=None) -> int:
    import argparse
    from . import Device
    ap = argparse.ArgumentParser(prog="python -m gpsjam.mitigate", description="write a capture with the interference excised")
    ap.add_argument("input")
    ap.add_argument("output")
    ap.add_argument("--nfft", type=int, default=1024)
    ap.add_argument("--rise-db", type=float, default=None, help="default: 12 dB, 6 dB with --pulsed")
    ap.add_argument("--fs", type=float, default=2.048e6)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--swept", action="store_true", help="chirp-domain excision of a fast sweep (clean_swept)")
    ap.add_argument("--pulsed", action="store_true", help="time-domain blanking of a pulse train (clean_pulsed; --rise-db defaults to 6)")
    ap.add_argument("--window", type=int, default=16, help="--pulsed: samples of the power window")
    ap.add_argument("--guard", type=int, default=8, help="--pulsed: samples blanked on either side of a detection")
    ap.add_argument("--spatial", metavar="B.bin", default=None,
                    help="cancel what the input shares with this second antenna's capture (clean_spatial)")
    ap.add_argument("--spatial2", metavar="C.bin", default=None,
                    help="with --spatial: a third antenna's capture, two nulls per bin (clean_spatial2)")
    ap.add_argument("--lag2", default=None, help="--spatial2: integer samples by which C lags the input, or k5 (default: --lag)")
    ap.add_argument("--frames-per-row", type=int, default=256, help="--spatial: frame pairs per weight set")
    ap.add_argument("--p-fa", type=float, default=1e-6, help="--spatial: false-alarm probability per cell")
    ap.add_argument("--lag", default="k5", help="--spatial: integer samples by which B lags the input, or k5")
    ap.add_argument("--spoofed", metavar="B.bin", default=None,
                    help="take the counterfeit signals out that the input shares with this second antenna's capture (clean_spoofed); "
                         "the output holds ONLY the cleaned range, --duration seconds (0.1) from --first-sample, not the whole input")
    ap.add_argument("--peaks", type=int, default=2, metavar="K", help="--spoofed: peaks searched per PRN")
    ap.add_argument("--out-b", metavar="OUT_B.bin", default=None, help="--spoofed: also write the second antenna's cleaned range")
    ap.add_argument("--first-sample", type=int, default=0, help="--spoofed: where the cleaned range starts")
    ap.add_argument("--duration", type=float, default=0.1, help="--spoofed: seconds of the cleaned range")
    ap.add_argument("--tracked", action="store_true",
                    help="--spoofed: follow the counterfeit signals with tracking loops and clean from --first-sample to the end of the "
                         "input (spoof.remove_tracked); --duration is then the part the signals are found on")
    args = ap.parse_args(argv)
    if sum(map(bool, (args.pulsed, args.swept, args.spatial, args.spoofed))) > 1:
        ap.error("--pulsed, --swept, --spatial and --spoofed exclude each other")
    if args.spatial2 and not args.spatial:
        ap.error("--spatial2 needs --spatial")
    if args.spoofed:
        from . import gnss, spoof
        with Device(args.device) as dev:
            search = gnss.AcqSearch(dev, fs=args.fs)
            try:
                with dev.capture(args.input) as cap, dev.capture(args.spoofed) as aux:
                    res = clean_spoofed(dev, cap, aux, k=args.peaks, search=search, first_sample=args.first_sample,
                                        duration_s=args.duration, tracked=args.tracked)
                    try:
                        res.capture_a.download().tofile(args.output)
                        if args.out_b:
                            res.capture_b.download().tofile(args.out_b)
                    finally:
                        res.capture_a.free()
                        res.capture_b.free()
            finally:
                search.close()
        rep = res.report
        verdict = "no verdict (too few PRNs)" if rep.spoofed is None else ("SPOOFED" if rep.spoofed else "not flagged")
        print(f"{args.output}: {res.capture_a.nsamples} samples from sample {args.first_sample}, {len(rep.candidates)} significant peak(s), "
              f"{len(rep.common_prns)} PRN(s) in one arc: {verdict}" + ("" if rep.spoofed else ", written as it came"))
        spoof._print_candidates(f"significant peaks on the input (up to {args.peaks} per PRN)", rep.candidates)
        if rep.spoofed:
            spoof._print_candidates("counterfeit (in the arc)", rep.counterfeit)
            spoof._print_candidates("authentic (outside the arc, same PRNs)", rep.authentic)
            spoof._print_removals("removed from the input", res.removals_a)
            spoof._print_removals(f"removed from {args.spoofed}", res.removals_b)
            print(f"bytes clipped: {int(res.records_a['n_clipped'].sum())} and {int(res.records_b['n_clipped'].sum())}")
        return 0
    if args.spatial2:
        as_lag = lambda v: "k5" if v == "k5" else int(v)
        lag_b, lag_c = as_lag(args.lag), as_lag(args.lag if args.lag2 is None else args.lag2)
        lags = "k5" if lag_b == lag_c == "k5" else (lag_b, lag_c)
        if "k5" in (lag_b, lag_c) and lags != "k5":
            ap.error("--lag and --lag2 are both k5 or both integers")
        with Device(args.device) as dev:
            with dev.capture(args.input) as cap, dev.capture(args.spatial) as aux_b, dev.capture(args.spatial2) as aux_c:
                res = clean_spatial2(dev, cap, aux_b, aux_c, nfft=args.nfft, frames_per_row=args.frames_per_row, p_fa=args.p_fa,
                                     lags=lags, fs=args.fs)
                _write(res.capture, args.output)
        print(f"{args.output}: {res.records.size} frames of {args.nfft} points, aligned by {res.scan.lag} and {res.scan_c.lag}, "
              + (f"{len(res.bands)} band(s) cancelled with two auxiliaries" if res.cancelled else res.note))
        _print_bands(res)
        return 0
    if args.spatial:
        lag = "k5" if args.lag == "k5" else int(args.lag)
        with Device(args.device) as dev:
            with dev.capture(args.input) as cap, dev.capture(args.spatial) as aux:
                res = clean_spatial(dev, cap, aux, nfft=args.nfft, frames_per_row=args.frames_per_row, p_fa=args.p_fa, lag=lag,
                                    fs=args.fs)
                _write(res.capture, args.output)
        print(f"{args.output}: {res.records.size} frames of {args.nfft} points, aligned by {res.scan.lag}, "
              + (f"{len(res.bands)} band(s) cancelled" if res.cancelled else res.note))
        _print_bands(res)
        return 0
    if args.pulsed:
        rise_db = 6.0 if args.rise_db is None else args.rise_db
        with Device(args.device) as dev:
            with dev.capture(args.input) as cap:
                res = clean_pulsed(dev, cap, window=args.window, guard=args.guard, rise_db=rise_db)
                _write(res.capture, args.output)
        print(f"{args.output}: window {args.window}, guard {args.guard}, threshold {res.threshold:.4g} LSB^2 with the floor from the "
              f"{res.floor_from}, {100.0 * res.blanked_share:.2f} % of the samples blanked on {int(res.records['n_rising'].sum())} "
              f"rising edges, {100.0 * res.removed_share:.2f} % of the power removed")
        return 0
    if args.rise_db is None:
        args.rise_db = 12.0
    with Device(args.device) as dev:
        with dev.capture(args.input) as cap:
            res = (clean_swept if args.swept else clean)(dev, cap, nfft=args.nfft, rise_db=args.rise_db, fs=args.fs)
            _write(res.capture, args.output)
    print(f"{args.output}: {res.records.size} frames of {args.nfft} points, floor from the {res.floor_from}, "
          f"{100.0 * res.removed_share:.2f} % of the power removed")
    if args.swept:
        print(f"chirp domain: {int(np.count_nonzero(res.rates))} frames de-chirped around {res.sweep_hz_per_s:.4g} Hz/s"
              if res.swept else "chirp domain: no fast sweep found, excised as plain frames")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
