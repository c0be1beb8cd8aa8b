"""What is transmitting: the kind of interferer and its parameters, from the short-time spectral ridge.

The detector says THAT a capture is jammed (K1, K4), how strongly (K3) and from where (K5); this module says WHAT the
interferer is.  The reference's simulator makes four kinds (simulate/frontend/jammers/): a continuous tone
(cwJammer.py), a saw-tooth chirp (chirpJammer.py), a carrier gated by a square wave (pulsedJammer.py) and wide-band
noise (broadbandJammer.py).  ``classify`` tells them apart from the records of ``Device.ridge`` alone -- pure numpy,
no GPU call; ``characterise`` joins it to the onset detector.  ``classify_swept`` reads the chirp-rate search
(``Device.chirp``) the same way, for sweeps that cross many bins inside one frame and read as "broadband" on the ridge;
``characterise_swept`` runs that search only where ``characterise`` leaves the question open.

Every threshold below follows from the window and the frame length, not from any particular input:

* a frame of complex Gaussian noise under the periodic Hann window has total power with relative standard deviation
  sqrt(sum w^4) / sum w^2 = sqrt(35/18) / sqrt(N)  (``total_rel_sigma``);
* its largest bin holds about (ln(N / 1.5) + 0.58) / N of the total: the maximum of N exponentials of which the
  window, 1.5 bins wide, leaves N / 1.5 independent  (``noise_concentration``; (ln N + 0.58) * 1.5 / N bounds it
  from above);
* a Hann-windowed tone holds between 0.48 (half a bin off) and 2/3 (on a bin) of its own power in the peak bin; in
  noise that share is multiplied by S / (S + N).
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np

KINDS = ("none", "cw", "chirp", "pulsed", "broadband")
TONE_SHARE_MIN, TONE_SHARE_MAX = 0.48, 2.0 / 3.0
SIGMAS = 6.0                 # how many standard deviations count as "not noise"
FLOOR_PERCENTILE = 10.0      # the floor without quiet frames: this percentile of `total`, corrected to the mean


class Interference(NamedTuple):
    """``kind``: one of KINDS.  ``jnr_db``: what the frames that are on hold above the noise floor, over the floor:
    10 log10(J / N) (None for "none").  ``freq_hz``: "cw" and a "pulsed" carrier.  ``sweep_hz_per_s``: "chirp".  ``prf_hz`` and
    ``duty``: "pulsed".  Parameters that do not apply are None.  ``evidence``: the features the decision used."""
    kind: str
    jnr_db: Optional[float]
    freq_hz: Optional[float]
    sweep_hz_per_s: Optional[float]
    prf_hz: Optional[float]
    duty: Optional[float]
    evidence: dict


def total_rel_sigma(nfft: int) -> float:
    return float(np.sqrt(35.0 / 18.0 / nfft))


def noise_concentration(nfft: int) -> float:
    return float((np.log(nfft / 1.5) + 0.58) / nfft)


def _wrap(d, n):
    """Circular bin difference in [-n/2, n/2)."""
    return (np.asarray(d, np.int64) + n // 2) % n - n // 2


def _period(on: np.ndarray):
    """(lag, strength) of the on/off sequence's periodicity: the first lag behind the main lobe whose normalised
    autocorrelation comes within 10 % of the largest one there -- the fundamental rather than one of its multiples."""
    x = on.astype(np.float64) - on.mean()
    n = x.size
    if n < 8 or not np.any(x):
        return 0, 0.0
    m = 1 << int(np.ceil(np.log2(2 * n)))
    f = np.fft.rfft(x, m)
    ac = np.fft.irfft(f * np.conj(f), m)[:n // 2]
    ac = ac / (np.arange(n, n - ac.size, -1) * x.var())            # unbiased, 1 at lag 0
    below = np.nonzero(ac < 0.0)[0]
    if below.size == 0 or below[0] + 1 >= ac.size:
        return 0, 0.0
    tail = ac[below[0]:]
    best = float(tail.max())
    if best <= 0.0:
        return 0, 0.0
    lag = int(below[0] + np.nonzero(tail >= 0.9 * best)[0][0])
    # the top of that peak, not its first shoulder
    while lag + 1 < ac.size and ac[lag + 1] > ac[lag]:
        lag += 1
    return lag, float(ac[lag])


def _sweep_bins_per_frame(bins: np.ndarray, nfft: int):
    """(slope in bins per frame, share of frame steps that follow it): a robust slope of the unwrapped differences.
    The coarse slope is the median circular difference over a span long enough to move several bins (single steps
    are mostly 0 or 1 bin).  Single steps that disagree with it -- a saw-tooth's fly-back, a frame whose peak is
    noise -- cut the track into runs; every run is unwrapped by summing its steps and fitted with a least-squares
    line, and the runs' slopes are averaged by the inverse of their variances (length cubed).  A line fit averages
    the bin quantisation away, which end-point differences would keep."""
    n = bins.size
    if n < 16:
        return 0.0, 0.0
    span = max(4, min(64, n // 8))
    coarse = float(np.median(_wrap(bins[span:] - bins[:-span], nfft))) / span
    d1 = _wrap(bins[1:] - bins[:-1], nfft)
    ok = np.abs(d1 - coarse) <= 2.0 + abs(coarse)
    if not ok.any():
        return coarse, 0.0
    num = den = 0.0
    cuts = np.concatenate(([-1], np.nonzero(~ok)[0], [n - 1]))          # run r: frames cuts[r]+1 .. cuts[r+1]
    for a, b in zip(cuts[:-1] + 1, cuts[1:]):
        m = int(b - a + 1)
        if m < 8:
            continue
        y = np.concatenate(([0.0], np.cumsum(d1[a:b])))
        t = np.arange(m) - 0.5 * (m - 1)
        num += float(np.dot(t, y))
        den += float(np.dot(t, t))                                      # ~ m^3 / 12: the run's weight
    if den == 0.0:
        return float(d1[ok].mean()), float(ok.mean())
    return num / den, float(ok.mean())


def classify(ridge, fs: float, hop: int, nfft: int, noise=None) -> Interference:
    """Kind and parameters of the interferer in ``ridge`` (a ``gpsjam.Ridge``, or anything with ``records``) computed
    at ``nfft`` points every ``hop`` samples of a capture sampled at ``fs``.  ``noise``: a Ridge of frames known to be
    quiet; without it the floor is a low percentile of ``total``."""
    rec = np.asarray(getattr(ridge, "records", ridge))
    total = rec["total"].astype(np.float64)
    peak = rec["peak"].astype(np.float64)
    second = rec["second"].astype(np.float64)
    bins = rec["peak_bin"].astype(np.int64)
    n = total.size
    sig = total_rel_sigma(nfft)
    ev = {"frames": int(n), "nfft": int(nfft), "hop": int(hop), "total_rel_sigma": sig}
    nothing = Interference("none", None, None, None, None, None, ev)
    if n == 0:
        return nothing
    overlap = min(1.0, hop / float(nfft))                            # overlapping frames are not independent
    nrec = None if noise is None else np.asarray(getattr(noise, "records", noise))
    if nrec is not None and nrec.size >= 8:
        floor = float(nrec["total"].astype(np.float64).mean())
        floor_sigma = sig / np.sqrt(max(1.0, nrec.size * overlap))
        ev["floor_from"] = "noise frames"
    else:
        # the 10th percentile of Gaussian-like totals lies 1.2816 sigma under their mean
        floor = float(np.percentile(total, FLOOR_PERCENTILE)) / max(0.1, 1.0 - 1.2816 * sig)
        floor_sigma = sig / 2.0
        ev["floor_from"] = "percentile"
    if not floor > 0.0:
        return nothing
    ev["floor"] = floor
    excess = float(total.mean()) / floor - 1.0
    loud = total > floor * (1.0 + SIGMAS * sig)
    ev["excess"], ev["loud_fraction"] = excess, float(loud.mean())
    significant = excess > SIGMAS * np.hypot(floor_sigma, sig / np.sqrt(max(1.0, n * overlap))) or loud.mean() >= 0.02
    if not significant:
        return nothing

    # frames that are on: above half way between the floor and the level of the loud frames, so that a frame the
    # gate cuts in two counts by the larger half and the fraction is the duty cycle
    level = float(np.percentile(total[loud], 75.0)) if loud.any() else float(total.max())
    on = total > 0.5 * (floor + level)
    if not on.any():
        return nothing
    frac = float(on.mean())
    on_total = total[on]
    jnr_db = float(10.0 * np.log10(max(on_total.mean() - floor, 1e-300) / floor))
    ev["on_level"], ev["on_fraction"] = level, frac

    # concentration of the frames that are on, against what a tone at their S / (S + N) must hold
    share = np.clip((on_total - floor) / on_total, 0.0, 1.0)
    conc = float(np.median(peak[on] / on_total))
    line_min = TONE_SHARE_MIN * float(np.median(share))
    ev["concentration"], ev["line_min"], ev["noise_concentration"] = conc, line_min, noise_concentration(nfft)
    # half the least a tone holds (a sweep inside the frame spreads it over neighbouring bins), and clear of noise
    line = conc > max(0.5 * line_min, 2.0 * noise_concentration(nfft))
    ev["second_over_peak"] = float(np.median(second[on] / np.maximum(peak[on], 1e-300)))
    ev["lines"] = "one" if ev["second_over_peak"] < 0.25 else "several"

    on_bins = bins[on]
    mode = int(np.bincount(on_bins % nfft, minlength=nfft).argmax())
    at_mode = float((np.abs(_wrap(on_bins - mode, nfft)) <= 1).mean())
    mode_hz = float((mode - nfft if mode >= nfft // 2 else mode) * fs / nfft)
    ev["modal_bin"], ev["modal_fraction"] = mode, at_mode

    lag, strength = _period(on)
    ev["period_frames"], ev["period_strength"] = lag, strength
    if 0.05 < frac < 0.95 and lag >= 2 and strength >= 0.5:
        return Interference("pulsed", jnr_db, mode_hz if line and at_mode >= 0.8 else None, None, fs / (hop * lag), frac, ev)
    if not line:
        return Interference("broadband", jnr_db, None, None, None, None, ev)
    if at_mode >= 0.8:
        return Interference("cw", jnr_db, mode_hz, None, None, None, ev)
    # consecutive on-frames only: a gap would count as one step
    steps = np.nonzero(on[1:] & on[:-1])[0]
    track = bins if steps.size == n - 1 else on_bins
    slope, follow = _sweep_bins_per_frame(track, nfft)
    ev["sweep_bins_per_frame"], ev["sweep_follow"] = slope, follow
    sweep = slope * (fs / nfft) / (hop / fs) if follow >= 0.5 else None
    return Interference("chirp", jnr_db, None, sweep, None, None, ev)


def characterise(dev, capture, fs: float = 2.048e6, nfft: int = 256, **onset_args) -> Interference:
    """``classify`` joined to the detector: K4 (``dev.onset``) finds where the interference starts, the frames that end
    before the onset are the noise, the frames from the onset on are classified.  With no onset the whole capture is
    classified against the percentile floor.  ``capture``: a resident ``Capture`` or host bytes."""
    hop = nfft // 2
    onset = dev.onset(capture, **onset_args)
    ridge = dev.ridge(capture, nfft=nfft, hop=hop)
    k = int(onset.start_index)
    if k < 0:
        res = classify(ridge, fs, hop, nfft)
        res.evidence["onset"] = -1
        return res
    quiet = (k - nfft) // hop + 1 if k >= nfft else 0              # frames with s_f + nfft <= k
    first = -(-k // hop)                                           # first frame with s_f >= k
    res = classify(ridge[first:], fs, hop, nfft, noise=ridge[:quiet] if quiet >= 8 else None)
    res.evidence["onset"], res.evidence["first_frame"], res.evidence["quiet_frames"] = k, first, quiet
    return res


def search_noise_concentration(nfft: int, n_rates: int) -> float:
    """``noise_concentration`` for the best of n_rates de-chirped spectra: the maximum of n_rates times as many cells."""
    return float((np.log(nfft * max(1, int(n_rates)) / 1.5) + 0.58) / nfft)


def classify_swept(scan, fs: float, noise=None) -> Interference:
    """Kind and parameters of the interferer in ``scan`` (a ``gpsjam.ChirpScan``): ``classify``'s floor, on-frame and line
    tests applied to the concentration BEHIND the best de-chirp.  ``noise``: a ChirpScan or Ridge of quiet frames (a
    frame's total does not depend on the rate).

    * "chirp" with ``sweep_hz_per_s`` when the de-chirped concentration passes the line test and the modal rate of the
      frames that are on is not 0.  The sweep is the MEDIAN q of those frames times fs^2 / nfft^2: the frames that hold a
      saw-tooth's fly-back do not concentrate at any rate and are out-voted.  Its resolution, one step of the rate grid,
      is ``evidence["rate_resolution_hz_per_s"]``.
    * at modal rate 0 the records are the ridge's own and the answer is ``classify``'s: "cw" for a steady tone.
    * "pulsed", "none" and, without a line, "broadband" as ``classify``.

    The one threshold that differs is the noise term of the line test: the best of n rates is the maximum of n times as
    many noise cells, so ``search_noise_concentration`` takes the place of ``noise_concentration``."""
    nfft, hop = int(scan.nfft), int(scan.hop)
    first, step, n_rates = scan.rates
    rec = np.asarray(scan.records)
    base = classify(rec, fs, hop, nfft, noise=noise)
    ev = base.evidence
    unit = (float(fs) / nfft) ** 2
    ev["rates"], ev["rate_resolution_hz_per_s"] = (int(first), int(step), int(n_rates)), unit * step
    if base.kind in ("none", "pulsed") or "on_level" not in ev:
        return base
    total = rec["total"].astype(np.float64)
    on = total > 0.5 * (ev["floor"] + ev["on_level"])                  # classify's frames that are on
    noise_conc = search_noise_concentration(nfft, n_rates)
    line = ev["concentration"] > max(0.5 * ev["line_min"], 2.0 * noise_conc)
    ev["search_noise_concentration"], ev["dechirped_line"] = noise_conc, bool(line)
    if not line:
        return Interference("broadband", base.jnr_db, None, None, None, None, ev)
    q = np.asarray(scan.rate)[on]
    values, counts = np.unique(q, return_counts=True)
    mode = int(values[counts.argmax()])
    ev["modal_rate"], ev["modal_rate_fraction"] = mode, float((np.abs(q - mode) <= step).mean())
    if mode == 0:
        return base
    ev["median_rate"] = float(np.median(q))
    return Interference("chirp", base.jnr_db, None, ev["median_rate"] * unit, None, None, ev)


def _scan_rates(dev, capture, nfft: int, hop: int, qmax: int):
    """``Device.chirp`` over the rates -qmax .. qmax at step 1, in batches of at most 256 rates, joined into one
    ChirpScan: per frame the batch with the largest peak, the smaller rate among equals."""
    from . import ChirpScan, _ffi
    best = None
    for lo in range(-qmax, qmax + 1, _ffi.GJ_CHIRP_MAX_RATES):
        n = min(_ffi.GJ_CHIRP_MAX_RATES, qmax + 1 - lo)
        part = dev.chirp(capture, nfft=nfft, hop=hop, rates=(lo, 1, n))
        rec = part.records.copy()
        rec["rate_index"] += lo + qmax
        if best is None:
            best, scan = rec, part
        else:
            better = rec["peak"] > best["peak"]
            best[better] = rec[better]
    return ChirpScan(best, nfft, hop, (-qmax, 1, 2 * qmax + 1), scan.first_sample, scan.guard)


def characterise_swept(dev, capture, fs: float = 2.048e6, nfft: int = 256, max_sweep_hz_per_s: float = 4.096e9,
                       **onset_args) -> Interference:
    """``characterise``, and where its answer leaves a fast sweep possible -- "broadband", or a "chirp" whose track less
    than half of the frame steps follow -- the chirp-rate search over the symmetric range of integer rates that covers
    ``max_sweep_hz_per_s`` (at most nfft^2 / 2 units of fs^2 / nfft^2), classified by ``classify_swept`` on the same
    frames against the same quiet frames.  Returns the better-founded answer with both evidences: the search's "chirp"
    with ``evidence["ridge"]`` = the ridge's evidence, otherwise ``characterise``'s own with ``evidence["swept"]``."""
    res = characterise(dev, capture, fs=fs, nfft=nfft, **onset_args)
    if not (res.kind == "broadband" or (res.kind == "chirp" and res.evidence.get("sweep_follow", 0.0) < 0.5)):
        return res
    hop = nfft // 2
    unit = (float(fs) / nfft) ** 2
    qmax = max(1, min(nfft * nfft // 2, int(np.ceil(abs(max_sweep_hz_per_s) / unit))))
    scan = _scan_rates(dev, capture, nfft, hop, qmax)
    if res.evidence.get("onset", -1) < 0:
        swept = classify_swept(scan, fs)
    else:
        first, quiet = res.evidence["first_frame"], res.evidence["quiet_frames"]
        swept = classify_swept(scan[first:], fs, noise=scan[:quiet] if quiet >= 8 else None)
    if swept.kind == "chirp" and swept.evidence.get("modal_rate", 0) != 0:
        swept.evidence["ridge"] = res.evidence
        for key in ("onset", "first_frame", "quiet_frames"):
            if key in res.evidence:
                swept.evidence[key] = res.evidence[key]
        return swept
    res.evidence["swept"] = swept.evidence
    return res
