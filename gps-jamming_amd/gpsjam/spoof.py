"""Two-antenna spoofing detection: the carrier phase difference of every PRN between two antennas on one clock.

Authentic satellites arrive from different directions: the phase of a PRN at antenna b against antenna a,
2 pi (baseline . direction) / wavelength, differs from PRN to PRN.  A spoofer sends every PRN from ONE antenna: all
its PRNs share one phase difference.  ``pair_phases`` measures the difference per PRN from the correlator bank's prompt
series (``gpsjam.postcorr``), ``common_direction`` finds the largest set of PRNs inside one arc and the probability of
such a set under uniform phases, and ``scan`` puts the two together.

The premise is ``coherence.scan``'s: the two receivers share a clock and the captures are sample-aligned (the
deployment ``gpsjam.local`` holds).

Limits.  One baseline measures one angle: it cannot separate a spoofer from satellites that happen to share its phase
cone, and ``p_chance`` is the price list for that.  Fewer than ``min_common`` (4) acquired PRNs give no verdict
(``spoofed`` is None).  A spoofer that overpowers the authentic signals is what the acquisition finds: ``scan`` sees one
peak per PRN, the counterfeit one, and loses a PRN whose two copies share a Doppler bin (the weaker one is the peak
test's second power).  ``scan_peaks`` takes its candidates from the K-peak search instead (``gnss.AcqSearch.peaks``, up to
``k`` per PRN), and names, next to the counterfeit signals in the common arc, the authentic ones outside it.  Two
signals of one PRN closer than the guard (2 samples per chip either side) are one peak to it.

``remove`` takes the counterfeit candidates out of a capture -- replicas rebuilt from the bank's prompts and subtracted
(``Device.subtract``, gj_subtract_dev) -- so that a receiver can go back to the authentic ones;
``gpsjam.mitigate.clean_spoofed`` does it for both antennas.  ``remove`` is open loop and good for a tenth of a second;
``remove_tracked`` follows every candidate with the tracking loops (``gpsjam.track``) and takes it out of the whole
capture with the NCOs the loops had, epoch by epoch (``Device.subtract_tracked``, gj_subtract_track_dev).

    python -m gpsjam.spoof A.bin B.bin [--peaks K]
"""
from __future__ import annotations

import math
from typing import List, NamedTuple, Optional, Sequence

import numpy as np

from . import gnss, postcorr


class PairPhase(NamedTuple):
    prn: int
    phase: float         # arg sum_k P_b[k] conj(P_a[k]), rad: antenna b against antenna a
    coherence: float     # |sum| / sqrt(sum |P_a|^2 sum |P_b|^2), 0 .. 1
    cn0_dbhz: float      # at antenna a
    doppler_hz: float


class Common(NamedTuple):
    members: List[int]   # indices into the phases given, in their order
    centre: float        # middle of the arc that holds them, rad
    p_chance: float      # bound on the probability of a set this large under uniform phases


class SpoofReport(NamedTuple):
    prns: List[int]
    phase: np.ndarray
    coherence: np.ndarray
    cn0: np.ndarray
    common_prns: List[int]
    p_chance: float
    spoofed: Optional[bool]      # None: fewer than min_common PRNs, no verdict


def pair_phases(dev, a, b, search, first_sample: int = 0, duration_s: float = 0.1, results=None) -> List[PairPhase]:
    """Acquire on ``a`` (``postcorr.observe``: the channels at the refined Doppler) and run the SAME channels on ``b``.
    z_p = sum_k P_b[k] conj(P_a[k]): navigation bits and whatever Doppler is left are common to both antennas and
    cancel, block by block.  Per acquired PRN ``phase = arg z_p`` and
    ``coherence = |z_p| / sqrt(sum |P_a|^2 sum |P_b|^2)``.  ``results``: as in ``postcorr.observe``."""
    with dev._resident(a) as cap_a, dev._resident(b) as cap_b:
        obs = postcorr.observe(dev, cap_a, search, first_sample, duration_s, results)
        if not obs:
            return []
        B = postcorr.block_samples(search)
        n = min(int(round(duration_s * search.fs)), cap_a.nsamples - int(first_sample), cap_b.nsamples - int(first_sample))
        bank = dev.corr_bank(cap_b, [o.channel for o in obs], postcorr.codes([o.prn for o in obs]), first_sample, n, B, (0,))
    out = []
    for o, pb in zip(obs, postcorr.tap_periods(bank, 0, [o.first_block for o in obs])):
        m = min(o.prompts.size, pb.size)
        pa, pb = o.prompts[:m], pb[:m]
        z = np.sum(pb * np.conj(pa))
        den = math.sqrt(float(np.sum(np.abs(pa) ** 2)) * float(np.sum(np.abs(pb) ** 2)))
        out.append(PairPhase(o.prn, float(np.angle(z)), float(abs(z) / den) if den > 0.0 else 0.0, o.cn0_dbhz, o.doppler_hz))
    return out


def chance(k: int, n: int, tol: float) -> float:
    """A bound on the probability that SOME arc of width 2 tol holds at least k of n independent uniform phases.

    Take the member of such a set that comes first going round anticlockwise: the others lie in the arc of width 2 tol that starts
    at it.  So the event is the union over the n phases i of A_i = "at least k - 1 of the other n - 1 phases lie in
    [phi_i, phi_i + 2 tol]".  Given phi_i, each of the others lies there with probability w = 2 tol / (2 pi) = tol / pi,
    independently, so P(A_i) = P(Binomial(n - 1, w) >= k - 1), and by the union bound

        P <= n sum_{m = k-1}^{n-1} C(n - 1, m) w^m (1 - w)^(n - 1 - m).

    For k = n and w < 1/2 the A_i exclude each other and the bound is the exact n (tol / pi)^(n - 1)."""
    k, n = int(k), int(n)
    if n < 1 or k < 2:
        return 1.0
    w = min(max(float(tol) / math.pi, 0.0), 1.0)
    tail = sum(math.comb(n - 1, m) * w ** m * (1.0 - w) ** (n - 1 - m) for m in range(k - 1, n))
    return min(1.0, n * tail)


def common_direction(phases: Sequence[float], tol: float = 0.15) -> Common:
    """The largest set of phases that lie within one arc of width 2 tol (rad), and ``chance`` of a set of its size
    among as many phases.  Every phase in turn is taken as the arc's start; of equally large sets the narrowest wins."""
    ph = np.asarray(phases, np.float64).reshape(-1)
    n = int(ph.size)
    if n == 0:
        return Common([], 0.0, 1.0)
    best, best_span = [], 0.0
    for i in range(n):
        ahead = (ph - ph[i]) % (2.0 * math.pi)
        inside = np.nonzero(ahead <= 2.0 * float(tol))[0]
        span = float(ahead[inside].max())
        if len(inside) > len(best) or (len(inside) == len(best) and span < best_span):
            best, best_span, start = inside.tolist(), span, float(ph[i])
    centre = (start + 0.5 * best_span + math.pi) % (2.0 * math.pi) - math.pi
    return Common(best, centre, chance(len(best), n, tol))


def scan(dev, a, b, search=None, tol: float = 0.15, min_common: int = 4, first_sample: int = 0,
         duration_s: float = 0.1) -> SpoofReport:
    """``pair_phases`` and ``common_direction``: ``spoofed`` when at least ``min_common`` PRNs share one arc, None when
    fewer than that were acquired at all.  ``search``: a ``gnss.AcqSearch`` of the caller's (default: one over all 32
    PRNs, closed again)."""
    own = search is None
    if own:
        search = gnss.AcqSearch(dev)
    try:
        found = pair_phases(dev, a, b, search, first_sample, duration_s)
    finally:
        if own:
            search.close()
    prns = [f.prn for f in found]
    common = common_direction([f.phase for f in found], tol)
    verdict = None if len(prns) < int(min_common) else len(common.members) >= int(min_common)
    return SpoofReport(prns, np.array([f.phase for f in found]), np.array([f.coherence for f in found]),
                       np.array([f.cn0_dbhz for f in found]), [prns[i] for i in common.members], common.p_chance, verdict)


class PeakCandidate(NamedTuple):
    """One significant peak of the K-peak search, measured on both antennas."""
    prn: int
    code_index: int      # the peak's: samples after ``first_sample`` at which the code starts
    doppler_hz: float    # the bin's Doppler plus the residual
    cn0_dbhz: float      # at antenna a
    phase: float         # antenna b against antenna a, rad
    coherence: float
    ratio: float         # the peak's power over the surface's floor


class PeakSpoofReport(NamedTuple):
    candidates: List[PeakCandidate]
    common: List[int]                    # indices into ``candidates`` of the largest set within one arc
    common_prns: List[int]               # their PRNs, each once
    p_chance: float
    spoofed: Optional[bool]              # None: fewer than min_common distinct PRNs, no verdict
    counterfeit: List[PeakCandidate]     # when spoofed: the candidates in the arc
    authentic: List[PeakCandidate]       # when spoofed: the candidates outside it of PRNs that have one inside


BANK_CHANNELS = 64                       # GJ_CORR_MAX_CHANNELS: candidates per bank


def pair_phases_peaks(dev, a, b, search, k: int = 2, pfa: float = 1e-3, first_sample: int = 0,
                      duration_s: float = 0.1) -> List[PeakCandidate]:
    """``pair_phases`` on the candidates of ``search.peaks(a, first_sample, k, pfa=pfa)``: every significant peak is a
    channel of its own, at its code index and its bin's Doppler, so a PRN that is in the air twice stands twice.  The
    candidates go through ``postcorr.observe`` and the same channels on ``b`` in slices of at most BANK_CHANNELS; phase
    and coherence are ``pair_phases``'s.  In the search's PRN order, a PRN's peaks largest first."""
    with dev._resident(a) as cap_a, dev._resident(b) as cap_b:
        found = [(p.prn, pk) for p in search.peaks(cap_a, first_sample, k, pfa=pfa) for pk in p.peaks if pk.significant]
        out = []
        for at in range(0, len(found), BANK_CHANNELS):
            part = found[at:at + BANK_CHANNELS]
            results = [gnss.AcqResult(prn, True, pk.ratio, 0.0, pk.code_index, pk.freq_index, pk.doppler_hz, 0, pk.power, 0.0, 0.0)
                       for prn, pk in part]
            for (prn, pk), f in zip(part, pair_phases(dev, cap_a, cap_b, search, first_sample, duration_s, results)):
                out.append(PeakCandidate(prn, pk.code_index, f.doppler_hz, f.cn0_dbhz, f.phase, f.coherence, pk.ratio))
    return out


def scan_peaks(dev, a, b, search=None, k: int = 2, tol: float = 0.15, min_common: int = 4, pfa: float = 1e-3,
               first_sample: int = 0, duration_s: float = 0.1) -> PeakSpoofReport:
    """``pair_phases_peaks`` and ``common_direction`` over ALL candidates.  A PRN counts once toward ``min_common``,
    however many of its candidates lie in the arc: ``spoofed`` is None when fewer than ``min_common`` distinct PRNs
    have a candidate at all, and otherwise whether that many distinct PRNs share the arc.  When spoofed, ``counterfeit``
    lists the candidates in the arc and ``authentic`` the candidates outside it of PRNs that also have one inside: the
    signals a receiver should go back to.  ``search``: as in ``scan``."""
    own = search is None
    if own:
        search = gnss.AcqSearch(dev)
    try:
        found = pair_phases_peaks(dev, a, b, search, k, pfa, first_sample, duration_s)
    finally:
        if own:
            search.close()
    common = common_direction([f.phase for f in found], tol)
    inside = sorted({found[i].prn for i in common.members})
    verdict = None if len({f.prn for f in found}) < int(min_common) else len(inside) >= int(min_common)
    counterfeit = [found[i] for i in common.members] if verdict else []
    members = set(common.members)
    authentic = [f for i, f in enumerate(found) if i not in members and f.prn in inside] if verdict else []
    return PeakSpoofReport(found, list(common.members), inside, common.p_chance, verdict, counterfeit, authentic)


class Removal(NamedTuple):
    """One signal taken out by ``remove``, measured by the bank on the range before and after."""
    prn: int
    code_index: int
    doppler_hz: float        # refined, what the replica was made with
    cn0_before: float        # moments C/N0 of its prompts, dB-Hz
    cn0_after: float
    suppression_db: float    # 10 log10 of the mean |prompt|^2 before over after


class Removed(NamedTuple):
    """Result of ``remove``: the cleaned range as a resident ``Capture`` of its own (the caller frees it), one ``Removal``
    per candidate, the SUB_DTYPE records of the subtraction and the ``postcorr.Observation`` of every candidate, whose
    channels the replicas were made with.  Where more than BANK_CHANNELS candidates go out in several passes, ``total``
    is the input's and ``removed`` and ``n_clipped`` are summed over the passes: every byte changed or clipped counts
    in the pass that did it."""
    capture: object
    removals: List[Removal]
    records: np.ndarray
    observations: list


def _copy_range(dev, cap, first_sample: int, n: int):
    """The range as a capture of its own and its records, through the subtraction with one channel of amplitude zero:
    byte for byte, by the definition (q = floor(d / 65536) = 0).  The library has no device-to-device copy of its own;
    ``mitigate.clean_spatial`` returns its unflagged copy the same way, through the canceller with zero weights."""
    ones = np.ones((1, gnss.CA_LEN), np.int16)
    B = 4096
    return dev.subtract(cap, [postcorr.Channel(0, 0, 0, 0, 0)], ones, np.zeros((1, -(-n // B), 2), np.int32), first_sample, n, B,
                        dither=False)


def remove(dev, capture, candidates, search, first_sample: int = 0, duration_s: float = 0.1, dither: bool = True,
           observations=None) -> Removed:
    """Successive interference cancellation of ``candidates`` (``PeakCandidate``s: ``scan_peaks(...).counterfeit``) from
    samples first_sample .. + duration_s of ``capture``, open loop: the candidates are observed again
    (``postcorr.observe(results=...)``: refined Doppler, sub-sample code phase), a one-tap bank at
    ``postcorr.block_samples`` gives each one's complex prompt per eighth of a code period, ``postcorr.amplitudes``
    turns them into one amplitude per code period, and ``Device.subtract`` rebuilds the replicas and takes them off
    the bytes (gj_subtract_dev).  A bank on the cleaned range measures what is left.  At most BANK_CHANNELS candidates
    go out per pass; more are taken in slices, each from the range the slice before it left.  ``observations``: those of
    an earlier ``remove`` on another antenna of the same clock -- the candidates are then not observed again, the SAME
    channels are used, and the amplitudes are this capture's own.  No candidate: the range comes back byte for byte.

    Limits.  One set of channels serves the whole range: 0.1 s is fine, ten seconds of a moving receiver are not
    (``remove_tracked`` is for those).  The
    replica has the mixer's 16-step carrier: what the bank sees is nulled, about 1 % of the signal's power stays behind
    as the staircase's harmonics, far from its Doppler.  Per code period one complex dimension of the noise goes out
    with the signal.  Two copies closer than the K-peak guard are one peak and are removed as one."""
    candidates = list(candidates)
    with dev._resident(capture) as cap:
        first = int(first_sample)
        n = min(int(round(duration_s * search.fs)), cap.nsamples - first)
        B, removals, seen, held, records = postcorr.block_samples(search), [], [], None, None
        period_s = postcorr.SUB_BLOCKS * B / float(search.fs)
        if not candidates:
            cleaned, records = _copy_range(dev, cap, first, n)
            return Removed(cleaned, [], records, [])
        try:
            for at in range(0, len(candidates), BANK_CHANNELS):
                part = candidates[at:at + BANK_CHANNELS]
                src = cap if held is None else held
                if observations is None:
                    results = [gnss.AcqResult(c.prn, True, c.ratio, c.cn0_dbhz, c.code_index,
                                              int(np.argmin(np.abs(np.asarray(search.freqs) - c.doppler_hz))), c.doppler_hz, 0, 0.0, 0.0, 0.0)
                               for c in part]
                    obs = postcorr.observe(dev, src, search, first, duration_s, results)
                else:
                    obs = list(observations[at:at + BANK_CHANNELS])
                chans, rows, starts = [o.channel for o in obs], postcorr.codes([o.prn for o in obs]), [o.first_block for o in obs]
                before = dev.corr_bank(src, chans, rows, first, n, B, (0,))
                cleaned, rec = dev.subtract(src, chans, rows, postcorr.amplitudes(before, starts), first, n, B, dither=dither)
                if records is None:
                    records = rec                            # ``total`` is the input's: the first pass reads it
                else:
                    records["removed"] += rec["removed"]
                    records["n_clipped"] += rec["n_clipped"]
                if held is not None:
                    held.free()
                held, first = cleaned, 0                     # the cleaned range is a capture of its own, from its sample 0
                after = dev.corr_bank(held, chans, rows, 0, n, B, (0,))
                for c, o, pb, pa in zip(part, obs, postcorr.tap_periods(before, 0, starts), postcorr.tap_periods(after, 0, starts)):
                    mb, ma = float(np.mean(np.abs(pb) ** 2)) if pb.size else 0.0, float(np.mean(np.abs(pa) ** 2)) if pa.size else 0.0
                    db = float(10.0 * np.log10(mb / ma)) if mb > 0.0 and ma > 0.0 else (float("inf") if mb > 0.0 else 0.0)
                    removals.append(Removal(o.prn, int(c.code_index), o.doppler_hz, postcorr.cn0(pb, period_s), postcorr.cn0(pa, period_s), db))
                seen.extend(obs)
        except BaseException:
            if held is not None:
                held.free()
            raise
    return Removed(held, removals, records, seen)


TRACKED_WINDOW = 100                     # epochs of one measuring window of ``remove_tracked``


def _window_prompts(dev, cap, origin: int, tracks, rows, B: int, windows):
    """Per track the prompts of one-tap banks over ``windows`` (first epochs) of TRACKED_WINDOW epochs each: a window
    starts on that track's epoch boundary, ``origin`` + start + m B of ``cap``, and holds the channel of that epoch's
    record for its length."""
    out = []
    for k, t in enumerate(tracks):
        parts = []
        for m in windows:
            r = t.records[m]
            ch = postcorr.Channel(int(r["code_phase"]), int(r["code_step"]), int(r["carr_phase"]), int(r["carr_step"]), k)
            count = min(TRACKED_WINDOW, t.records.size - m)
            parts.append(dev.corr_bank(cap, [ch], rows, origin + t.start + m * B, count * B, B, (0,)).tap(0)[0])
        out.append(np.concatenate(parts))
    return out


def remove_tracked(dev, capture, candidates, search, first_sample: int = 0, pull_in: int = 200, dither: bool = True) -> Removed:
    """``remove`` over a whole capture, closed loop: ``track.follow(results=...)`` runs its DLL / FLL / PLL on every
    candidate from ``first_sample`` to the end of ``capture`` (``pull_in`` epochs with the wide loops),
    ``track.amplitudes`` makes one amplitude per epoch from each epoch's own prompt, and ``Device.subtract_tracked``
    (gj_subtract_track_dev) rebuilds every replica with the NCOs its loop had in that epoch and takes it off the bytes.
    At most BANK_CHANNELS candidates go out per pass, as in ``remove``.  A ``Removal`` per candidate: C/N0 and
    suppression from one-tap banks before and after, on windows of TRACKED_WINDOW epochs, one per second of capture,
    each at the channel of its first epoch's record; ``doppler_hz`` is the loop's mean.  ``Removed.observations`` holds
    the ``track.Track`` of every candidate.  No candidate: the range comes back byte for byte.

    Limits.  Samples in front of a channel's ``start`` (the candidate's code index) and behind its last whole epoch keep
    that channel's signal.  An epoch with a navigation bit flip inside it has a small prompt and is under-subtracted.
    One amplitude per epoch takes one complex dimension of the noise per epoch out with the signal.  While the loops
    pull in, the replica is as good as the loops are.  The staircase carrier and the K-peak guard: as in ``remove``."""
    from . import track
    candidates = list(candidates)
    with dev._resident(capture) as cap:
        first = int(first_sample)
        n = cap.nsamples - first
        if not candidates:
            cleaned, records = _copy_range(dev, cap, first, n)
            return Removed(cleaned, [], records, [])
        removals, seen, held, records = [], [], None, None
        try:
            for at in range(0, len(candidates), BANK_CHANNELS):
                part = candidates[at:at + BANK_CHANNELS]
                src = cap if held is None else held
                results = [gnss.AcqResult(c.prn, True, c.ratio, c.cn0_dbhz, c.code_index,
                                          int(np.argmin(np.abs(np.asarray(search.freqs) - c.doppler_hz))), c.doppler_hz, 0, 0.0, 0.0, 0.0)
                           for c in part]
                tracks = track.follow(dev, src, search, first, pull_in, results=results)
                if len(tracks) != len(part):
                    raise ValueError("the capture holds no whole epoch behind the candidates' code indices")
                B = int(round(tracks[0].block_s * search.fs))
                rows = postcorr.codes([t.prn for t in tracks])
                rec_in = np.stack([t.records for t in tracks])
                E = rec_in.shape[1]
                stride = max(TRACKED_WINDOW, int(round(search.fs / B)))
                windows = [m for m in range(0, E, stride) if m + TRACKED_WINDOW <= E] or [0]
                before = _window_prompts(dev, src, first, tracks, rows, B, windows)
                cleaned, rec = dev.subtract_tracked(src, [(t.start, k) for k, t in enumerate(tracks)], rows, rec_in,
                                                    track.amplitudes(rec_in, B), first, n, B, dither=dither)
                if records is None:
                    records = rec                            # ``total`` is the input's: the first pass reads it
                else:
                    records["removed"] += rec["removed"]
                    records["n_clipped"] += rec["n_clipped"]
                if held is not None:
                    held.free()
                held, first = cleaned, 0                     # the cleaned range is a capture of its own, from its sample 0
                after = _window_prompts(dev, held, 0, tracks, rows, B, windows)
                for c, t, pb, pa in zip(part, tracks, before, after):
                    mb, ma = float(np.mean(np.abs(pb) ** 2)), float(np.mean(np.abs(pa) ** 2))
                    db = float(10.0 * np.log10(mb / ma)) if mb > 0.0 and ma > 0.0 else (float("inf") if mb > 0.0 else 0.0)
                    removals.append(Removal(t.prn, int(c.code_index), float(t.doppler_hz.mean()), postcorr.cn0(pb, t.block_s),
                                            postcorr.cn0(pa, t.block_s), db))
                seen.extend(tracks)
        except BaseException:
            if held is not None:
                held.free()
            raise
    return Removed(held, removals, records, seen)


def _print_removals(title, rows):
    print(f"{title}: {len(rows)}")
    for r in rows:
        print(f"  PRN {r.prn:2d}  code {r.code_index:5d}  Doppler {r.doppler_hz:+9.1f} Hz  C/N0 {r.cn0_before:5.1f} -> {r.cn0_after:5.1f} dB-Hz  "
              f"suppression {r.suppression_db:5.1f} dB")


def _print_candidates(title, rows):
    print(f"{title}: {len(rows)}")
    for c in rows:
        print(f"  PRN {c.prn:2d}  code {c.code_index:5d}  Doppler {c.doppler_hz:+9.1f} Hz  C/N0 {c.cn0_dbhz:5.1f} dB-Hz  "
              f"phase {c.phase:+7.3f} rad  coherence {c.coherence:5.3f}  peak/floor {c.ratio:6.1f}")


def main(argv=None) -> int:
    import argparse
    from . import Device
    ap = argparse.ArgumentParser(prog="python -m gpsjam.spoof", description="print each PRN's phase between two antennas and the spoofing verdict")
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--tol", type=float, default=0.15, help="half width of the common arc, rad")
    ap.add_argument("--min-common", type=int, default=4)
    ap.add_argument("--first-sample", type=int, default=0)
    ap.add_argument("--duration", type=float, default=0.1, help="seconds")
    ap.add_argument("--fs", type=float, default=2.048e6)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--peaks", type=int, default=0, metavar="K",
                    help="search K peaks per PRN and list counterfeit and authentic signals of the same PRN apart")
    ap.add_argument("--pfa", type=float, default=1e-3, help="with --peaks: false-alarm bound per PRN of a significant peak")
    args = ap.parse_args(argv)
    with Device(args.device) as dev:
        search = gnss.AcqSearch(dev, fs=args.fs)
        try:
            with dev.capture(args.a) as cap_a, dev.capture(args.b) as cap_b:
                if args.peaks:
                    rep = scan_peaks(dev, cap_a, cap_b, search, args.peaks, args.tol, args.min_common, args.pfa,
                                     args.first_sample, args.duration)
                else:
                    rep = scan(dev, cap_a, cap_b, search, args.tol, args.min_common, args.first_sample, args.duration)
        finally:
            search.close()
    if args.peaks:
        _print_candidates(f"{args.a} / {args.b}: significant peaks on the first antenna (up to {args.peaks} per PRN)", rep.candidates)
        verdict = "no verdict (too few PRNs)" if rep.spoofed is None else ("SPOOFED" if rep.spoofed else "not flagged")
        print(f"largest common arc (+-{args.tol} rad): {len(rep.common_prns)} PRN(s) {rep.common_prns}, chance {rep.p_chance:.3g}: {verdict}")
        if rep.spoofed:
            _print_candidates("counterfeit (in the arc)", rep.counterfeit)
            _print_candidates("authentic (outside the arc, same PRNs)", rep.authentic)
        return 0
    print(f"{args.a} / {args.b}: {len(rep.prns)} PRN(s) acquired on the first antenna")
    for prn, ph, co, c in zip(rep.prns, rep.phase, rep.coherence, rep.cn0):
        mark = " *" if prn in rep.common_prns and len(rep.common_prns) >= args.min_common else ""
        print(f"  PRN {prn:2d}  phase {ph:+7.3f} rad  coherence {co:5.3f}  C/N0 {c:5.1f} dB-Hz{mark}")
    verdict = "no verdict (too few PRNs)" if rep.spoofed is None else ("SPOOFED" if rep.spoofed else "not flagged")
    print(f"largest common arc (+-{args.tol} rad): {len(rep.common_prns)} PRN(s) {rep.common_prns}, chance {rep.p_chance:.3g}: {verdict}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
