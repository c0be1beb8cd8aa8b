"""Following a satellite: closed-loop tracking of every acquired PRN over a whole capture.

Everything behind the acquisition in ``gpsjam.postcorr`` and ``gpsjam.spoof`` runs open loop: one Doppler and one code
rate per channel for the whole range, which is fine for 0.1 s and not for 10 s of a moving receiver.  The reference's
receiver spends its life in closed loops instead (sdrtracking -> correlator -> pll / dll, sdrtrk.c): each millisecond
the early, prompt and late sums steer a carrier and a code NCO.  ``Device.track`` (gj_track_dev, k_track.hip) runs that
loop for every channel in one launch, in exact integers; what is left for the host is the loop gains, the hand-over from
the acquisition and float arithmetic on the records, and lives here.  ``amplitudes`` makes of the records what
``Device.subtract_tracked`` (gj_subtract_track_dev) needs to take a followed signal out of the capture again
(``gpsjam.spoof.remove_tracked``).

Nothing here is a CPU fallback for the kernel: the records come from the library.
"""
from __future__ import annotations

import math
from typing import List, NamedTuple, Optional

import numpy as np

from . import _ffi, gnss, postcorr

WIDE = (30.0, 200.0, 5.0)      # PLL, FLL and DLL noise bandwidth in Hz while pulling in (sdrinit.c:196-201)
NARROW = (20.0, 50.0, 2.0)     # ... and once locked (sdrinit.c:202-206)
AID_L1CA = 1540                # carrier cycles per chip: the code NCO follows the carrier NCO / 1540
_PERIOD = gnss.CA_LEN << 32


def gains(pll_hz: float, fll_hz: float, dll_hz: float, block_samples: int, fs: float, spacing: int = 1,
          aid_div: int = AID_L1CA) -> "_ffi.TrackParams":
    """The integer gains of gj_track_params from the reference's loop bandwidths.  For a second-order loop of noise
    bandwidth b: w2 = (b / 0.53)^2, aw = 1.414 b / 0.53; the FLL's fllw = b / 0.25; dt = block_samples / fs
    (sdrinit.c:196-206).  The carrier discriminator is in 2^-32 cycles and carr_step in 2^-32 cycles per sample
    (GJ_TRACK_PLL_SHIFT = 32); the code discriminator is Q16 and code_step Q32.32 chips per sample
    (GJ_TRACK_DLL_SHIFT = 24)."""
    dt = float(block_samples) / float(fs)
    w2, aw = (pll_hz / 0.53) ** 2, 1.414 * pll_hz / 0.53
    w2d, awd = (dll_hz / 0.53) ** 2, 1.414 * dll_hz / 0.53
    fllw = fll_hz / 0.25
    r = lambda v: int(math.floor(v + 0.5))
    return _ffi.TrackParams(int(spacing), int(aid_div), r(2.0 * aw / fs * 2.0 ** 32), r(2.0 * w2 * dt / fs * 2.0 ** 32),
                            r(2.0 * math.pi * fllw * dt / fs * 2.0 ** 32), r(awd / fs * 2.0 ** 40), r(w2d * dt / fs * 2.0 ** 40), 0)


def states(search, results, first_sample: int = 0):
    """(prns, states): one TRACK_STATE_DTYPE record per acquired PRN of ``results`` (``search.search(capture,
    first_sample)``), code row k for the k-th of them.  ``start`` is the acquisition's ``code_index``: every channel's
    epochs begin where its code period does, so a navigation bit flips between epochs and not inside one.  The code
    phase is 0 there and the Doppler is the bin's."""
    from . import TRACK_STATE_DTYPE
    prns, rows = [], []
    for r in results:
        if not r.acquired:
            continue
        ch = postcorr.channel(len(rows), 0.0, float(r.doppler_hz), search.fs)
        rows.append((tuple(ch), 0, int(r.code_index), 0, 0, 0, (0, 0)))
        prns.append(int(r.prn))
    return prns, np.array(rows, TRACK_STATE_DTYPE).reshape(-1)


class Track(NamedTuple):
    """One PRN followed through a capture.  Series are per epoch unless they say per window."""
    prn: int
    start: int                 # sample after first_sample at which epoch 0 begins
    block_s: float             # an epoch in seconds
    doppler_hz: np.ndarray     # float64: the carrier NCO each epoch's sums were made with
    code_phase_chips: np.ndarray   # float64: the code NCO's phase at each epoch's first sample
    carrier_cycles: np.ndarray     # float64: the carrier NCO's phase there, in [0, 1)
    prompts: np.ndarray        # complex128
    bits: np.ndarray           # int8: sign(I_P), +1 where it is 0
    window: int                # epochs per window
    lock: np.ndarray           # float64 per window: sum |I_P| / sum |P| (1 in phase lock, 2 / pi without)
    cn0_dbhz: np.ndarray       # float64 per window: postcorr.cn0 of the window's prompts
    records: np.ndarray        # TRACK_EPOCH_DTYPE: everything the library wrote
    state: np.ndarray          # TRACK_STATE_DTYPE record behind the last epoch


def _series(prn: int, start: int, rec: np.ndarray, state, block_s: float, fs: float, window: int) -> Track:
    step = ((rec["carr_step"].astype(np.int64) + 2 ** 31) % 2 ** 32 - 2 ** 31).astype(np.float64)
    prompts = rec["prompt"][:, 0].astype(np.float64) + 1j * rec["prompt"][:, 1].astype(np.float64)
    edges = list(range(0, max(rec.size - window // 2, 1), window)) + [rec.size]     # a short tail joins the last window
    lock, cn0 = [], []
    for lo, hi in zip(edges, edges[1:]):
        p = prompts[lo:hi]
        total = float(np.abs(p).sum())
        lock.append(float(np.abs(p.real).sum()) / total if total > 0.0 else 0.0)
        cn0.append(postcorr.cn0(p, block_s))
    return Track(prn, start, block_s, step / 2.0 ** 32 * fs, rec["code_phase"].astype(np.float64) / 2.0 ** 32,
                 rec["carr_phase"].astype(np.float64) / 2.0 ** 32, prompts, np.where(rec["prompt"][:, 0] < 0, -1, 1).astype(np.int8),
                 window, np.array(lock), np.array(cn0), rec, state)


def follow(dev, capture, search, first_sample: int = 0, pull_in: int = 200, block_samples: Optional[int] = None,
           spacing: int = 1, window: Optional[int] = None, results=None) -> List[Track]:
    """The chain on a resident capture (or host bytes): acquisition at ``first_sample``; ``pull_in`` epochs with the
    WIDE loops; the rest of the capture with the NARROW ones from the written-back states, in launches of at most
    TRACK_MAX_EPOCHS epochs.  One ``Track`` per acquired PRN, in the search's order.  ``block_samples``: an epoch,
    default one code period down to a multiple of 16 (2048 at 2.048 MS/s); ``window``: epochs per entry of the lock and
    C/N0 series, default one second; ``results``: ``gnss.AcqResult`` records to use in place of ``search.search``."""
    from . import TRACK_MAX_CHANNELS, TRACK_MAX_EPOCHS
    B = max(16, int(search.nsamp) // 16 * 16) if block_samples is None else int(block_samples)
    block_s = B / float(search.fs)
    window = max(1, int(round(1.0 / block_s))) if window is None else max(1, int(window))
    with dev._resident(capture) as cap:
        results = search.search(cap, first_sample) if results is None else list(results)
        prns, st = states(search, results, first_sample)
        if not prns:
            return []
        if len(prns) > TRACK_MAX_CHANNELS:
            raise ValueError(f"{len(prns)} channels: one launch takes {TRACK_MAX_CHANNELS}")
        starts = st["start"].astype(np.int64)
        n = cap.nsamples - int(first_sample)
        left = (n - int(starts.max())) // B
        rows, pieces = postcorr.codes(prns), []
        schedule = [(min(int(pull_in), left), WIDE)] if pull_in > 0 else []
        schedule.append((left - (schedule[0][0] if schedule else 0), NARROW))
        for count, bands in schedule:
            params = gains(*bands, B, search.fs, spacing)
            while count > 0:
                step = min(count, TRACK_MAX_EPOCHS)
                rec, st = dev.track(cap, st, rows, params, first_sample, n, B, step)
                pieces.append(rec)
                count -= step
    if not pieces:
        return []
    rec = np.concatenate(pieces, axis=1)
    return [_series(prn, int(starts[k]), rec[k], st[k], block_s, float(search.fs), window) for k, prn in enumerate(prns)]


def amplitudes(records, block_samples: int) -> np.ndarray:
    """int32[n_channels][n_epochs][2]: the amplitudes (aI, aQ) with which ``Device.subtract_tracked`` takes out what the
    loops followed, from TRACK_EPOCH_DTYPE[n_channels][n_epochs] records (one channel's row alone counts as one channel).
    Per epoch the least-squares amplitude of the loop's own template, as ``postcorr.amplitudes`` makes it per code period:

        a = round(P / (block_samples * MIXER_GAIN) * 2^SUB_FRAC),    P the epoch's prompt

    The prompt was made with exactly the NCO the replica will be made with, so the replica's own prompt is P again and
    the epoch's prompt is nulled.  Limits: an epoch with a navigation bit flip inside it has a small prompt and is
    under-subtracted (``states`` starts every channel on its code period, so a flip falls between epochs unless the code
    has slipped); and one amplitude per epoch takes one complex dimension of the noise per epoch out with the signal."""
    rec = np.asarray(records)
    if rec.ndim == 1:
        rec = rec[None, :]
    alpha = rec["prompt"].astype(np.float64) / (float(block_samples) * postcorr.MIXER_GAIN) * 2.0 ** postcorr.SUB_FRAC
    return np.floor(alpha + 0.5).astype(np.int32)


def main(argv=None) -> int:
    import argparse
    from . import Device
    ap = argparse.ArgumentParser(prog="python -m gpsjam.track", description="follow every acquired PRN through a capture: one line per PRN and second")
    ap.add_argument("input")
    ap.add_argument("--first-sample", type=int, default=0)
    ap.add_argument("--pull-in", type=int, default=200, help="epochs with the wide loops")
    ap.add_argument("--spacing", type=int, default=1, help="early / late taps, whole samples either side")
    ap.add_argument("--fs", type=float, default=2.048e6)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv)
    with Device(args.device) as dev:
        search = gnss.AcqSearch(dev, fs=args.fs)
        try:
            with dev.capture(args.input) as cap:
                tracks = follow(dev, cap, search, args.first_sample, args.pull_in, spacing=args.spacing)
        finally:
            search.close()
    if not tracks:
        print(f"{args.input}: no PRN acquired")
    for t in tracks:
        for w, (lock, cn0) in enumerate(zip(t.lock, t.cn0_dbhz)):
            lo, hi = w * t.window, min((w + 1) * t.window, t.doppler_hz.size) if w + 1 < t.lock.size else t.doppler_hz.size
            print(f"PRN {t.prn:2d}  {lo * t.block_s:7.2f} s  Doppler {t.doppler_hz[lo:hi].mean():+9.1f} Hz  code {t.code_phase_chips[lo]:8.3f} chips  "
                  f"C/N0 {cn0:5.1f} dB-Hz  lock {lock:.3f}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
