"""Pair alignment: antenna b resampled and retuned onto antenna a's clock (``Device.align``, gj_align_dev).

Every two-antenna feature of the project (``coherence.scan``, ``mitigate.clean_spatial`` / ``clean_spatial2``,
``spoof.scan`` / ``scan_peaks``, ``mitigate.clean_spoofed``, ``tdoa.refine``) asks for sample-aligned captures on one
clock.  Receivers that each run on a crystal of their own do not deliver that: the crystal sets the sample clock AND the
tuner, so a relative error of 1 ppm is a slip of 20 samples over a 10-s capture and a carrier offset of 1575 Hz at L1.
This module estimates the three constants of such a pair and writes b again as a would have sampled it:

    taps, rot_table     the int16 tables of the kernel: a Kaiser-windowed sinc at 256 sub-sample positions, one turn
    params              (lag, drift, offset_hz) -> the kernel's fixed-point time base and phase
    estimate            lag, drift and offset of b against a, from the library's own correlators
    to                  the aligned capture: a ``Capture`` of a's length, usable wherever a ``Capture`` is

The model, in K5's sign convention (a positive lag: b is delayed): sample n of a and sample ``n * (1 + drift) + lag`` of
b show the source at the same instant, and b sees it ``offset_hz`` higher.  ``drift`` > 0: b's clock is fast.

The estimate has three passes, each on the GPU but for a few hundred numbers:

 0. the cross-ambiguity search (``Device.xcorr_caf``) on slices spread over the capture: per slice the integer lag, and
    over all of them the offset's bin (the median);
 1. b with that offset taken out (the kernel with the identity time base) against a: the exact lag-window correlation
    of every slice (``Device.xcorr_fine``) with its block records.  The phase progression of the records at the peak
    lag gives the offset that is left -- as the slices see it: a jammer f_j off the centre frequency appears
    ``f_j * drift`` lower in b, which no tuner caused -- and ``tdoa.fine_lag`` per slice with a straight line through
    the slices gives lag and drift;
 2. b aligned with what pass 1 found against a: one correlation over the whole capture around lag 0, whose records give
    the offset that is left now that the time bases agree, and the lag and drift that are left (a Newton step).

With ``rf_hz`` the drift is ``offset_hz / rf_hz`` instead of the line's slope: one crystal drives both, and the offset
is by far the better-measured of the two.  ``rf_hz`` carries the sign of the tuner's conversion: where baseband is
``f - f_LO`` and f_LO rises with the crystal, a fast b sees the source LOWER, and ``rf_hz = -f_LO`` says so.

Limits: a common source with bandwidth (a jammer) must be in both captures -- a carrier has a
phase, not a delay, and noise alone has neither; drift and offset are constants of the capture (a crystal that warms up
during it is not followed); and the aligned capture is rounded to bytes once more, which adds 1/12 LSB^2 per component.
"""
from __future__ import annotations

import contextlib
from typing import NamedTuple, Optional

import numpy as np

from . import ALIGN_PHASES, ALIGN_ROT_LEN, ALIGN_TAPS, FINE_BLOCK, AlignParams, Capture, FineCorr, GJ_LAG_INVALID, tdoa

__all__ = ["UNIT", "BETA", "taps", "rot_table", "params", "Estimate", "estimate", "to", "main"]

UNIT = 16384             # unit gain of both tables
BETA = 5.0               # Kaiser window of the taps: profiles/NOTES_align.md has the sweep
HALF = ALIGN_TAPS // 2   # the sinc's support, samples either side of the interpolation point
MIN_SLICE = 8192         # two block records: the least a slice's offset can be read from


def taps(beta: float = BETA) -> np.ndarray:
    """int16[ALIGN_PHASES][ALIGN_TAPS]: row p interpolates at sample k + p / 256 from samples k - 7 .. k + 8, a sinc
    under a Kaiser window of support +-8 around the interpolation point.  Every row is scaled to unit DC gain, rounded,
    and corrected on its largest tap so that it sums to exactly UNIT; row 0 is exactly the delta at tap 7."""
    frac = np.arange(ALIGN_PHASES, dtype=np.float64)[:, None] / ALIGN_PHASES
    x = np.arange(ALIGN_TAPS, dtype=np.float64)[None, :] - (HALF - 1) - frac            # tap position less the point's
    window = np.i0(float(beta) * np.sqrt(np.clip(1.0 - (x / HALF) ** 2, 0.0, None))) / np.i0(float(beta))
    h = np.sinc(x) * window
    rows = np.rint(UNIT * h / h.sum(axis=1, keepdims=True)).astype(np.int64)
    top = np.argmax(rows, axis=1)
    rows[np.arange(ALIGN_PHASES), top] += UNIT - rows.sum(axis=1)
    return rows.astype(np.int16)


def rot_table() -> np.ndarray:
    """int16[ALIGN_ROT_LEN]: UNIT * cos(2 pi i / 1024), rounded; the kernel reads the sine a quarter turn behind."""
    return np.rint(UNIT * np.cos(2.0 * np.pi * np.arange(ALIGN_ROT_LEN) / ALIGN_ROT_LEN)).astype(np.int16)


def params(lag: float = 0.0, drift: float = 0.0, offset_hz: float = 0.0, fs: float = 2.048e6) -> AlignParams:
    """The kernel's parameters for the model above: output sample n takes b at ``n * (1 + drift) + lag``, and the
    rotation takes ``offset_hz`` out at that source time.  The library refuses |drift| above 2^-8 and |lag| from 2^28."""
    step = 1.0 + float(drift)
    turn = -float(offset_hz) / float(fs)                     # turns per source sample
    return AlignParams(int(round(float(lag) * 2.0 ** 32)), int(round(step * 2.0 ** 32)),
                       int(round((turn * float(lag)) % 1.0 * 2.0 ** 32)) & 0xFFFFFFFF,
                       int(round((turn * step) % 1.0 * 2.0 ** 32)) & 0xFFFFFFFF, 0)


class Estimate(NamedTuple):
    lag: float               # samples by which b lags a at a's sample 0
    drift: float             # b's samples per sample of a, less 1
    offset_hz: float         # b sees the source that much higher
    coarse_lags: tuple       # pass 0: the cross-ambiguity search's integer lag of every slice
    coarse_offset_hz: float  # pass 0: the median of their offset bins
    slice_times: np.ndarray  # pass 1: a's sample index at the middle of every slice
    slice_lags: np.ndarray   # pass 1: the fine lag there (NaN where the estimator gave none)
    spread: float            # pass 2: rms distance of the residual lags from their line, samples
    ok: bool                 # every pass had what it needs


@contextlib.contextmanager
def _window(cap: Capture, first: int, n: int):
    """Samples first .. first + n of a resident capture as a ``Capture`` in place: nothing is copied, and nothing is
    freed on the way out."""
    view = Capture.__new__(Capture)
    view.dev, view.ptr, view.nbytes, view.path = cap.dev, cap.ptr + 2 * int(first), 2 * int(n), None
    view.results, view.ingest_ms, view.results_unpack = {}, None, None
    try:
        yield view
    finally:
        view.ptr = 0


def _phase_slope(blocks: np.ndarray, n_samples: int):
    """(numerator, denominator, column) of the weighted least-squares slope, radians per sample, of the block records'
    phase at the lag where they are strongest; the weights are the records' magnitudes."""
    mag = np.abs(blocks)
    col = int(np.argmax(mag.sum(axis=0)))
    z, w = blocks[:, col], mag[:, col]
    if z.size < 2 or not np.isfinite(w).all() or w.sum() <= 0.0:
        return 0.0, 0.0, col
    start = FINE_BLOCK * np.arange(z.size, dtype=np.float64)
    t = 0.5 * (start + np.minimum(start + FINE_BLOCK, float(n_samples)))
    ph = np.unwrap(np.angle(z))
    tm, pm = (w * t).sum() / w.sum(), (w * ph).sum() / w.sum()
    return float((w * (t - tm) * (ph - pm)).sum()), float((w * (t - tm) ** 2).sum()), col


def _line(t: np.ndarray, y: np.ndarray, slope: Optional[float] = None):
    """(intercept, slope, rms residual) of the least-squares line through the finite points; ``slope`` given: only the
    intercept is fitted.  (nan, 0, 0) without a point; one point, or a given slope: the slope is not fitted."""
    keep = np.isfinite(y)
    t, y = t[keep], y[keep]
    if t.size == 0:
        return float("nan"), 0.0 if slope is None else float(slope), 0.0
    if slope is None:
        slope = float(np.polyfit(t, y, 1)[0]) if t.size >= 2 else 0.0
    resid = y - slope * t
    return float(resid.mean()), float(slope), float(np.sqrt(np.mean((resid - resid.mean()) ** 2)))


def _slices(n: int, n_slices: int, slice_samples: int):
    length = min(int(slice_samples), max(MIN_SLICE, n // max(int(n_slices), 1)), n)
    count = max(1, min(int(n_slices), n // max(length, 1)))
    return [int(s) for s in np.linspace(0, n - length, count)], length


def estimate(dev, a, b, rf_hz: Optional[float] = None, fs: float = 2.048e6, n_slices: int = 8, slice_samples: int = 65536,
             max_offset_hz: float = 4000.0, half_width: int = 16, beta: float = BETA) -> Estimate:
    """Lag, drift and offset of ``b`` against ``a`` (host bytes, uploaded once each, or resident ``Capture``s) by the
    three passes of the module's text.  ``n_slices`` slices of ``slice_samples`` samples (fewer and shorter on a short
    capture, never under 8192 samples while the capture holds that many); ``max_offset_hz``: the range of the
    cross-ambiguity search; ``half_width``: the lag window of the fine correlation, which the drift across ONE slice
    must stay inside."""
    tp, rt = taps(beta), rot_table()
    with contextlib.ExitStack() as temps:
        cap_a, cap_b = dev._residents(temps, a, b)
        n = min(cap_a.nsamples, cap_b.nsamples)
        if n < 2:
            raise ValueError("the captures are too short to align")
        starts, length = _slices(n, n_slices, slice_samples)
        d_taps = dev._on_device(temps, tp, np.int16, tp.size, "taps", "")
        d_rot = dev._on_device(temps, rt, np.int16, rt.size, "rot", "")

        # ---- pass 0: integer lag per slice, the offset's bin
        views = [temps.enter_context(_window(cap, s, length)) for s in starts for cap in (cap_a, cap_b)]
        peaks = dev.xcorr_caf(views, [(2 * k, 2 * k + 1) for k in range(len(starts))], max_offset_hz=max_offset_hz, fs=fs)
        found = [p for p in peaks if p.lag != GJ_LAG_INVALID]
        if not found:
            raise ValueError("the captures share nothing the cross-ambiguity search can find")
        f0 = float(np.median([p.offset_hz for p in found]))
        lag0 = int(np.median([p.lag for p in found]))
        coarse = tuple(int(p.lag) if p.lag != GJ_LAG_INVALID else lag0 for p in peaks)

        # ---- pass 1: the offset taken out, every slice's fine correlation
        b1, _ = dev.align(cap_b, params(0.0, 0.0, f0, fs), d_taps, d_rot)
        temps.callback(b1.free)
        corrs = [dev.xcorr_fine(cap_a, b1, lag_center=c, half_width=half_width, first_a=s, first_b=s, n_samples=length, want_blocks=True)
                 for s, c in zip(starts, coarse)]
        num = den = 0.0
        for c in corrs:
            u, v, _ = _phase_slope(c.blocks, c.n_samples)
            num, den = num + u, den + v
        f1 = num / den * fs / (2.0 * np.pi) if den > 0.0 else 0.0
        fine = [tdoa.fine_lag(c, offset_hz=f1, fs=fs) for c in corrs]
        times = np.array(starts, np.float64) + 0.5 * length
        lags = np.array([fl.lag if fl.ok else np.nan for fl in fine])
        drift1 = None if rf_hz is None else (f0 + f1) / float(rf_hz)
        lag1, drift1, _ = _line(times, lags, drift1)
        ok = bool(np.isfinite(lag1) and den > 0.0)
        if not np.isfinite(lag1):
            lag1 = float(lag0)

        # ---- pass 2: aligned by pass 1; what is left, over the whole capture
        b2, _ = dev.align(cap_b, params(lag1, drift1, f0 + f1, fs), d_taps, d_rot, n_out=cap_a.nsamples)
        temps.callback(b2.free)
        whole = dev.xcorr_fine(cap_a, b2, lag_center=0, half_width=half_width, want_blocks=True)
        u, v, _ = _phase_slope(whole.blocks, whole.n_samples)
        f2 = u / v * fs / (2.0 * np.pi) if v > 0.0 else 0.0
        nb = whole.blocks.shape[0]
        start = FINE_BLOCK * np.arange(nb, dtype=np.float64)
        mid = 0.5 * (start + np.minimum(start + FINE_BLOCK, float(whole.n_samples)))
        turned = whole.blocks * np.exp(-2j * np.pi * f2 * mid / fs)[:, None]
        per = max(1, -(-nb // max(len(starts), 2)))
        points = tdoa.series(FineCorr(whole.lags, turned.sum(axis=0), turned, whole.n_samples), per)
        t2 = np.array([0.5 * (FINE_BLOCK * m + min(FINE_BLOCK * (m + per), whole.n_samples)) for m in range(0, nb, per)], np.float64)
        l2 = np.array([p.lag if p.ok else np.nan for p in points])
        offset = f0 + f1 + f2
        if rf_hz is None:
            slope = None if np.isfinite(l2).sum() >= 3 else 0.0
        else:                                                 # the drift that is left is known: the offset's, less pass 1's
            slope = (1.0 + offset / float(rf_hz)) / (1.0 + drift1) - 1.0
        lag2, drift2, spread = _line(t2, l2, slope)
        if not np.isfinite(lag2):
            lag2, ok = 0.0, False

    drift = (1.0 + drift1) * (1.0 + drift2) - 1.0 if rf_hz is None else offset / float(rf_hz)
    return Estimate(lag1 + lag2 * (1.0 + drift1), drift, offset, coarse, f0, times, lags, spread, ok)


_estimate = estimate      # ``to`` takes an argument of that name


def to(dev, a, b, estimate: Optional[Estimate] = None, fs: float = 2.048e6, beta: float = BETA, **search) -> Capture:
    """``b`` on a's clock: a resident ``Capture`` of a's length (the caller frees it), sample n of which shows what a's
    sample n shows.  ``estimate``: what ``align.estimate`` found (default: it is run here, with ``search`` passed on)."""
    with contextlib.ExitStack() as temps:
        cap_a, cap_b = dev._residents(temps, a, b)
        est = _estimate(dev, cap_a, cap_b, fs=fs, beta=beta, **search) if estimate is None else estimate
        aligned, _ = dev.align(cap_b, params(est.lag, est.drift, est.offset_hz, fs), taps(beta), rot_table(), n_out=cap_a.nsamples)
    return aligned


def main(argv=None) -> int:
    import argparse
    from . import Device
    ap = argparse.ArgumentParser(prog="python -m gpsjam.align", description="estimate lag, drift and offset of capture B against "
                                 "capture A and write B again on A's clock")
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("out_b")
    ap.add_argument("--rf-hz", type=float, default=None, help="tuned frequency, signed: the drift is offset / rf-hz")
    ap.add_argument("--fs", type=float, default=2.048e6)
    ap.add_argument("--max-offset-hz", type=float, default=4000.0)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv)
    with Device(args.device) as dev:
        with dev.capture(args.a) as cap_a, dev.capture(args.b) as cap_b:
            est = estimate(dev, cap_a, cap_b, rf_hz=args.rf_hz, fs=args.fs, max_offset_hz=args.max_offset_hz)
            with to(dev, cap_a, cap_b, est, fs=args.fs) as aligned:
                aligned.download().tofile(args.out_b)
                n = aligned.nsamples
    print(f"{args.b} against {args.a}: lag {est.lag:+.3f} samples, drift {est.drift * 1e6:+.3f} ppm, offset {est.offset_hz:+.2f} Hz "
          f"(search: {est.coarse_offset_hz:+.1f} Hz, lags {list(est.coarse_lags)}), residual spread {est.spread:.3f} samples, "
          f"{'ok' if est.ok else 'NOT ok'}")
    print(f"{args.out_b}: {n} samples on {args.a}'s clock")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
