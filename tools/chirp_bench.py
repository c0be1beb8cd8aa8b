#!/usr/bin/env python3
"""The chirp-rate search (gj_chirp_dev) against the ridge (gj_ridge_dev) on one resident capture.

The search loads, unpacks and windows a frame once and transforms it once per rate; R ridge calls would load it R times.
What a rate adds on top of the ridge's transform is the de-chirp: sixteen sine / cosine pairs and complex products per
thread.  bench.py does not time either kernel, so the figures come from here:

  chirp   gj_chirp_dev at nfft 256, hop 128, 1, 16 and 64 rates from 0 at step 1, all frames of a 10-s synthetic capture
          (40 960 000 bytes), no d_peaks, HIP events around one launch
  ridge   gj_ridge_dev at the same nfft and hop on the same capture

The calls are interleaved round by round, so that every set of figures comes from the same moment of the same GPU; every
shape is warmed up first; medians over --steps rounds.  Prints one JSON line.
    python tools/chirp_bench.py [--steps 50] [--warmup 5]"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "gps-jamming_amd"), REPO]
NBYTES = 40960000
NFFT, HOP = 256, 128
RATES = (1, 16, 64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import gpsjam
    from gpsjam.synth import StreamSpec
    n = NBYTES // 2
    with gpsjam.Device(0) as dev:
        cap = dev.alloc(NBYTES)
        dev.synth_dev(StreamSpec(seed=9, antenna=0, delay=0, jam_start=n // 2, jam_end=1 << 40, jam_sigma=50.0), n, cap)
        frames = gpsjam.ridge_frames(NBYTES, 0, NFFT, HOP)
        d_ridge = dev.alloc(frames * gpsjam.RIDGE_DTYPE.itemsize)
        d_chirp = dev.alloc(frames * gpsjam.CHIRP_DTYPE.itemsize)
        ridge_ms, chirp_ms = [], {r: [] for r in RATES}
        for step in range(args.warmup + args.steps):
            dev.timer_start()
            dev.ridge_dev(cap, NBYTES, 0, NFFT, HOP, frames, 2, d_ridge)
            t = dev.timer_stop()
            if step >= args.warmup:
                ridge_ms.append(t)
            for r in RATES:
                dev.timer_start()
                dev.chirp_dev(cap, NBYTES, 0, NFFT, HOP, frames, 2, 0, 1, r, d_chirp)
                t = dev.timer_stop()
                if step >= args.warmup:
                    chirp_ms[r].append(t)
        ridge = statistics.median(ridge_ms)
        rows = {}
        for r in RATES:
            c = statistics.median(chirp_ms[r])
            rows[str(r)] = {"chirp_ms": round(c, 4), "chirp_ms_min": round(min(chirp_ms[r]), 4),
                            "chirp_ms_max": round(max(chirp_ms[r]), 4), "ms_per_rate": round(c / r, 4),
                            "over_as_many_ridge_calls": round(c / (r * ridge), 3)}
        for b in (d_ridge, d_chirp, cap):
            b.free()
        info = dev.info()
    print(json.dumps({"bench": "chirp_vs_ridge", "device": info["name"], "capture_bytes": NBYTES, "nfft": NFFT, "hop": HOP,
                      "frames": frames, "steps": args.steps, "warmup": args.warmup, "ridge_ms": round(ridge, 4),
                      "ridge_ms_min": round(min(ridge_ms), 4), "ridge_ms_max": round(max(ridge_ms), 4), "rates": rows}))


if __name__ == "__main__":
    main()
