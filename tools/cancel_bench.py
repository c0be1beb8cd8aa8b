#!/usr/bin/env python3
"""The two-antenna canceller (gj_cancel_dev) against the excisor (gj_excise_dev) on one resident capture pair.

Per frame the canceller makes three transforms (a's, b's, the inverse) where the excisor makes two, reads two captures
where the excisor reads one, and writes the same bytes.  Both kernels run at two workgroups per CU with the same runs.
The expectation this tool tests: about 1.5 x the excisor's time in a family bound by instruction issue.  bench.py does
not time either, so the figures come from here:

  cancel  gj_cancel_dev over a 10-s synthetic pair (2 x 40 960 000 bytes, the second antenna delayed by 4 samples), one
          weight set per 512 frames (|W| <= 1, random phases), thresholds at +inf, records on, HIP events around the
          call = both launches
  excise  gj_excise_dev over capture a, the same thresholds, records on, HIP events around the call = both launches

Both come from the same library and are interleaved call by call, so that every pair of figures comes from the same
moment of the same GPU; both are warmed up first; medians over --steps pairs, with min and max.  Prints one JSON line.
    python tools/cancel_bench.py [--steps 200] [--warmup 20] [--nfft 256 1024 4096]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "gps-jamming_amd"), REPO]
NBYTES = 40960000
FRAMES_PER_SET = 512


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--nfft", type=int, nargs="+", default=[256, 1024, 4096])
    args = ap.parse_args()
    import gpsjam
    from gpsjam.synth import StreamSpec
    n = NBYTES // 2
    with gpsjam.Device(0) as dev:
        caps = [dev.alloc(NBYTES), dev.alloc(NBYTES)]
        for ant, (cap, delay) in enumerate(zip(caps, (0, 4))):
            dev.synth_dev(StreamSpec(seed=9, antenna=ant, delay=delay, jam_start=n // 2, jam_end=1 << 40, jam_sigma=50.0), n, cap)
        d_out = dev.alloc(NBYTES)
        sizes = {}
        for nfft in args.nfft:
            frames = gpsjam.excise_frames(n, nfft)
            n_sets = -(-frames // FRAMES_PER_SET)
            rng = np.random.default_rng(nfft)
            w = (rng.uniform(0.0, 1.0, (n_sets, nfft)) * np.exp(2j * np.pi * rng.uniform(0.0, 1.0, (n_sets, nfft)))).astype(np.complex64)
            d_w = dev.alloc(w.nbytes).upload(w.view(np.float32))
            d_thr = dev.alloc(4 * nfft).upload(np.full(nfft, np.inf, np.float32))
            d_rec = dev.alloc(16 * frames)
            cancel_ms, excise_ms = [], []
            for step in range(args.warmup + args.steps):
                dev.timer_start()
                dev.cancel_dev(caps[0], NBYTES, 0, caps[1], NBYTES, 0, n, nfft, d_w, FRAMES_PER_SET, n_sets, d_thr, d_out, d_rec)
                c = dev.timer_stop()
                dev.timer_start()
                dev.excise_dev(caps[0], NBYTES, 0, n, nfft, d_thr, d_out, d_rec)
                e = dev.timer_stop()
                if step >= args.warmup:
                    cancel_ms.append(c)
                    excise_ms.append(e)
            c, e = statistics.median(cancel_ms), statistics.median(excise_ms)
            sizes[str(nfft)] = {"frames": frames, "weight_sets": n_sets, "cancel_ms": round(c, 4), "cancel_ms_min": round(min(cancel_ms), 4),
                                "cancel_ms_max": round(max(cancel_ms), 4), "excise_ms": round(e, 4), "excise_ms_min": round(min(excise_ms), 4),
                                "excise_ms_max": round(max(excise_ms), 4), "cancel_over_excise": round(c / e, 3),
                                "cancel_read_gb_s": round(2 * NBYTES / c / 1e6, 1)}
            for buf in (d_w, d_thr, d_rec):
                buf.free()
        for buf in (*caps, d_out):
            buf.free()
        info = dev.info()
    print(json.dumps({"bench": "cancel_vs_excise", "device": info["name"], "capture_bytes": NBYTES, "frames_per_set": FRAMES_PER_SET,
                      "steps": args.steps, "warmup": args.warmup, "sizes": sizes}))


if __name__ == "__main__":
    main()
