#!/usr/bin/env python3
"""The three-antenna canceller (gj_cancel2_dev) against the two-antenna canceller (gj_cancel_dev) on resident captures.

Per frame gj_cancel2_dev makes four transforms (a's, b's, c's, the inverse) where gj_cancel_dev makes three, reads three
captures where that one reads two, and writes the same bytes.  Both kernels run at two workgroups per CU with the same
runs.  The expectation this tool tests: about 4/3 of the pair's time in a family bound by instruction issue.  bench.py
does not time either, so the figures come from here:

  cancel2  gj_cancel2_dev over a 10-s synthetic triple (3 x 40 960 000 bytes, the auxiliaries delayed by 4 and 7 samples),
           one weight set (W1, W2) per 512 frames (|W| <= 0.7, random phases), thresholds at +inf, records on, HIP events
           around the call = both launches
  cancel   gj_cancel_dev over captures a and b with every set's W1, the same thresholds, records on, HIP events around the
           call = both launches

Both come from the same library and are interleaved call by call in one process, so that every pair of figures comes
from the same moment of the same GPU; both are warmed up first; medians over --steps pairs, with min and max.  Prints one
JSON line.  One process, one GPU; run it under a time limit of its own and chain it to other GPU steps with &&:
    timeout -k 10 300 python tools/cancel2_bench.py [--steps 200] [--warmup 20] [--nfft 256 1024 4096]"""
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
DELAYS = (0, 4, 7)


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
        caps = [dev.alloc(NBYTES) for _ in DELAYS]
        for ant, (cap, delay) in enumerate(zip(caps, DELAYS)):
            dev.synth_dev(StreamSpec(seed=9, antenna=ant, delay=delay, jam_start=n // 2, jam_end=1 << 40, jam_sigma=50.0), n, cap)
        d_out = dev.alloc(NBYTES)
        sizes = {}
        for nfft in args.nfft:
            frames = gpsjam.excise_frames(n, nfft)
            n_sets = -(-frames // FRAMES_PER_SET)
            rng = np.random.default_rng(nfft)
            w = (rng.uniform(0.0, 0.7, (n_sets, 2, nfft)) * np.exp(2j * np.pi * rng.uniform(0.0, 1.0, (n_sets, 2, nfft)))).astype(np.complex64)
            d_w2 = dev.alloc(w.nbytes).upload(w.view(np.float32).reshape(-1).view(np.uint8))
            w1 = np.ascontiguousarray(w[:, 0])
            d_w1 = dev.alloc(w1.nbytes).upload(w1.view(np.float32).reshape(-1).view(np.uint8))
            d_thr = dev.alloc(4 * nfft).upload(np.full(nfft, np.inf, np.float32).view(np.uint8))
            d_rec = dev.alloc(16 * frames)
            triple_ms, pair_ms = [], []
            for step in range(args.warmup + args.steps):
                dev.timer_start()
                dev.cancel2_dev(caps[0], NBYTES, 0, caps[1], NBYTES, 0, caps[2], NBYTES, 0, n, nfft, d_w2, FRAMES_PER_SET, n_sets, d_thr,
                                d_out, d_rec)
                t = dev.timer_stop()
                dev.timer_start()
                dev.cancel_dev(caps[0], NBYTES, 0, caps[1], NBYTES, 0, n, nfft, d_w1, FRAMES_PER_SET, n_sets, d_thr, d_out, d_rec)
                p = dev.timer_stop()
                if step >= args.warmup:
                    triple_ms.append(t)
                    pair_ms.append(p)
            t, p = statistics.median(triple_ms), statistics.median(pair_ms)
            sizes[str(nfft)] = {"frames": frames, "weight_sets": n_sets, "cancel2_ms": round(t, 4), "cancel2_ms_min": round(min(triple_ms), 4),
                                "cancel2_ms_max": round(max(triple_ms), 4), "cancel_ms": round(p, 4), "cancel_ms_min": round(min(pair_ms), 4),
                                "cancel_ms_max": round(max(pair_ms), 4), "cancel2_over_cancel": round(t / p, 3),
                                "cancel2_read_gb_s": round(3 * NBYTES / t / 1e6, 1)}
            for buf in (d_w2, d_w1, d_thr, d_rec):
                buf.free()
        for buf in (*caps, d_out):
            buf.free()
        info = dev.info()
    print(json.dumps({"bench": "cancel2_vs_cancel", "device": info["name"], "capture_bytes": NBYTES, "frames_per_set": FRAMES_PER_SET,
                      "steps": args.steps, "warmup": args.warmup, "sizes": sizes}))


if __name__ == "__main__":
    main()
