#!/usr/bin/env python3
"""The pulse blanker (gj_blank_dev) against a device-to-device copy and against the excisor on one resident capture
(DESIGN section 4).

The blanker reads every byte of the capture once and writes as many: a copy of the same byte count is the floor for any
kernel of that shape.  The excisor (gj_excise_dev at 1024 points) is what a pulsed jammer would otherwise be handed to.
bench.py does not time either, so the figures come from here:

  blank   gj_blank_dev at (window, guard) = (1, 0), (16, 8) and (1024, 1024) over a whole 10-s synthetic capture
          (40 960 000 bytes), threshold 4 x the noise power, records on, HIP events around the call (one launch)
  excise  gj_excise_dev at nfft 1024, a flat threshold 16 x the noise floor, frame records on (both launches)
  copy    torch's device-to-device copy of the 40 960 000 bytes, between the same events on the same stream

The five are interleaved call by call, so that every set of figures comes from the same moment of the same GPU; every
shape is warmed up first; medians over --steps rounds.  The capture fits the 256 MiB Infinity Cache, for all five alike.
Prints one JSON line.
    python tools/blank_bench.py [--steps 200] [--warmup 20]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "gps-jamming_amd"), REPO]
NBYTES = 40960000
SHAPES = ((1, 0), (16, 8), (1024, 1024))
NFFT = 1024
NOISE_SIGMA = 6.25


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    import torch
    import gpsjam
    from gpsjam.synth import StreamSpec
    n = NBYTES // 2
    with gpsjam.Device(0) as dev:
        dev.set_stream(torch.cuda.current_stream().cuda_stream)
        cap = torch.empty(NBYTES, dtype=torch.uint8, device="cuda")
        out = torch.empty(NBYTES, dtype=torch.uint8, device="cuda")
        dev.synth_dev(StreamSpec(seed=9, antenna=0, delay=0, jam_start=n // 2, jam_end=1 << 40, jam_sigma=50.0), n, cap)
        blocks, frames = gpsjam.blank_blocks(n), gpsjam.excise_frames(n, NFFT)
        d_rec = dev.alloc(max(blocks * gpsjam.BLANK_DTYPE.itemsize, frames * gpsjam.EXCISE_DTYPE.itemsize))
        floor = 0.375 * NFFT * 2.0 * NOISE_SIGMA ** 2 / 127.5 ** 2
        d_thr = dev.alloc(4 * NFFT).upload(np.full(NFFT, 16.0 * floor, np.float32))
        threshold = 4.0 * 2.0 * NOISE_SIGMA ** 2
        ms = {name: [] for name in ("copy", "excise") + SHAPES}
        for step in range(args.warmup + args.steps):
            got = {}
            dev.timer_start()
            out.copy_(cap)
            got["copy"] = dev.timer_stop()
            for window, guard in SHAPES:
                dev.timer_start()
                dev.blank_dev(cap, NBYTES, 0, n, window, guard, threshold, out, d_rec)
                got[(window, guard)] = dev.timer_stop()
            dev.timer_start()
            dev.excise_dev(cap, NBYTES, 0, n, NFFT, d_thr, out, d_rec)
            got["excise"] = dev.timer_stop()
            if step >= args.warmup:
                for k, v in got.items():
                    ms[k].append(v)
        rec = None
        rows = {}
        copy, excise = statistics.median(ms["copy"]), statistics.median(ms["excise"])
        for window, guard in SHAPES:
            dev.blank_dev(cap, NBYTES, 0, n, window, guard, threshold, out, d_rec)
            rec = d_rec.download(gpsjam.BLANK_DTYPE, blocks)
            t = statistics.median(ms[(window, guard)])
            rows[f"{window},{guard}"] = {"blank_ms": round(t, 4), "blank_ms_min": round(min(ms[(window, guard)]), 4),
                                         "blank_ms_max": round(max(ms[(window, guard)]), 4), "blank_over_copy": round(t / copy, 3),
                                         "blank_over_excise": round(t / excise, 3), "read_plus_write_gb_s": round(2 * NBYTES / t / 1e6, 1),
                                         "blanked_share": round(float(rec["n_blanked"].sum()) / n, 4)}
        info = dev.info()
        dev.set_stream(None, external=False)
        d_rec.free()
        d_thr.free()
    print(json.dumps({"bench": "blank_vs_copy_and_excise", "device": info["name"], "capture_bytes": NBYTES, "steps": args.steps,
                      "warmup": args.warmup, "copy_ms": round(copy, 4), "copy_ms_min": round(min(ms["copy"]), 4),
                      "copy_ms_max": round(max(ms["copy"]), 4), "copy_read_plus_write_gb_s": round(2 * NBYTES / copy / 1e6, 1),
                      "excise_1024_ms": round(excise, 4), "excise_1024_ms_min": round(min(ms["excise"]), 4),
                      "excise_1024_ms_max": round(max(ms["excise"]), 4), "shapes": rows}))


if __name__ == "__main__":
    main()
