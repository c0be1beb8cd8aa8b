#!/usr/bin/env python3
"""The pair alignment (gj_align_dev) against a device-to-device copy of the same bytes, on one resident capture.

The alignment reads every byte of the source once and writes as many: a copy of the same bytes is the floor for any
kernel of that shape.  On top of it come 32 multiply-adds and 16 LDS words per sample for the interpolation and four
64-bit products for the rotation.  bench.py times none of this, so the figures come from here:

  align     gj_align_dev over a whole 10-s capture (20 480 000 samples, 40 960 000 bytes) with the library's own tables,
            HIP events around the call (one launch): a pair 3.25 samples, 40 ppm and 300 Hz apart with records; the same
            without records; the identity time base (rotation only); the largest drift (2^-8)
  copy      torch's device-to-device copy of 40 960 000 bytes between the same events on the same stream

All are interleaved call by call, so that every set of figures comes from the same moment of the same GPU; every shape is
warmed up first; medians, minima and maxima over --steps rounds.  The capture fits the 256 MiB Infinity Cache, for all
alike.  Prints one JSON line.
    python tools/align_bench.py [--steps 50] [--warmup 5]"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "gps-jamming_amd"), REPO]
NBYTES = 40960000
FS = 2.048e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import torch
    import gpsjam
    from gpsjam import align
    from gpsjam.synth import StreamSpec
    n = NBYTES // 2
    with gpsjam.Device(0) as dev:
        dev.set_stream(torch.cuda.current_stream().cuda_stream)
        cap = torch.empty(NBYTES, dtype=torch.uint8, device="cuda")
        out = torch.empty(NBYTES, dtype=torch.uint8, device="cuda")
        dev.synth_dev(StreamSpec(seed=9, antenna=0, delay=0, jam_start=1 << 40, jam_end=1 << 40, jam_sigma=0.0), n, cap)
        taps, rot = align.taps(), align.rot_table()
        d_taps, d_rot = dev.alloc(taps.nbytes).upload(taps), dev.alloc(rot.nbytes).upload(rot)
        d_rec = dev.alloc(16 * gpsjam.align_blocks(n))
        pair = align.params(3.25, 40e-6, 300.0, FS)
        shapes = {"align_pair": (pair, True), "align_pair_no_records": (pair, False),
                  "align_rotation_only": (align.params(0.0, 0.0, 300.0, FS), True),
                  "align_largest_drift": (align.params(3.25, 2.0 ** -8, 300.0, FS), True)}
        names = ("copy",) + tuple(shapes)
        ms = {name: [] for name in names}
        for step in range(args.warmup + args.steps):
            got = {}
            dev.timer_start()
            out.copy_(cap)
            got["copy"] = dev.timer_stop()
            for name, (p, records) in shapes.items():
                dev.timer_start()
                dev.align_dev(cap, NBYTES, p, d_taps, d_rot, n, out, d_rec if records else None)
                got[name] = dev.timer_stop()
            if step >= args.warmup:
                for k, v in got.items():
                    ms[k].append(v)
        # the same bytes twice: the launch is deterministic; and the identity is the copy
        dev.align_dev(cap, NBYTES, pair, d_taps, d_rot, n, out, d_rec)
        dev.synchronize()
        first = out[:1 << 20].cpu().numpy().tobytes()
        dev.align_dev(cap, NBYTES, pair, d_taps, d_rot, n, out, d_rec)
        dev.synchronize()
        assert first == out[:1 << 20].cpu().numpy().tobytes()
        dev.align_dev(cap, NBYTES, align.params(), d_taps, d_rot, n, out, None)
        dev.synchronize()
        assert torch.equal(out, cap)
        info = dev.info()
        dev.set_stream(None, external=False)
        for buf in (d_taps, d_rot, d_rec):
            buf.free()
    med = {k: statistics.median(v) for k, v in ms.items()}
    row = {"bench": "align_vs_copy", "device": info["name"], "capture_bytes": NBYTES, "steps": args.steps, "warmup": args.warmup}
    for k in names:
        row[f"{k}_ms"] = round(med[k], 4)
        row[f"{k}_ms_min"], row[f"{k}_ms_max"] = round(min(ms[k]), 4), round(max(ms[k]), 4)
    row["copy_read_plus_write_gb_s"] = round(2 * NBYTES / med["copy"] / 1e6, 1)
    row["align_pair_over_copy"] = round(med["align_pair"] / med["copy"], 2)
    row["align_pair_gsample_s"] = round(n / med["align_pair"] / 1e6, 2)
    row["align_pair_read_plus_write_gb_s"] = round(2 * NBYTES / med["align_pair"] / 1e6, 1)
    print(json.dumps(row))


if __name__ == "__main__":
    main()
