#!/usr/bin/env python3
"""The lag-window correlation (gj_xcorr_fine_dev) against a device-to-device copy and against K5 on one resident pair of
captures.

The kernel reads every byte of both ranges once and writes next to nothing: a copy that reads as many bytes is the floor
for any kernel of that shape (it also writes them, which the kernel does not).  K5 (gj_xcorr_lags_dev) is what finds the
integer lag that the window is centred on.  bench.py times neither, so the figures come from here:

  whole    gj_xcorr_fine_dev at R = 16 over a whole 10-s pair (2 x 40 960 000 bytes), once with block records and once
           without, HIP events around the call (a memset and one launch)
  copy     torch's device-to-device copy of 2 x 40 960 000 bytes between the same events on the same stream
  slice    gj_xcorr_fine_dev at R = 16 over the reference's 50 000-sample slice, and K5 over the same slice

All are interleaved call by call, so that every set of figures comes from the same moment of the same GPU; every shape is
warmed up first; medians, minima and maxima over --steps rounds.  The pair fits the 256 MiB Infinity Cache, for all alike.
Prints one JSON line.
    python tools/fine_bench.py [--steps 200] [--warmup 20]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "gps-jamming_amd"), REPO]
NBYTES = 40960000
HALF = 16
SLICE = 50000
DELAY = 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    import torch
    import gpsjam
    from gpsjam.synth import StreamSpec
    n, nl = NBYTES // 2, 2 * HALF + 1
    with gpsjam.Device(0) as dev:
        dev.set_stream(torch.cuda.current_stream().cuda_stream)
        pair = torch.empty(2 * NBYTES, dtype=torch.uint8, device="cuda")
        out = torch.empty(2 * NBYTES, dtype=torch.uint8, device="cuda")
        a, b = pair[:NBYTES], pair[NBYTES:]
        for ant, (cap, delay) in enumerate(((a, 0), (b, DELAY))):
            dev.synth_dev(StreamSpec(seed=9, antenna=ant, delay=delay, jam_start=0, jam_end=1 << 40, jam_sigma=40.0), n, cap)
        blocks = gpsjam.fine_blocks(n)
        d_total, d_blocks = dev.alloc(16 * nl), dev.alloc(8 * nl * blocks)
        d_starts = dev.alloc(16).upload(np.zeros(2, np.int64))
        d_k5 = dev.alloc(3 * 4)
        dev.reserve(dev.xcorr_workspace(2, SLICE, 1))
        names = ("copy", "fine_blocks", "fine", "fine_slice", "k5_slice")
        ms = {name: [] for name in names}
        for step in range(args.warmup + args.steps):
            got = {}
            dev.timer_start()
            out.copy_(pair)
            got["copy"] = dev.timer_stop()
            dev.timer_start()
            dev.xcorr_fine_dev(a, NBYTES, 0, b, NBYTES, 0, n, DELAY, HALF, d_total, d_blocks)
            got["fine_blocks"] = dev.timer_stop()
            dev.timer_start()
            dev.xcorr_fine_dev(a, NBYTES, 0, b, NBYTES, 0, n, DELAY, HALF, d_total, None)
            got["fine"] = dev.timer_stop()
            dev.timer_start()
            dev.xcorr_fine_dev(a, NBYTES, 0, b, NBYTES, 0, SLICE, DELAY, HALF, d_total, None)
            got["fine_slice"] = dev.timer_stop()
            dev.timer_start()
            dev.xcorr_lags_dev([a, b], [NBYTES, NBYTES], d_starts, SLICE, [(0, 1)], d_k5.ptr, d_k5.ptr + 4, d_k5.ptr + 8)
            got["k5_slice"] = dev.timer_stop()
            if step >= args.warmup:
                for k, v in got.items():
                    ms[k].append(v)
        k5_lag = int(d_k5.download(np.int32, 1)[0])
        dev.xcorr_fine_dev(a, NBYTES, 0, b, NBYTES, 0, n, DELAY, HALF, d_total, d_blocks)
        total = d_total.download(np.int64, 2 * nl).reshape(nl, 2)
        rec = d_blocks.download(np.int32, 2 * nl * blocks).reshape(blocks, nl, 2)
        info = dev.info()
        dev.set_stream(None, external=False)
        for buf in (d_total, d_blocks, d_starts, d_k5):
            buf.free()
    assert np.array_equal(rec.astype(np.int64).sum(axis=0), total), "the block records sum to the totals"
    peak_at = int(np.argmax(np.hypot(total[:, 0].astype(np.float64), total[:, 1].astype(np.float64)))) - HALF + DELAY
    med = {k: statistics.median(v) for k, v in ms.items()}
    row = {"bench": "fine_vs_copy_and_k5", "device": info["name"], "pair_bytes": 2 * NBYTES, "half_width": HALF, "steps": args.steps,
           "warmup": args.warmup, "peak_lag": peak_at, "k5_lag": k5_lag}
    for k in names:
        row[f"{k}_ms"] = round(med[k], 4)
        row[f"{k}_ms_min"], row[f"{k}_ms_max"] = round(min(ms[k]), 4), round(max(ms[k]), 4)
    row["fine_over_copy"] = round(med["fine"] / med["copy"], 3)
    row["fine_blocks_over_fine"] = round(med["fine_blocks"] / med["fine"], 3)
    row["fine_slice_over_k5"] = round(med["fine_slice"] / med["k5_slice"], 3)
    row["fine_read_gb_s"] = round(2 * NBYTES / med["fine"] / 1e6, 1)
    row["copy_read_plus_write_gb_s"] = round(4 * NBYTES / med["copy"] / 1e6, 1)
    row["fine_gmac_s"] = round(4.0 * n * nl / med["fine"] / 1e6, 1)
    print(json.dumps(row))


if __name__ == "__main__":
    main()
