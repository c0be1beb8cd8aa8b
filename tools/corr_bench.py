#!/usr/bin/env python3
"""The correlator bank (gj_corr_bank_dev) against a device-to-device copy and against the acquisition series on one
resident capture.

The bank reads every byte of the range once and writes next to nothing: a copy that reads as many bytes is the floor for
any kernel of that shape (it also writes them, which the bank does not).  AcqSearch.series over the same capture is what
the library knew of a satellite before, for scale.  bench.py times none of them, so the figures come from here:

  bank     gj_corr_bank_dev over a whole 10-s capture (20 480 000 samples, 40 960 000 bytes): 8 channels x 3 taps,
           block 2048, HIP events around the call (one launch); also 1 channel and 32 channels, and block 256 (what
           gpsjam.postcorr.observe runs)
  copy     torch's device-to-device copy of 40 960 000 bytes between the same events on the same stream
  series   AcqSearch.series of the same 8 PRNs over the same capture at its defaults (one search per 0.1 s), once

bank and copy are interleaved call by call, so that every set of figures comes from the same moment of the same GPU; every
shape is warmed up first; medians, minima and maxima over --steps rounds.  The capture fits the 256 MiB Infinity Cache,
for both alike.  Prints one JSON line.
    python tools/corr_bench.py [--steps 100] [--warmup 10]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "gps-jamming_amd"), REPO]
NBYTES = 40960000
PRNS = (2, 5, 9, 12, 17, 21, 25, 30)
TAPS = (0, -1, 1)
FS = 2.048e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    import torch
    import gpsjam
    from gpsjam import gnss, postcorr
    from gpsjam.synth import StreamSpec
    n = NBYTES // 2
    with gpsjam.Device(0) as dev:
        dev.set_stream(torch.cuda.current_stream().cuda_stream)
        cap = torch.empty(NBYTES, dtype=torch.uint8, device="cuda")
        out = torch.empty(NBYTES, dtype=torch.uint8, device="cuda")
        dev.synth_dev(StreamSpec(seed=9, antenna=0, delay=0, jam_start=1 << 40, jam_end=1 << 40, jam_sigma=0.0), n, cap)
        all_prns = list(range(1, 33))
        rows = postcorr.codes(all_prns)
        d_codes = dev.alloc(rows.nbytes).upload(rows)
        chans = [postcorr.channel(p - 1, 37.25 * p, -5000.0 + 311.0 * p, FS, 0.01 * p) for p in all_prns]
        eight = np.array([chans[p - 1] for p in PRNS], gpsjam.CORR_CHANNEL_DTYPE)
        d_eight = dev.alloc(eight.nbytes).upload(eight)
        d_all = dev.alloc(32 * 32).upload(np.array(chans, gpsjam.CORR_CHANNEL_DTYPE))
        d_out = dev.alloc(8 * 32 * gpsjam.corr_blocks(n, 256) * 3)
        shapes = {"bank_8ch_3taps_b2048": (d_eight, 8, 2048, TAPS), "bank_1ch_3taps_b2048": (d_eight, 1, 2048, TAPS),
                  "bank_32ch_3taps_b2048": (d_all, 32, 2048, TAPS), "bank_8ch_3taps_b256": (d_eight, 8, 256, TAPS),
                  "bank_8ch_9taps_b2048": (d_eight, 8, 2048, (0, -1, 1, -2, 2, -3, 3, -4, 4))}
        names = ("copy",) + tuple(shapes)
        ms = {name: [] for name in names}
        for step in range(args.warmup + args.steps):
            got = {}
            dev.timer_start()
            out.copy_(cap)
            got["copy"] = dev.timer_stop()
            for name, (d_ch, n_ch, B, taps) in shapes.items():
                dev.timer_start()
                dev.corr_bank_dev(cap, NBYTES, 0, n, B, d_codes, 32, d_ch, n_ch, taps, d_out)
                got[name] = dev.timer_stop()
            if step >= args.warmup:
                for k, v in got.items():
                    ms[k].append(v)
        # the same records twice: the launch is deterministic
        dev.corr_bank_dev(cap, NBYTES, 0, n, 2048, d_codes, 32, d_eight, 8, TAPS, d_out)
        first = d_out.download(np.int32, 2 * 8 * 10000 * 3)
        dev.corr_bank_dev(cap, NBYTES, 0, n, 2048, d_codes, 32, d_eight, 8, TAPS, d_out)
        assert first.tobytes() == d_out.download(np.int32, 2 * 8 * 10000 * 3).tobytes()
        search = gnss.AcqSearch(dev, prns=list(PRNS))
        search.series(cap)                                       # warm-up: the workspace grows here
        series = search.series(cap)
        series_ms, epochs = dev.last_kernel_ms, series.n_epochs
        search.close()
        info = dev.info()
        dev.set_stream(None, external=False)
        for buf in (d_codes, d_eight, d_all, d_out):
            buf.free()
    med = {k: statistics.median(v) for k, v in ms.items()}
    row = {"bench": "corr_bank_vs_copy_and_series", "device": info["name"], "capture_bytes": NBYTES, "steps": args.steps,
           "warmup": args.warmup}
    for k in names:
        row[f"{k}_ms"] = round(med[k], 4)
        row[f"{k}_ms_min"], row[f"{k}_ms_max"] = round(min(ms[k]), 4), round(max(ms[k]), 4)
    row["bank_over_copy"] = round(med["bank_8ch_3taps_b2048"] / med["copy"], 2)
    row["bank_read_gb_s"] = round(NBYTES / med["bank_8ch_3taps_b2048"] / 1e6, 1)
    row["copy_read_plus_write_gb_s"] = round(2 * NBYTES / med["copy"] / 1e6, 1)
    row["bank_gsample_channel_taps_s"] = round(n * 8 * 3 / med["bank_8ch_3taps_b2048"] / 1e6, 1)
    row["acq_series_ms"], row["acq_series_epochs"] = round(series_ms, 3), epochs
    print(json.dumps(row))


if __name__ == "__main__":
    main()
