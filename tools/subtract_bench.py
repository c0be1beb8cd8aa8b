#!/usr/bin/env python3
"""The counterfeit-signal subtraction (gj_subtract_dev) against a device-to-device copy of the same bytes and against
the correlator bank at the same channels with one tap, on one resident capture.

The subtraction reads every byte of the range once and writes as many: a copy of the same bytes is the floor for any
kernel of that shape.  Per sample and channel it rebuilds what the bank takes apart (a chip, a carrier index, four
multiply-adds), so the bank with one tap at the same channels is its arithmetic yardstick.  bench.py times none of them,
so the figures come from here:

  subtract  gj_subtract_dev over a whole 10-s capture (20 480 000 samples, 40 960 000 bytes), block 256 (what
            gpsjam.spoof.remove runs), dither on, records on, HIP events around the call (one launch): 1, 5, 8, 32 and 64
            channels; also 8 channels without dither and without records
  bank      gj_corr_bank_dev at the same channels, block 256, the prompt tap alone
  copy      torch's device-to-device copy of 40 960 000 bytes between the same events on the same stream

All are interleaved call by call, so that every set of figures comes from the same moment of the same GPU; every shape is
warmed up first; medians, minima and maxima over --steps rounds.  The capture fits the 256 MiB Infinity Cache, for all
alike.  Prints one JSON line.
    python tools/subtract_bench.py [--steps 50] [--warmup 5]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "gps-jamming_amd"), REPO]
NBYTES = 40960000
FS = 2.048e6
B = 256
CHANNELS = (1, 5, 8, 32, 64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import torch
    import gpsjam
    from gpsjam import postcorr
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
        chans = [postcorr.channel((p - 1) % 32, 37.25 * p, -5000.0 + 151.0 * p, FS, 0.01 * p) for p in range(1, 65)]
        d_ch = dev.alloc(64 * 32).upload(np.array(chans, gpsjam.CORR_CHANNEL_DTYPE))
        blocks = gpsjam.corr_blocks(n, B)
        rng = np.random.default_rng(3)
        d_amp = dev.alloc(8 * 64 * blocks).upload(rng.integers(-4000, 4001, (64, blocks, 2)).astype(np.int32))
        d_rec = dev.alloc(24 * gpsjam.subtract_blocks(n))
        d_bank = dev.alloc(8 * 64 * blocks)
        shapes = {f"subtract_{c}ch": ("sub", c, 1, True) for c in CHANNELS}
        shapes["subtract_8ch_no_dither"] = ("sub", 8, 0, True)
        shapes["subtract_8ch_no_records"] = ("sub", 8, 1, False)
        shapes.update({f"bank_{c}ch_1tap": ("bank", c, 0, False) for c in CHANNELS})
        names = ("copy",) + tuple(shapes)
        ms = {name: [] for name in names}
        for step in range(args.warmup + args.steps):
            got = {}
            dev.timer_start()
            out.copy_(cap)
            got["copy"] = dev.timer_stop()
            for name, (kind, n_ch, flags, records) in shapes.items():
                dev.timer_start()
                if kind == "sub":
                    dev.subtract_dev(cap, NBYTES, 0, n, B, d_codes, 32, d_ch, n_ch, d_amp, flags, 7, out, d_rec if records else None)
                else:
                    dev.corr_bank_dev(cap, NBYTES, 0, n, B, d_codes, 32, d_ch, n_ch, (0,), d_bank)
                got[name] = dev.timer_stop()
            if step >= args.warmup:
                for k, v in got.items():
                    ms[k].append(v)
        # the same bytes twice: the launch is deterministic
        dev.subtract_dev(cap, NBYTES, 0, n, B, d_codes, 32, d_ch, 8, d_amp, 1, 7, out, d_rec)
        dev.synchronize()
        first = out[:1 << 20].cpu().numpy().tobytes()
        dev.subtract_dev(cap, NBYTES, 0, n, B, d_codes, 32, d_ch, 8, d_amp, 1, 7, out, d_rec)
        dev.synchronize()
        assert first == out[:1 << 20].cpu().numpy().tobytes()
        info = dev.info()
        dev.set_stream(None, external=False)
        for buf in (d_codes, d_ch, d_amp, d_rec, d_bank):
            buf.free()
    med = {k: statistics.median(v) for k, v in ms.items()}
    row = {"bench": "subtract_vs_copy_and_bank", "device": info["name"], "capture_bytes": NBYTES, "block_samples": B,
           "steps": args.steps, "warmup": args.warmup}
    for k in names:
        row[f"{k}_ms"] = round(med[k], 4)
        row[f"{k}_ms_min"], row[f"{k}_ms_max"] = round(min(ms[k]), 4), round(max(ms[k]), 4)
    row["copy_read_plus_write_gb_s"] = round(2 * NBYTES / med["copy"] / 1e6, 1)
    for c in CHANNELS:
        row[f"subtract_{c}ch_over_copy"] = round(med[f"subtract_{c}ch"] / med["copy"], 2)
        row[f"subtract_{c}ch_over_bank"] = round(med[f"subtract_{c}ch"] / med[f"bank_{c}ch_1tap"], 2)
        row[f"subtract_{c}ch_gsample_channels_s"] = round(n * c / med[f"subtract_{c}ch"] / 1e6, 1)
    row["subtract_5ch_read_plus_write_gb_s"] = round(2 * NBYTES / med["subtract_5ch"] / 1e6, 1)
    print(json.dumps(row))


if __name__ == "__main__":
    main()
