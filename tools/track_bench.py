#!/usr/bin/env python3
"""The tracking loops (gj_track_dev) against the correlator bank (gj_corr_bank_dev) over the same range of one resident
capture.

The bank makes the same three sums per channel and block open loop, every block at once; the loops make them one epoch
after the other, each epoch behind the update of the one before.  The ratio of the two is what closing the loop costs.
bench.py times neither, so the figures come from here:

  track    gj_track_dev over a whole 10-s capture (20 480 000 samples, 40 960 000 bytes): 10 000 epochs of 2048 samples
           per channel, spacing 1, the WIDE gains, aid_div 1540, at 1, 8 and 64 channels (one workgroup each); the
           states are put back in front of every call, outside the timed region; HIP events around the call (one launch)
  bank     gj_corr_bank_dev over the same range with the same channels at the taps (+1, 0, -1), block 2048

track and bank are interleaved call by call, so that every set of figures comes from the same moment of the same GPU;
every shape is warmed up first; medians, minima and maxima over --steps rounds.  The capture fits the 256 MiB Infinity
Cache, for both alike.  Prints one JSON line.
    python tools/track_bench.py [--steps 20] [--warmup 3]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "gps-jamming_amd"), REPO]
NBYTES = 40960000
B = 2048
FS = 2.048e6
COUNTS = (1, 8, 64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch
    import gpsjam
    from gpsjam import postcorr, track
    from gpsjam.synth import StreamSpec
    n = NBYTES // 2
    n_epochs = n // B
    with gpsjam.Device(0) as dev:
        dev.set_stream(torch.cuda.current_stream().cuda_stream)
        cap = torch.empty(NBYTES, dtype=torch.uint8, device="cuda")
        dev.synth_dev(StreamSpec(seed=9, antenna=0, delay=0, jam_start=1 << 40, jam_end=1 << 40, jam_sigma=0.0), n, cap)
        all_prns = list(range(1, 33))
        rows = postcorr.codes(all_prns)
        d_codes = dev.alloc(rows.nbytes).upload(rows)
        chans = [postcorr.channel(k % 32, 37.25 * k, -5000.0 + 155.0 * k, FS, 0.01 * k) for k in range(max(COUNTS))]
        states = np.zeros(len(chans), gpsjam.TRACK_STATE_DTYPE)
        states["ch"] = np.array(chans, gpsjam.CORR_CHANNEL_DTYPE)
        d_ch = dev.alloc(32 * len(chans)).upload(states["ch"])
        d_st = dev.alloc(states.nbytes)
        d_rec = dev.alloc(gpsjam.TRACK_EPOCH_DTYPE.itemsize * len(chans) * n_epochs)
        d_bank = dev.alloc(8 * len(chans) * n_epochs * 3)
        params = track.gains(*track.WIDE, B, FS)
        ms = {f"{kind}_{c}ch": [] for c in COUNTS for kind in ("track", "bank")}
        for step in range(args.warmup + args.steps):
            for c in COUNTS:
                d_st.upload(states)
                dev.timer_start()
                dev.track_dev(cap, NBYTES, 0, n, B, n_epochs, d_codes, 32, d_st, c, params, d_rec)
                t = dev.timer_stop()
                dev.timer_start()
                dev.corr_bank_dev(cap, NBYTES, 0, n, B, d_codes, 32, d_ch, c, (1, 0, -1), d_bank)
                b = dev.timer_stop()
                if step >= args.warmup:
                    ms[f"track_{c}ch"].append(t)
                    ms[f"bank_{c}ch"].append(b)
        # the same records twice: the launch is deterministic
        d_st.upload(states)
        dev.track_dev(cap, NBYTES, 0, n, B, 100, d_codes, 32, d_st, 8, params, d_rec)
        first = d_rec.download(np.uint8, 56 * 100)
        d_st.upload(states)
        dev.track_dev(cap, NBYTES, 0, n, B, 100, d_codes, 32, d_st, 8, params, d_rec)
        assert first.tobytes() == d_rec.download(np.uint8, 56 * 100).tobytes()
        info = dev.info()
        dev.set_stream(None, external=False)
        for buf in (d_codes, d_ch, d_st, d_rec, d_bank):
            buf.free()
    row = {"bench": "track_vs_corr_bank", "device": info["name"], "capture_bytes": NBYTES, "block_samples": B, "epochs": n_epochs,
           "steps": args.steps, "warmup": args.warmup}
    for k, v in ms.items():
        row[f"{k}_ms"] = round(statistics.median(v), 4)
        row[f"{k}_ms_min"], row[f"{k}_ms_max"] = round(min(v), 4), round(max(v), 4)
    for c in COUNTS:
        row[f"track_{c}ch_us_per_epoch"] = round(1e3 * statistics.median(ms[f"track_{c}ch"]) / n_epochs, 3)
        row[f"track_over_bank_{c}ch"] = round(statistics.median(ms[f"track_{c}ch"]) / statistics.median(ms[f"bank_{c}ch"]), 1)
    print(json.dumps(row))


if __name__ == "__main__":
    main()
