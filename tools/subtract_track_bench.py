#!/usr/bin/env python3
"""The subtraction of tracked signals (gj_subtract_track_dev) against gj_subtract_dev on the same bytes and against a
device-to-device copy of them, on one resident capture.

Both kernels read every byte of the range once and write as many; per sample and channel both rebuild a chip, a carrier
index and four multiply-adds.  The tracked one takes its NCOs from one 56-byte record per channel and epoch instead of
one channel per call, and a thread's run may be cut by an epoch boundary.  bench.py times neither, so the figures come
from here:

  track     gj_subtract_track_dev over a whole 10-s capture (20 480 000 samples, 40 960 000 bytes), epochs of 2048
            samples (what gpsjam.track.follow runs at 2.048 MS/s), dither on, records on, HIP events around the call (one
            launch): 5 and 64 channels whose records are one constant channel advanced by 2048 samples per epoch, start 0
  subtract  gj_subtract_dev with those constant channels, block 2048, the same amplitudes: it writes the same bytes, which
            a SHA-256 of both outputs checks before anything is timed
  cut       gj_subtract_track_dev with the same records from starts 1000 + 37 k, no multiple of 16: every epoch boundary
            cuts a thread's run, the case of a real acquisition's code index (its bytes are others: one epoch less)
  copy      torch's device-to-device copy of 40 960 000 bytes between the same events on the same stream

All are interleaved call by call, so that every set of figures comes from the same moment of the same GPU; every shape is
warmed up first; medians, minima and maxima over --steps rounds.  The capture fits the 256 MiB Infinity Cache, for all
alike.  Prints one JSON line.
    python tools/subtract_track_bench.py [--steps 50] [--warmup 5]"""
import argparse
import hashlib
import json
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "gps-jamming_amd"), REPO]
NBYTES = 40960000
FS = 2.048e6
B = 2048
CHANNELS = (5, 64)
PERIOD = 1023 << 32


def advanced(chans, n_epochs, dtype):
    """dtype[len(chans)][n_epochs]: every channel advanced by m B samples per epoch (exact: m B step < 2^63)."""
    rec = np.zeros((len(chans), n_epochs), dtype)
    m = np.arange(n_epochs, dtype=np.uint64) * np.uint64(B)
    for k, ch in enumerate(chans):
        rec["code_phase"][k] = (np.uint64(ch.code_phase) + m * np.uint64(ch.code_step)) % np.uint64(PERIOD)
        rec["code_step"][k] = ch.code_step
        rec["carr_phase"][k] = (np.uint64(ch.carr_phase) + m * np.uint64(ch.carr_step)) & np.uint64(0xFFFFFFFF)
        rec["carr_step"][k] = ch.carr_step
    return rec


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
    E = n // B
    assert E * B == n
    with gpsjam.Device(0) as dev:
        dev.set_stream(torch.cuda.current_stream().cuda_stream)
        cap = torch.empty(NBYTES, dtype=torch.uint8, device="cuda")
        out = torch.empty(NBYTES, dtype=torch.uint8, device="cuda")
        dev.synth_dev(StreamSpec(seed=9, antenna=0, delay=0, jam_start=1 << 40, jam_end=1 << 40, jam_sigma=0.0), n, cap)
        rows = postcorr.codes(list(range(1, 33)))
        d_codes = dev.alloc(rows.nbytes).upload(rows)
        chans = [postcorr.channel((p - 1) % 32, 37.25 * p, -5000.0 + 151.0 * p, FS, 0.01 * p) for p in range(1, 65)]
        d_ch = dev.alloc(64 * 32).upload(np.array(chans, gpsjam.CORR_CHANNEL_DTYPE))
        d_tab = dev.alloc(64 * 8).upload(np.array([(0, c.code_row) for c in chans], gpsjam.SUB_TRACK_CHANNEL_DTYPE))
        d_cut = dev.alloc(64 * 8).upload(np.array([(1000 + 37 * k, c.code_row) for k, c in enumerate(chans)], gpsjam.SUB_TRACK_CHANNEL_DTYPE))
        d_epochs = dev.alloc(56 * 64 * E).upload(advanced(chans, E, gpsjam.TRACK_EPOCH_DTYPE).reshape(-1))
        rng = np.random.default_rng(3)
        d_amp = dev.alloc(8 * 64 * E).upload(rng.integers(-4000, 4001, (64, E, 2)).astype(np.int32))
        d_rec = dev.alloc(24 * gpsjam.subtract_blocks(n))

        def call(kind, n_ch):
            if kind == "subtract":
                dev.subtract_dev(cap, NBYTES, 0, n, B, d_codes, 32, d_ch, n_ch, d_amp, 1, 7, out, d_rec)
            elif kind == "track":
                dev.subtract_track_dev(cap, NBYTES, 0, n, B, E, d_codes, 32, d_tab, n_ch, d_epochs, d_amp, 1, 7, out, d_rec)
            else:   # the last epoch would run past the range from these starts
                dev.subtract_track_dev(cap, NBYTES, 0, n, B, E - 2, d_codes, 32, d_cut, n_ch, d_epochs, d_amp, 1, 7, out, d_rec)

        def digest():
            dev.synchronize()
            return hashlib.sha256(out.cpu().numpy().tobytes() + d_rec.download(np.uint8).tobytes()).hexdigest()

        digests = {}
        for c in CHANNELS:   # the amplitude and record rows of channel k are at k * E in both layouts: the first c channels are the same
            call("subtract", c)
            want = digest()
            out.zero_()
            call("track", c)
            digests[c] = digest()
            assert digests[c] == want, f"{c} channels: gj_subtract_track_dev and gj_subtract_dev wrote other bytes"
        shapes = {f"{kind}_{c}ch": (kind, c) for c in CHANNELS for kind in ("subtract", "track", "cut")}
        names = ("copy",) + tuple(shapes)
        ms = {name: [] for name in names}
        for step in range(args.warmup + args.steps):
            got = {}
            dev.timer_start()
            out.copy_(cap)
            got["copy"] = dev.timer_stop()
            for name, (kind, n_ch) in shapes.items():
                dev.timer_start()
                call(kind, n_ch)
                got[name] = dev.timer_stop()
            if step >= args.warmup:
                for k, v in got.items():
                    ms[k].append(v)
        info = dev.info()
        dev.set_stream(None, external=False)
        for buf in (d_codes, d_ch, d_tab, d_cut, d_epochs, d_amp, d_rec):
            buf.free()
    med = {k: statistics.median(v) for k, v in ms.items()}
    row = {"bench": "subtract_track_vs_subtract_and_copy", "device": info["name"], "capture_bytes": NBYTES, "block_samples": B,
           "n_epochs": E, "steps": args.steps, "warmup": args.warmup, "same_bytes_as_subtract": True}
    for k in names:
        row[f"{k}_ms"] = round(med[k], 4)
        row[f"{k}_ms_min"], row[f"{k}_ms_max"] = round(min(ms[k]), 4), round(max(ms[k]), 4)
    row["copy_read_plus_write_gb_s"] = round(2 * NBYTES / med["copy"] / 1e6, 1)
    for c in CHANNELS:
        row[f"track_{c}ch_over_subtract"] = round(med[f"track_{c}ch"] / med[f"subtract_{c}ch"], 2)
        row[f"cut_{c}ch_over_subtract"] = round(med[f"cut_{c}ch"] / med[f"subtract_{c}ch"], 2)
        row[f"track_{c}ch_over_copy"] = round(med[f"track_{c}ch"] / med["copy"], 2)
        row[f"track_{c}ch_gsample_channels_s"] = round(n * c / med[f"track_{c}ch"] / 1e6, 1)
        row[f"sha256_{c}ch"] = digests[c][:16]
    print(json.dumps(row))


if __name__ == "__main__":
    main()
