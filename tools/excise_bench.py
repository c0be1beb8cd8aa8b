#!/usr/bin/env python3
"""The frequency-domain excisor (gj_excise_dev) against K2 on one resident capture.

K2 (gj_welch_dev) does one forward transform per frame at the same 50 % overlap and averages the spectra; the excisor
does the forward transform, the mask, a second transform back and writes a byte per byte read.  From the code alone
that is roughly twice K2's time.  bench.py does not time the excisor, so the figures come from here:

  excise  gj_excise_dev at nfft 256, 1024 and 4096 over a whole 10-s synthetic capture (40 960 000 bytes), a flat
          threshold 16 x the noise floor, frame records on, HIP events around the call (both launches)
  k2      gj_welch_timed_dev kernel_ms (the transform launch alone, without the finalize) at the same nperseg, 1-s chunks

The two are interleaved call by call, so that every pair of figures comes from the same moment of the same GPU; every
shape is warmed up first; medians over --steps pairs.  Prints one JSON line.
    python tools/excise_bench.py [--steps 200] [--warmup 20]"""
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
SIZES = (256, 1024, 4096)
NOISE_SIGMA = 6.25


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    import gpsjam
    from gpsjam.synth import StreamSpec
    n = NBYTES // 2
    with gpsjam.Device(0) as dev:
        cap = dev.alloc(NBYTES)
        dev.synth_dev(StreamSpec(seed=9, antenna=0, delay=0, jam_start=n // 2, jam_end=1 << 40, jam_sigma=50.0), n, cap)
        d_out = dev.alloc(NBYTES)
        rows = {}
        for nfft in SIZES:
            frames = gpsjam.excise_frames(n, nfft)
            floor = 0.375 * nfft * 2.0 * NOISE_SIGMA ** 2 / 127.5 ** 2
            d_thr = dev.alloc(4 * nfft).upload(np.full(nfft, 16.0 * floor, np.float32))
            d_rec = dev.alloc(frames * gpsjam.EXCISE_DTYPE.itemsize)
            psd_rows = dev.welch_rows(NBYTES, 2048000, nfft)
            d_psd = dev.alloc(4 * psd_rows * nfft)
            dev.reserve(dev.welch_workspace(NBYTES, 2048000, nfft))
            ex_ms, k2_ms = [], []
            for step in range(args.warmup + args.steps):
                dev.timer_start()
                dev.excise_dev(cap, NBYTES, 0, n, nfft, d_thr, d_out, d_rec)
                e = dev.timer_stop()
                k, _ = dev.welch_timed_dev(cap, NBYTES, 2048000, nfft, FS, d_psd)
                if step >= args.warmup:
                    ex_ms.append(e)
                    k2_ms.append(k)
            e, k = statistics.median(ex_ms), statistics.median(k2_ms)
            rec = d_rec.download(gpsjam.EXCISE_DTYPE, frames)
            # what the algorithm needs: every frame's 2 N bytes once (the overlap is re-read), N bytes out per frame;
            # two transforms of 5 N log2 N, 2 N unpack + window, 4 N for |X|^2 and the mask, 4 N overlap-add and rounding
            flop = frames * (10 * nfft * (nfft.bit_length() - 1) + 10 * nfft)
            rows[str(nfft)] = {"frames": frames, "excise_ms": round(e, 4), "excise_ms_min": round(min(ex_ms), 4),
                               "excise_ms_max": round(max(ex_ms), 4), "k2_kernel_ms": round(k, 4),
                               "k2_kernel_ms_min": round(min(k2_ms), 4), "k2_kernel_ms_max": round(max(k2_ms), 4),
                               "excise_over_k2": round(e / k, 3), "excise_read_gb_s": round(frames * 2 * nfft / e / 1e6, 1),
                               "excise_write_gb_s": round(NBYTES / e / 1e6, 1), "excise_gflop_s": round(flop / e / 1e6, 1),
                               "bins_excised": round(float(rec["n_excised"].mean()) / nfft, 4)}
            for b in (d_thr, d_rec, d_psd):
                b.free()
        cap.free()
        d_out.free()
        info = dev.info()
    print(json.dumps({"bench": "excise_vs_k2", "device": info["name"], "capture_bytes": NBYTES, "steps": args.steps,
                      "warmup": args.warmup, "sizes": rows}))


if __name__ == "__main__":
    main()
