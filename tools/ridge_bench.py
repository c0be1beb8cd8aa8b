#!/usr/bin/env python3
"""The short-time spectral ridge (gj_ridge_dev) against K2 on one resident capture.

K2 (gj_welch_dev) does the same transforms at the same 50 % overlap and averages them; the ridge reduces every frame
to one 16-byte record instead.  bench.py does not time the ridge, so the figures come from here:

  ridge   gj_ridge_dev at nfft 256 and 1024, hop = nfft / 2, all frames of a 10-s synthetic capture (40 960 000 bytes),
          HIP events around one launch
  k2      gj_welch_timed_dev kernel_ms (the transform launch alone, without the finalize) at the same nperseg, 1-s chunks

The two are interleaved call by call, so that every pair of figures comes from the same moment of the same GPU; every
shape is warmed up first; medians over --steps pairs.  Prints one JSON line.
    python tools/ridge_bench.py [--steps 200] [--warmup 20]"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "gps-jamming_amd"), REPO]
NBYTES = 40960000
FS = 2.048e6
SIZES = (256, 1024)


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
        rows = {}
        for nfft in SIZES:
            hop = nfft // 2
            frames = gpsjam.ridge_frames(NBYTES, 0, nfft, hop)
            d_rec = dev.alloc(frames * gpsjam.RIDGE_DTYPE.itemsize)
            psd_rows = dev.welch_rows(NBYTES, 2048000, nfft)
            d_psd = dev.alloc(4 * psd_rows * nfft)
            dev.reserve(dev.welch_workspace(NBYTES, 2048000, nfft))
            ridge_ms, k2_ms = [], []
            for step in range(args.warmup + args.steps):
                dev.timer_start()
                dev.ridge_dev(cap, NBYTES, 0, nfft, hop, frames, 2, d_rec)
                r = dev.timer_stop()
                k, _ = dev.welch_timed_dev(cap, NBYTES, 2048000, nfft, FS, d_psd)
                if step >= args.warmup:
                    ridge_ms.append(r)
                    k2_ms.append(k)
            r, k = statistics.median(ridge_ms), statistics.median(k2_ms)
            # what the algorithm needs: every frame's 2 N bytes once (the overlap is re-read), 16 bytes out; 5 N log2 N
            # for the transform, 2 N unpack + window, 4 N for |X|^2 and its sum
            read = frames * 2 * nfft
            flop = frames * (5 * nfft * (nfft.bit_length() - 1) + 6 * nfft)
            rows[str(nfft)] = {"frames": frames, "ridge_ms": round(r, 4), "ridge_ms_min": round(min(ridge_ms), 4),
                               "ridge_ms_max": round(max(ridge_ms), 4), "k2_kernel_ms": round(k, 4),
                               "k2_kernel_ms_min": round(min(k2_ms), 4), "k2_kernel_ms_max": round(max(k2_ms), 4),
                               "ridge_over_k2": round(r / k, 3), "ridge_read_gb_s": round(read / r / 1e6, 1),
                               "ridge_gflop_s": round(flop / r / 1e6, 1), "record_bytes": frames * 16}
            d_rec.free()
            d_psd.free()
        cap.free()
        info = dev.info()
    print(json.dumps({"bench": "ridge_vs_k2", "device": info["name"], "capture_bytes": NBYTES, "steps": args.steps,
                      "warmup": args.warmup, "sizes": rows}))


if __name__ == "__main__":
    main()
