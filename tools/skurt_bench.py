#!/usr/bin/env python3
"""Spectral kurtosis (gj_sk_dev) against K2 on one resident capture.

At hop = nfft the kurtosis kernel reads every byte once and runs HALF of K2's transforms (K2 overlaps by 50 %); it
keeps 32 accumulators per thread more, writes one partial pair per block of 16 frames and adds them in a second launch.
The expectation this tool tests: it is not slower than K2 at the same transform size.  bench.py does not time it, so
the figures come from here:

  sk      gj_sk_dev at nfft 256, 1024 and 4096, hop = nfft, 256 frames per row, every row of a 10-s synthetic capture
          (40 960 000 bytes), estimator on, HIP events around the call = both launches
  k2      gj_welch_timed_dev kernel_ms + finalize_ms (both launches too) at the same nperseg, 1-s chunks

The two are interleaved call by call, so that every pair of figures comes from the same moment of the same GPU; every
shape is warmed up first; medians over --steps pairs.  Prints one JSON line.
    python tools/skurt_bench.py [--steps 200] [--warmup 20]"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "gps-jamming_amd"), REPO]
NBYTES = 40960000
FS = 2.048e6
SIZES = (256, 1024, 4096)
FRAMES_PER_ROW = 256


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
            n_rows = gpsjam.sk_rows(NBYTES, 0, nfft, nfft, FRAMES_PER_ROW)
            d_out = dev.alloc(3 * 4 * n_rows * nfft)
            d_s1, d_s2, d_sk = d_out.ptr, d_out.ptr + 4 * n_rows * nfft, d_out.ptr + 8 * n_rows * nfft
            psd_rows = dev.welch_rows(NBYTES, 2048000, nfft)
            d_psd = dev.alloc(4 * psd_rows * nfft)
            ws = dev.sk_workspace(nfft, FRAMES_PER_ROW, n_rows)
            dev.reserve(max(dev.welch_workspace(NBYTES, 2048000, nfft), ws))
            sk_ms, k2_ms, k2_kernel_ms = [], [], []
            for step in range(args.warmup + args.steps):
                dev.timer_start()
                dev.spectral_kurtosis_dev(cap, NBYTES, 0, nfft, nfft, FRAMES_PER_ROW, n_rows, d_s1, d_s2, d_sk)
                s = dev.timer_stop()
                k, fin = dev.welch_timed_dev(cap, NBYTES, 2048000, nfft, FS, d_psd)
                if step >= args.warmup:
                    sk_ms.append(s)
                    k2_ms.append(k + fin)
                    k2_kernel_ms.append(k)
            s, k = statistics.median(sk_ms), statistics.median(k2_ms)
            # what the algorithm needs: every byte once, a partial pair written and read back, three float32 per cell
            # out; 5 N log2 N for the transform, 2 N unpack + window, 3 N for |X|^2, 3 N for the two sums
            frames = n_rows * FRAMES_PER_ROW
            read = frames * 2 * nfft
            flop = frames * (5 * nfft * (nfft.bit_length() - 1) + 8 * nfft)
            rows[str(nfft)] = {"rows": n_rows, "frames": frames, "sk_ms": round(s, 4), "sk_ms_min": round(min(sk_ms), 4),
                               "sk_ms_max": round(max(sk_ms), 4), "k2_ms": round(k, 4), "k2_ms_min": round(min(k2_ms), 4),
                               "k2_ms_max": round(max(k2_ms), 4), "k2_kernel_ms": round(statistics.median(k2_kernel_ms), 4),
                               "sk_over_k2": round(s / k, 3), "sk_read_gb_s": round(read / s / 1e6, 1),
                               "sk_gflop_s": round(flop / s / 1e6, 1), "workspace_bytes": ws}
            d_out.free()
            d_psd.free()
        cap.free()
        info = dev.info()
    print(json.dumps({"bench": "skurt_vs_k2", "device": info["name"], "capture_bytes": NBYTES, "frames_per_row": FRAMES_PER_ROW,
                      "steps": args.steps, "warmup": args.warmup, "sizes": rows}))


if __name__ == "__main__":
    main()
