#!/usr/bin/env python3
"""Cross-spectral density (gj_csd_dev) against two spectral kurtoses (gj_sk_dev) on one resident capture pair.

At the same geometry the call reads and transforms exactly what two gj_sk_dev calls, one per capture, read and transform
together; it keeps 64 accumulators per thread against 32, holds one capture's bins while the other is transformed, and
therefore runs at two workgroups per CU where the kurtosis runs at three (nfft < 512).  The expectation this tool
tests: a ratio near 1.  bench.py does not time either, so the figures come from here:

  csd     gj_csd_dev at nfft 256, hop 256, 1024 frame pairs per row, every row of a 10-s synthetic pair
          (2 x 40 960 000 bytes, the second antenna delayed by 4 samples), coherence on, HIP events around the call =
          both launches
  2sk     gj_sk_dev on capture a, then on capture b, same geometry, estimator on, HIP events around the two calls =
          four launches

Both come from the same library and are interleaved call by call, so that every pair of figures comes from the same
moment of the same GPU; both are warmed up first; medians over --steps pairs.  Prints one JSON line.
    python tools/csd_bench.py [--steps 200] [--warmup 20] [--nfft 256]"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "gps-jamming_amd"), REPO]
NBYTES = 40960000
FRAMES_PER_ROW = 1024


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--nfft", type=int, nargs="+", default=[256])
    args = ap.parse_args()
    import gpsjam
    from gpsjam.synth import StreamSpec
    n = NBYTES // 2
    with gpsjam.Device(0) as dev:
        caps = [dev.alloc(NBYTES), dev.alloc(NBYTES)]
        for ant, (cap, delay) in enumerate(zip(caps, (0, 4))):
            dev.synth_dev(StreamSpec(seed=9, antenna=ant, delay=delay, jam_start=n // 2, jam_end=1 << 40, jam_sigma=50.0), n, cap)
        rows = {}
        for nfft in args.nfft:
            n_rows = gpsjam.csd_rows(NBYTES, 0, NBYTES, 0, nfft, nfft, FRAMES_PER_ROW)
            cells = n_rows * nfft
            d_csd = dev.alloc(5 * 4 * cells)
            d_sk = dev.alloc(6 * 4 * cells)
            ws = dev.csd_workspace(nfft, FRAMES_PER_ROW, n_rows)
            dev.reserve(max(ws, dev.sk_workspace(nfft, FRAMES_PER_ROW, n_rows)))
            csd_ms, sk_ms = [], []
            for step in range(args.warmup + args.steps):
                dev.timer_start()
                dev.cross_spectrum_dev(caps[0], NBYTES, 0, caps[1], NBYTES, 0, nfft, nfft, FRAMES_PER_ROW, n_rows,
                                       d_csd.ptr + 8 * cells, d_csd.ptr + 12 * cells, d_csd.ptr, d_csd.ptr + 16 * cells)
                c = dev.timer_stop()
                dev.timer_start()
                for k, cap in enumerate(caps):
                    at = d_sk.ptr + 12 * cells * k
                    dev.spectral_kurtosis_dev(cap, NBYTES, 0, nfft, nfft, FRAMES_PER_ROW, n_rows, at, at + 4 * cells, at + 8 * cells)
                s = dev.timer_stop()
                if step >= args.warmup:
                    csd_ms.append(c)
                    sk_ms.append(s)
            c, s = statistics.median(csd_ms), statistics.median(sk_ms)
            pairs = n_rows * FRAMES_PER_ROW
            read = 2 * pairs * 2 * nfft
            rows[str(nfft)] = {"rows": n_rows, "frame_pairs": pairs, "csd_ms": round(c, 4), "csd_ms_min": round(min(csd_ms), 4),
                               "csd_ms_max": round(max(csd_ms), 4), "two_sk_ms": round(s, 4), "two_sk_ms_min": round(min(sk_ms), 4),
                               "two_sk_ms_max": round(max(sk_ms), 4), "csd_over_two_sk": round(c / s, 3),
                               "csd_read_gb_s": round(read / c / 1e6, 1), "workspace_bytes": ws}
            d_csd.free()
            d_sk.free()
        for cap in caps:
            cap.free()
        info = dev.info()
    print(json.dumps({"bench": "csd_vs_two_skurt", "device": info["name"], "capture_bytes": NBYTES, "frames_per_row": FRAMES_PER_ROW,
                      "steps": args.steps, "warmup": args.warmup, "sizes": rows}))


if __name__ == "__main__":
    main()
