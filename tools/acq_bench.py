#!/usr/bin/env python3
"""Time of one cold acquisition search (32 PRNs x 71 Doppler bins x 10 ms) on a quiet capture: nothing acquires, so
every PRN runs all ten integration steps (the worst case).  HIP events around 20 searches.

--series: the acquisition series over 100 epochs at nsamp 2048 (gj_acq_series_dev, one call, stride 0.1 s) against
the host loop of 100 gj_acq_search_dev calls it replaces, interleaved on one GPU (--reps rounds of each)."""
import argparse
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gps-jamming_amd"))


def cold_search(dev, cap):
    from gpsjam.gnss import AcqSearch
    for fs in (2.048e6, 1.024e6):
        srch = AcqSearch(dev, fs=fs)
        for _ in range(5):
            srch.search_dev(cap, cap.nbytes, 0)
        dev.synchronize()
        reps = 20
        dev.timer_start()
        for _ in range(reps):
            srch.search_dev(cap, cap.nbytes, 0)
        ms = dev.timer_stop() / reps
        n_fft = len(srch.prns) * len(srch.freqs) * srch.intg + len(srch.freqs) * srch.intg + len(srch.prns)
        found = sum(r.acquired for r in srch.results())
        print(f"fs {fs / 1e6:.3f} MS/s (FFT {2 * srch.nsamp}): {ms:.3f} ms per search, {n_fft / ms / 1e3:.1f} M transforms/s, "
              f"{found} false acquisitions", flush=True)
        srch.close()


def series_vs_loop(dev, cap, n_epochs, reps, epochs_per_launch):
    import numpy as np
    from gpsjam.gnss import AcqSearch, _AcqStruct
    srch = AcqSearch(dev)
    stride = int(0.1 * srch.fs)
    dev.reserve(srch.series_workspace(n_epochs, epochs_per_launch))
    d_out = dev.alloc(C.sizeof(_AcqStruct) * n_epochs * len(srch.prns))

    def series():
        srch.series_dev(cap, cap.nbytes, 0, stride, n_epochs, d_out, epochs_per_launch)

    def loop():
        for e in range(n_epochs):
            srch.search_dev(cap, cap.nbytes, e * stride)

    runs = {"series": series, "loop": loop}
    for f in runs.values():                               # warm-up: code objects, workspace, caches
        f()
    dev.synchronize()
    times = {k: [] for k in runs}
    for _ in range(reps):
        for name, f in runs.items():
            dev.timer_start()
            f()
            times[name].append(dev.timer_stop())
    for name in runs:
        t = np.array(times[name])
        print(f"{name:6s} {n_epochs} epochs (nsamp {srch.nsamp}, 32 PRNs x 71 bins x 10 ms): median {np.median(t):.3f} ms "
              f"[min {t.min():.3f}, max {t.max():.3f}] = {np.median(t) / n_epochs:.4f} ms per epoch", flush=True)
    print(f"speed-up of the series over the loop: {np.median(times['loop']) / np.median(times['series']):.2f}x", flush=True)
    d_out.free()
    srch.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--series", action="store_true")
    ap.add_argument("--epochs", type=int, default=100)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--epochs-per-launch", type=int, default=0)
    a = ap.parse_args()
    import numpy as np
    import gpsjam
    dev = gpsjam.Device(0)
    rng = np.random.RandomState(3)
    n = 2048 * 64 if not a.series else 204800 * (a.epochs - 1) + 11 * 2048
    raw = np.clip(np.rint(rng.normal(0.0, 6.25, 2 * n)), -128, 127).astype(np.int16) + 128
    cap = dev.capture(raw.astype(np.uint8))
    if a.series:
        series_vs_loop(dev, cap, a.epochs, a.reps, a.epochs_per_launch)
    else:
        cold_search(dev, cap)


if __name__ == "__main__":
    main()
