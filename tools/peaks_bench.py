#!/usr/bin/env python3
"""The K-peak search (gj_acq_peaks_dev) against a device-to-device copy of its input, and AcqSearch.peaks against
AcqSearch.search on one resident capture.

The kernel reads every cell of the surface once and writes next to nothing: a copy that reads as many bytes is the floor
for any kernel of that shape (it also writes them, which the search does not).  bench.py times none of this, so the
figures come from here:

  peaks    gj_acq_peaks_dev over double[32][71][2048] (37 224 448 bytes): k = 2, guard = 4, HIP events around the call
           (two launches); also k = 1 and k = 8, one PRN, and nsamp 512
  copy     torch's device-to-device copy of the same 37 224 448 bytes between the same events on the same stream
  search   AcqSearch.search (32 PRNs, one peak each, early stop) and AcqSearch.peaks (the same search to the last step
           with the surface in memory, then the kernel) on a synthetic capture: whole calls, HIP events inside them

peaks and copy are interleaved call by call, so that every set of figures comes from the same moment of the same GPU;
every shape is warmed up first; medians, minima and maxima over --steps rounds.  The surface fits the 256 MiB Infinity
Cache, for both alike.  Prints one JSON line.
    python tools/peaks_bench.py [--steps 100] [--warmup 10]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "gps-jamming_amd"), REPO]
N_PRN, N_FREQ, NSAMP = 32, 71, 2048


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    import torch
    import gpsjam
    from gpsjam import gnss
    from gpsjam.synth import StreamSpec
    cells = N_PRN * N_FREQ * NSAMP
    with gpsjam.Device(0) as dev:
        dev.set_stream(torch.cuda.current_stream().cuda_stream)
        surface = torch.from_numpy(np.random.default_rng(5).gamma(10.0, 1.0, cells)).cuda()
        out = torch.empty_like(surface)
        d_peaks, d_floor = dev.alloc(16 * N_PRN * 8), dev.alloc(16 * N_PRN)
        dev.reserve(dev.acq_peaks_workspace(NSAMP, N_PRN))
        shapes = {"peaks_k2": (N_PRN, N_FREQ, NSAMP, 2, 4), "peaks_k1": (N_PRN, N_FREQ, NSAMP, 1, 4),
                  "peaks_k8": (N_PRN, N_FREQ, NSAMP, 8, 4), "peaks_k2_one_prn": (1, N_FREQ, NSAMP, 2, 4),
                  "peaks_k2_nsamp512": (N_PRN, N_FREQ, 512, 2, 4)}
        names = ("copy",) + tuple(shapes)
        ms = {name: [] for name in names}
        for step in range(args.warmup + args.steps):
            got = {}
            dev.timer_start()
            out.copy_(surface)
            got["copy"] = dev.timer_stop()
            for name, (n_prn, n_freq, nsamp, k, guard) in shapes.items():
                dev.timer_start()
                dev.acq_peaks_dev(surface, n_prn, n_freq, nsamp, k, guard, d_peaks, d_floor)
                got[name] = dev.timer_stop()
            if step >= args.warmup:
                for key, v in got.items():
                    ms[key].append(v)
        # the same records twice: the launches are deterministic
        dev.acq_peaks_dev(surface, N_PRN, N_FREQ, NSAMP, 8, 4, d_peaks, d_floor)
        first = d_peaks.download(np.uint8).tobytes() + d_floor.download(np.uint8).tobytes()
        dev.acq_peaks_dev(surface, N_PRN, N_FREQ, NSAMP, 8, 4, d_peaks, d_floor)
        assert first == d_peaks.download(np.uint8).tobytes() + d_floor.download(np.uint8).tobytes()
        # the whole calls, on a capture with no satellite in it (no PRN stops early: both integrate all steps)
        search = gnss.AcqSearch(dev)
        n = search.samples_needed()
        cap = torch.empty(2 * n, dtype=torch.uint8, device="cuda")
        dev.synth_dev(StreamSpec(seed=9, antenna=0, delay=0, jam_start=1 << 40, jam_end=1 << 40, jam_sigma=0.0), n, cap)
        whole = {"search": [], "search_with_power": [], "search_peaks": []}
        for step in range(3 + 10):
            search.search(cap)
            a = dev.last_kernel_ms
            search.search(cap, want_power=True)
            b = dev.last_kernel_ms
            search.peaks(cap)
            c = dev.last_kernel_ms
            if step >= 3:
                whole["search"].append(a), whole["search_with_power"].append(b), whole["search_peaks"].append(c)
        search.close()
        info = dev.info()
        dev.set_stream(None, external=False)
        d_peaks.free(), d_floor.free()
    med = {k: statistics.median(v) for k, v in ms.items()}
    row = {"bench": "acq_peaks_vs_copy_and_search", "device": info["name"], "surface_bytes": 8 * cells, "steps": args.steps,
           "warmup": args.warmup}
    for k in names:
        row[f"{k}_ms"] = round(med[k], 4)
        row[f"{k}_ms_min"], row[f"{k}_ms_max"] = round(min(ms[k]), 4), round(max(ms[k]), 4)
    row["peaks_over_copy"] = round(med["peaks_k2"] / med["copy"], 2)
    row["peaks_read_gb_s"] = round(8 * cells / med["peaks_k2"] / 1e6, 1)
    row["copy_read_plus_write_gb_s"] = round(2 * 8 * cells / med["copy"] / 1e6, 1)
    for k, v in whole.items():
        row[f"acq_{k}_ms"] = round(statistics.median(v), 3)
    print(json.dumps(row))


if __name__ == "__main__":
    main()
