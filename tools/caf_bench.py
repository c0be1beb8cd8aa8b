#!/usr/bin/env python3
"""The cross-ambiguity search against a loop of K5 solves, interleaved on one box.

  A   one gj_xcorr_caf_dev: 3 antennas / 3 pairs, n_bins bins                       (this tree's library)
  B   n_bins back-to-back gj_xcorr_lags_dev solves of the same shape                 (--parent-lib: the library of the
      parent commit) -- what a host loop over pre-rotated slices would cost at best
  K5  one gj_xcorr_lags_dev, 3 pairs, n = 2^19, this tree's library against the parent's: the new kernels share K5's
      module and must not move it

One child process per (variant, round), HIP events around `reps` back-to-back calls, median over the rounds.
    python tools/caf_bench.py --parent-lib build_ab/libgpsjam_parent.so [--rounds 10] [--bpl 0,8,...]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "gps-jamming_amd"), REPO]
SHAPES = [(50000, 129), (1 << 19, 33)]
PAIRS = [(0, 1), (0, 2), (1, 2)]


def child(args):
    import numpy as np
    import gpsjam
    from gpsjam import _ffi
    from gpsjam.synth import StreamSpec
    if os.environ.get("GPSJAM_LIB"):       # an older library: bind only what it exports
        import ctypes
        old = ctypes.CDLL(_ffi.LIB_PATH)
        for name in [k for k in _ffi.SIGNATURES if not hasattr(old, k)]:
            del _ffi.SIGNATURES[name]
    n, n_bins, bpl = args.n, args.bins, int(args.bpl)
    with gpsjam.Device(0) as dev:
        caps = []
        for a, d in enumerate((0, 3, -5)):
            c = dev.alloc(2 * n + 64)
            dev.synth_dev(StreamSpec(seed=9, antenna=a, delay=d, jam_start=0, jam_end=1 << 40, jam_sigma=50.0), n + 32, c)
            caps.append(c)
        starts = dev.alloc(64)
        starts.upload(np.array([8, 8, 8, 0, 0, 0, 0, 0], np.int64).view(np.uint8))
        sizes = [2 * n + 64] * 3
        d_l, d_p, d_m = dev.alloc(64), dev.alloc(64), dev.alloc(64)
        if args.what == "caf":
            d_out, d_bl, d_bp = dev.alloc(24 * 3), dev.alloc(12 * n_bins), dev.alloc(12 * n_bins)
            dev.reserve(dev.xcorr_caf_workspace(3, n, 3, n_bins, bpl))
            call = lambda: dev.xcorr_caf_dev(caps, sizes, starts, n, PAIRS, -(n_bins // 2), n_bins, d_out, d_bl, d_bp,
                                             bins_per_launch=bpl)
        else:
            def call():
                for _ in range(n_bins):
                    dev.xcorr_lags_dev(caps, sizes, starts, n, PAIRS, d_l, d_p, d_m)
        for _ in range(3):
            call()
        dev.synchronize()
        times = []
        for _ in range(5):
            dev.timer_start()
            for _ in range(args.reps):
                call()
            times.append(1e3 * dev.timer_stop() / args.reps)
        print(json.dumps({"us": statistics.median(times), "us_best": min(times)}))


def run(what, n, bins, bpl, reps, lib):
    env = dict(os.environ)
    if lib:
        env["GPSJAM_LIB"] = os.path.abspath(lib)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--what", what, "--n", str(n), "--bins", str(bins),
                        "--bpl", str(bpl), "--reps", str(reps)], env=env, capture_output=True, text=True, timeout=300)
    line = next((ln for ln in r.stdout.splitlines() if ln.startswith("{")), None)
    if r.returncode or not line:
        raise SystemExit(f"{what} n {n} bins {bins} lib {lib}: rc {r.returncode}\n{r.stderr[-2000:]}")
    return json.loads(line)["us"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="libgpsjam_hip.so built from the parent commit (B and the K5 A/B)")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--bpl", default="0", help="comma list of bins_per_launch values to measure A with (0 = the default)")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--what", default="caf")
    ap.add_argument("--n", type=int, default=50000)
    ap.add_argument("--bins", type=int, default=129)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    if args.child:
        return child(args)
    bpls = [int(x) for x in args.bpl.split(",")]
    rows = {}
    for rnd in range(args.rounds):
        for n, bins in SHAPES:
            for bpl in bpls:
                rows.setdefault(("A", n, bins, bpl), []).append(run("caf", n, bins, bpl, 10, None))
            if args.parent_lib:
                rows.setdefault(("B", n, bins, "-"), []).append(run("k5", n, bins, 0, 3, args.parent_lib))
        rows.setdefault(("K5", 1 << 19, 1, "this tree"), []).append(run("k5", 1 << 19, 1, 0, 200, None))
        if args.parent_lib:
            rows.setdefault(("K5", 1 << 19, 1, "parent"), []).append(run("k5", 1 << 19, 1, 0, 200, args.parent_lib))
        print(f"round {rnd} done", flush=True)
    out = {}
    for (what, n, bins, tag), v in rows.items():
        med = statistics.median(v)
        out[f"{what} n={n} bins={bins} {tag}"] = {"median_us": round(med, 1), "per_bin_us": round(med / bins, 2),
                                                  "min_us": round(min(v), 1), "max_us": round(max(v), 1), "rounds": len(v)}
        print(f"{what:>3} n {n:>7} bins {bins:>4} {str(tag):>10}: median {med:10.1f} us  ({med / bins:8.2f} us per bin)  "
              f"min {min(v):.1f} max {max(v):.1f}  [{len(v)} rounds]", flush=True)
    for n, bins in SHAPES:
        a, b = out.get(f"A n={n} bins={bins} {bpls[0]}"), out.get(f"B n={n} bins={bins} -")
        if a and b:
            print(f"n {n} bins {bins}: A / B = {a['median_us'] / b['median_us']:.3f}  (A < B required: {a['median_us'] < b['median_us']})")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
