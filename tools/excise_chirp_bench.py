#!/usr/bin/env python3
"""The chirp-domain excisor (gj_excise_chirp_dev) against the plain one (gj_excise_dev) on one resident capture, and the
whole mitigate.clean_swept chain.

Both kernels are in the same library and walk the same frames; the chirp-domain one adds, per thread and frame, the
factor construction (three sincospif from 256 points on, 32 lane permutations, about 25 complex products) and two times
sixteen complex multiplications.  From the code alone that is a little over 1 x.  bench.py times neither, so the figures
come from here:

  chirp   gj_excise_chirp_dev at nfft 256, 1024 and 4096 over a whole 10-s synthetic capture (40 960 000 bytes), a flat
          threshold 16 x the noise floor, frame records on, one rate per frame cycling through --rate-cycle values around
          a 4 GHz/s sweep (the rate's value does not change the instruction stream), HIP events around the call
  plain   gj_excise_dev with the same arguments but the rates
  chain   mitigate.clean_swept with the sweep and the threshold given (no characterise_swept, no floor measurement):
          the chirp-rate search over 17 rates at hop nfft / 2, the picker, the excisor, records and rates to the host;
          host wall clock around the call, which ends with a download and so with the stream drained

chirp and plain are interleaved call by call, so that every pair of figures comes from the same moment of the same GPU;
every shape is warmed up first; medians over --steps pairs, min and max beside them.  Prints one JSON line.
    python tools/excise_chirp_bench.py [--steps 200] [--warmup 20] [--chain-steps 10]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "gps-jamming_amd"), REPO]
NBYTES = 40960000
FS = 2.048e6
SIZES = (256, 1024, 4096)
NOISE_SIGMA = 6.25
SWEEP = 4.0e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--chain-steps", type=int, default=10)
    ap.add_argument("--rate-cycle", type=int, default=5)
    args = ap.parse_args()
    import gpsjam
    from gpsjam import mitigate
    from gpsjam.synth import StreamSpec
    n = NBYTES // 2
    with gpsjam.Device(0) as dev:
        buf = dev.alloc(NBYTES)
        dev.synth_dev(StreamSpec(seed=9, antenna=0, delay=0, jam_start=n // 2, jam_end=1 << 40, jam_sigma=50.0), n, buf)
        cap = gpsjam.Capture.from_device(dev, buf, NBYTES)
        d_out = dev.alloc(NBYTES)
        rows = {}
        for nfft in SIZES:
            frames = gpsjam.excise_frames(n, nfft)
            floor = 0.375 * nfft * 2.0 * NOISE_SIGMA ** 2 / 127.5 ** 2
            thr = np.full(nfft, 16.0 * floor, np.float32)
            d_thr = dev.alloc(4 * nfft).upload(thr)
            d_rec = dev.alloc(frames * gpsjam.EXCISE_DTYPE.itemsize)
            q0 = mitigate.sweep_rate_units(SWEEP, nfft, FS)
            rates = (q0 + np.arange(frames) % max(1, args.rate_cycle)).astype(np.int32)
            d_rate = dev.alloc(4 * frames).upload(rates)
            sw_ms, pl_ms = [], []
            for step in range(args.warmup + args.steps):
                dev.timer_start()
                dev.excise_chirp_dev(cap, NBYTES, 0, n, nfft, d_rate, d_thr, d_out, d_rec)
                s = dev.timer_stop()
                dev.timer_start()
                dev.excise_dev(cap, NBYTES, 0, n, nfft, d_thr, d_out, d_rec)
                p = dev.timer_stop()
                if step >= args.warmup:
                    sw_ms.append(s)
                    pl_ms.append(p)
            chain = []
            for step in range(2 + args.chain_steps):
                t0 = time.perf_counter()
                res = mitigate.clean_swept(dev, cap, nfft=nfft, fs=FS, sweep_hz_per_s=SWEEP, threshold=thr)
                t1 = time.perf_counter()
                res.capture.free()
                if step >= 2:
                    chain.append(1e3 * (t1 - t0))
            s, p = statistics.median(sw_ms), statistics.median(pl_ms)
            rows[str(nfft)] = {"frames": frames, "q0": q0,
                               "excise_chirp_ms": round(s, 4), "excise_chirp_ms_min": round(min(sw_ms), 4),
                               "excise_chirp_ms_max": round(max(sw_ms), 4), "excise_ms": round(p, 4),
                               "excise_ms_min": round(min(pl_ms), 4), "excise_ms_max": round(max(pl_ms), 4),
                               "chirp_over_plain": round(s / p, 3),
                               "clean_swept_given_threshold_ms": round(statistics.median(chain), 3),
                               "clean_swept_ms_min": round(min(chain), 3), "clean_swept_ms_max": round(max(chain), 3),
                               "frames_dechirped": int(np.count_nonzero(res.rates))}
            for b in (d_thr, d_rec, d_rate):
                b.free()
        cap.free()
        d_out.free()
        info = dev.info()
    print(json.dumps({"bench": "excise_chirp_vs_excise", "device": info["name"], "capture_bytes": NBYTES, "steps": args.steps,
                      "warmup": args.warmup, "chain_steps": args.chain_steps, "sizes": rows}))


if __name__ == "__main__":
    main()
