#!/usr/bin/env python3
"""ONE measurement of K2 solo for an A/B between two builds of the library: a fresh process, one 1-GiB capture, the
clocks preconditioned with 20 launches (as tools/k2_ab_probe.py does with its first rounds), then the median and the
range of 10 launches' kernel_ms (gj_welch_timed_dev: K2 without the finalize).  Interleave the builds from the shell:

    for i in 1 2 3 4 5 6; do
      GPSJAM_LIB=$PWD/build_ab/libgpsjam_parent.so python tools/k2_solo_ms.py 4096
      python tools/k2_solo_ms.py 4096
    done
"""
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "gps-jamming_amd"))


def main():
    import gpsjam
    from gpsjam.synth import StreamSpec
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    dev = gpsjam.Device(0)
    nbytes = 1 << 30
    ns = nbytes // 2
    cap = dev.alloc(nbytes)
    dev.synth_dev(StreamSpec(seed=1234, antenna=0, jam_start=int(0.4 * ns), jam_end=int(0.7 * ns), jam_sigma=60.0), ns, cap)
    psd = dev.alloc(4 * dev.welch_rows(nbytes, 2048000, n) * n)
    dev.reserve(dev.welch_workspace(nbytes, 2048000, n))
    for _ in range(20):
        dev.welch_timed_dev(cap, nbytes, 2048000, n, 2.048e6, psd)
    ks = [dev.welch_timed_dev(cap, nbytes, 2048000, n, 2.048e6, psd)[0] for _ in range(10)]
    lib = os.path.basename(gpsjam.library_path())
    print(f"k2_solo nperseg={n} lib={lib} median_ms={statistics.median(ks):.4f} min_ms={min(ks):.4f} max_ms={max(ks):.4f}")
    dev.close()


if __name__ == "__main__":
    main()
