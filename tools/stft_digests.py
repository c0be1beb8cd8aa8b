#!/usr/bin/env python3
"""SHA-256 of every output of the five short-time kernels that share device stages (ridge, chirp-rate search, excisor,
chirp excisor, canceller) on small seeded captures: one line per digest.

Two builds of the library compute the same bits exactly when two runs of this script, one process per build chosen
with GPSJAM_LIB, print the same lines:
    GPSJAM_LIB=/path/to/other/libgpsjam_hip.so python tools/stft_digests.py > other.txt
    python tools/stft_digests.py > this.txt && cmp other.txt this.txt
The script itself checks what must hold inside one build: rates (0, 1, 1) give the ridge's fields, and W = 0 gives the
excisor's bytes; it exits 1 when either does not.

Inputs: 1 MiB of uniform random bytes per capture (seeds 20240607 and 20240608), both unpack conventions, every nfft
from 16 to 4096, first sample 3.  Ridge and search at hop 37 and at hop 1 (more than one step per workgroup and a
part-filled last step), guard 1, every frame that fits; the search at rates (-3, 2, 4) with peaks.  The cleaners over
524 277 samples (a tail behind the last hop and a short last run), flat threshold 0.5 nfft; the chirp excisor at rates
cycling through (0, 1, -2, 5); the canceller with three seeded weight sets, |W| <= 1, and a frames_per_set that does not
divide the frame count.  Reads nothing outside the repository."""
import hashlib
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "gps-jamming_amd"), REPO]
NBYTES = 1 << 20
FIRST = 3
N_CLEAN = 524277
SIZES = tuple(1 << k for k in range(4, 13))
CONVENTIONS = ((127.5, 1.0 / 127.5), (128.0, 1.0 / 128.0))


def digest(*arrays) -> str:
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def main() -> int:
    import gpsjam
    raw_a = np.random.default_rng(20240607).integers(0, 256, NBYTES, dtype=np.uint8)
    raw_b = np.random.default_rng(20240608).integers(0, 256, NBYTES, dtype=np.uint8)
    wrng = np.random.default_rng(20240609)
    bad = 0

    def show(conv, nfft, what, *arrays):
        print(f"off={conv[0]} nfft={nfft} {what} {digest(*arrays)}")

    def cleaned(result):
        cap, rec = result
        with cap:
            return cap.download(), rec

    with gpsjam.Device(0) as dev, dev.capture(raw_a) as a, dev.capture(raw_b) as b:
        for conv in CONVENTIONS:
            dev.set_unpack(*conv)
            for nfft in SIZES:
                for hop in (37, 1):
                    ridge = dev.ridge(a, nfft, hop, FIRST, guard=1)
                    show(conv, nfft, f"ridge hop={hop} frames={len(ridge)}", ridge.records)
                    scan = dev.chirp(a, nfft, hop, (-3, 2, 4), FIRST, guard=1, want_peaks=True)
                    show(conv, nfft, f"chirp hop={hop} records", scan.records)
                    show(conv, nfft, f"chirp hop={hop} peaks", scan.peaks)
                    zero = dev.chirp(a, nfft, hop, (0, 1, 1), FIRST, guard=1)
                    same = all(np.array_equal(zero.records[k].view(np.uint32), ridge.records[k].view(np.uint32))
                               for k in ("total", "peak", "second", "peak_bin")) and not zero.rate_index.any()
                    bad += not same
                    show(conv, nfft, f"chirp hop={hop} rate0 ridge_fields={'equal' if same else 'DIFFER'}", zero.records)
                thr = np.full(nfft, 0.5 * nfft, np.float32)
                frames = gpsjam.excise_frames(N_CLEAN, nfft)
                out, rec = cleaned(dev.excise(a, thr, nfft, FIRST, N_CLEAN))
                show(conv, nfft, f"excise frames={frames} bytes", out)
                show(conv, nfft, "excise records", rec)
                rates = np.resize(np.array([0, 1, -2, 5], np.int32), frames)
                out_c, rec_c = cleaned(dev.excise_chirp(a, thr, rates, nfft, FIRST, N_CLEAN))
                show(conv, nfft, "excise_chirp bytes", out_c)
                show(conv, nfft, "excise_chirp records", rec_c)
                w = (wrng.uniform(0, 1, (3, nfft)) * np.exp(2j * np.pi * wrng.uniform(0, 1, (3, nfft)))).astype(np.complex64)
                per_set = frames // 3 + 1 if frames % (frames // 3 + 1) else frames // 3 + 2
                out_w, rec_w = cleaned(dev.cancel(a, b, w, thr, nfft, FIRST, 5, N_CLEAN, per_set))
                show(conv, nfft, f"cancel sets=3 frames_per_set={per_set} bytes", out_w)
                show(conv, nfft, "cancel records", rec_w)
                out_0, rec_0 = cleaned(dev.cancel(a, b, np.zeros(nfft, np.complex64), thr, nfft, FIRST, 5, N_CLEAN))
                same = np.array_equal(out_0, out)
                bad += not same
                show(conv, nfft, f"cancel W=0 excise_bytes={'equal' if same else 'DIFFER'}", out_0)
                show(conv, nfft, "cancel W=0 records", rec_0)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
