"""Inputs, shapes and calls of the fused scan and of K2 whose OUTPUT BYTES are pinned by tests/golden/valu_diet_hashes.json
-- test infrastructure, never imported by the product.  The hashes were recorded from the kernels as they stood before
K2's detrend was rewritten for fewer vector instructions (profiles/NOTES_valu_diet.md): a rewrite of
that kind has to return the same bytes, whatever it does inside.

    python tests/valu_diet_cases.py --write tests/golden/valu_diet_hashes.json     # on a GPU, at the commit to pin

tests/valu_diet/test_round6_gpu.py compares against the file, and against the integer-exact restatements of
tests/exact_restatement.py where they cover a quantity."""
import hashlib
import json
import os
import sys

import numpy as np

TILE = 65536
FS = 2.048e6
NOISE, WINDOW, FACTOR = 3000, 100, 50.0


def sha(b) -> str:
    return hashlib.sha256(np.ascontiguousarray(b).tobytes()).hexdigest()


# ------------------------------------------------------------------------------------------------ captures
def synth(dev, seed, nbytes):
    """nbytes of the library's integer generator (gj_synth_dev), a jammer switched on two thirds of the way through."""
    from gpsjam.synth import StreamSpec
    ns = (nbytes + 1) // 2
    cap = dev.alloc(2 * ns)
    dev.synth_dev(StreamSpec(seed=seed, jam_start=(2 * ns) // 3, jam_end=1 << 40, jam_sigma=40.0, dc_i_q8=600, dc_q_q8=-900), ns, cap)
    dev.synchronize()
    raw = cap.download(np.uint8)[:nbytes].copy()
    cap.free()
    return raw


def capture_bytes(dev, kind, nbytes):
    if kind == "zeros":
        return np.zeros(nbytes, np.uint8)
    if kind == "ones":
        return np.full(nbytes, 255, np.uint8)
    if kind == "offset":                     # I = 200, Q = 40: a large mean, so the detrend matters
        raw = np.empty(nbytes, np.uint8)
        raw[0::2], raw[1::2] = 200, 40
        return raw
    assert kind.startswith("seed")
    return synth(dev, int(kind[4:]), nbytes)


KINDS = ["seed11", "seed12", "zeros", "ones", "offset"]

# ------------------------------------------------------------------------------------------------ the scan
# name -> (bytes, chunk_bytes).  Tiles are 64 KiB = 64 blocks of 512 samples; a full tile takes the four-vectors-a-trip
# path, a shorter last one the one-vector-a-trip path.
SCAN_SHAPES = {
    "one_tile": (TILE, TILE),
    "tile_plus_16": (TILE + 16, TILE),
    "ends_inside_a_block": (TILE + 2 * (512 * 5 + 100), TILE),
    "ragged_3_samples": (2 * TILE + 16 * 7 + 2 * 3, TILE),
    "odd_trailing_byte": (TILE + 4096 + 1, TILE),
    "seven_tiles_tpc1": (7 * TILE + 2468, TILE),
    "seven_tiles_tpc3": (7 * TILE + 2468, 3 * TILE),
}
#: rssi_threshold 0 (no first-hit tracking: the instantiation the benchmark runs) and one inside the amplitude range
THRESHOLDS = [0.0, 0.9]
#: (offset, scale) of the unpack: the reference's and gnssdec's
CONVENTIONS = {"ref": (127.5, 1.0 / 127.5), "gnssdec": (128.0, 1.0 / 128.0)}


def _zeros(dev, n):
    return dev.alloc(n).upload(np.zeros(n, np.uint8))


def run_scan(dev, raw, chunk_bytes, thr):
    """The capture through gj_capture_scan_dev (power, threshold, amplitude statistics, onset) and, as ONE part that is
    the whole capture, through gj_part_scan_dev (which hands out the amplitude tiles: sum and first hit per 64 KiB).
    {name: bytes}."""
    from gpsjam import _ffi
    n = raw.size
    cap = dev.alloc(n + 16).upload(raw)
    nch, nt = dev.chunk_count(n, chunk_bytes), dev.amp_tile_count(n)
    bufs = dict(power=_zeros(dev, 4 * nch), amp=_zeros(dev, 32), onset=_zeros(dev, 32), stats=_zeros(dev, 12),
                part_power=_zeros(dev, 4 * nch), tiles=_zeros(dev, 16 * nt), amp_part=_zeros(dev, 32), part_onset=_zeros(dev, 32))
    try:
        dev.capture_scan_dev(cap, n, chunk_bytes, bufs["power"], thr, bufs["amp"], NOISE, WINDOW, FACTOR, bufs["onset"], d_stats=bufs["stats"])
        view = _ffi.PartView(cap.ptr, n, 0, 0, n, n, None)
        dev.part_scan_dev(view, chunk_bytes, bufs["part_power"], thr, bufs["tiles"], bufs["amp_part"], NOISE, WINDOW, FACTOR, bufs["part_onset"])
        dev.synchronize()
        return {k: b.download(np.uint8).tobytes() for k, b in bufs.items()}
    finally:
        for b in list(bufs.values()) + [cap]:
            b.free()


def run_scan_part(dev, raw, thr, first_tile=2, halo_tiles=1):
    """A part in the middle of the capture through the split entry point: its buffer starts `halo_tiles` in front of its
    own range (skip_tiles > 0) and does not hold the capture's noise span (one more workgroup sums the copy)."""
    from gpsjam import _ffi
    n = raw.size
    b0, own0 = (first_tile - halo_tiles) * TILE, first_tile * TILE
    own = n - own0
    cap, d_noise = dev.alloc(n - b0 + 16).upload(raw[b0:]), dev.alloc(2 * NOISE).upload(raw[:2 * NOISE])
    nch, nt = dev.chunk_count(own, TILE), dev.amp_tile_count(own)
    bufs = dict(part_power=_zeros(dev, 4 * nch), tiles=_zeros(dev, 16 * nt), amp_part=_zeros(dev, 32), part_onset=_zeros(dev, 32))
    try:
        view = _ffi.PartView(cap.ptr, n - b0, b0, own0, own, n, d_noise.ptr)
        dev.part_scan_dev(view, TILE, bufs["part_power"], thr, bufs["tiles"], bufs["amp_part"], NOISE, WINDOW, FACTOR, bufs["part_onset"])
        dev.synchronize()
        return {k: b.download(np.uint8).tobytes() for k, b in bufs.items()}
    finally:
        for b in list(bufs.values()) + [cap, d_noise]:
            b.free()


def scan_cases():
    """(case id, kind, shape name, threshold, convention); every shape with the two seeds, the hand-made captures at the
    shape that has every path (full tiles, a last tile that ends inside a block)."""
    out = []
    for shape in SCAN_SHAPES:
        for thr in THRESHOLDS:
            out.append((f"scan-{shape}-seed11-thr{thr}-ref", "seed11", shape, thr, "ref"))
    for kind in ("seed12", "zeros", "ones", "offset"):
        for thr in THRESHOLDS:
            out.append((f"scan-ends_inside_a_block-{kind}-thr{thr}-ref", kind, "ends_inside_a_block", thr, "ref"))
    for thr in THRESHOLDS:
        out.append((f"scan-ends_inside_a_block-seed11-thr{thr}-gnssdec", "seed11", "ends_inside_a_block", thr, "gnssdec"))
        out.append((f"scan-seven_tiles_tpc1-seed12-thr{thr}-gnssdec", "seed12", "seven_tiles_tpc1", thr, "gnssdec"))
    return out


def scan_part_cases():
    return [(f"scanpart-seven_tiles-{kind}-thr{thr}", kind, thr) for kind in ("seed11", "offset") for thr in THRESHOLDS]


def quiet_capture(nbytes):
    """Bytes 127 / 128 (m = 2 per sample) with ONE louder sample per 512-sample block, different from block to block: the
    sum of m over any run of blocks stays below 2^24, so the float32 noise level of an onset call over the first k blocks
    tells exactly which block sums it was made of."""
    rng = np.random.default_rng(5)
    raw = rng.integers(127, 129, nbytes, dtype=np.uint8)
    ns = nbytes // 2
    for b in range((ns + 511) // 512):
        s = b * 512 + (b * 37) % 512
        if s < ns:
            raw[2 * s] = 128 + 1 + (b * 7) % 90
    return raw


# ------------------------------------------------------------------------------------------------ K2
def k2_geometry(nperseg, nseg):
    """Three full chunks of `nseg` segments and a shorter last one that still holds a segment (tests/k2_prefetch)."""
    chunk = nperseg + (nperseg // 2) * (nseg - 1)
    if nseg == 1:
        return chunk, 4 * chunk + min(101, nperseg - 1), 4       # four one-segment chunks and a tail that gives no row
    last = max(nperseg + min(101, nperseg // 2 - 1), chunk - nperseg // 2 - 3)
    assert nperseg <= last < chunk
    return chunk, 3 * chunk + last, 4


K2_SIZES = [16, 32, 64, 128, 256, 512, 1024, 2048, 4096]


def k2_cases():
    """(case id, kind, nperseg, segments per chunk): every size at 3 segments per chunk and at enough of them for several
    steps per transform group; 4096 and 1024 at 1, 2, 3 and 6; the hand-made captures at 4096, 1024 and 64."""
    out = []
    for n in K2_SIZES:
        for nseg in sorted({3, 2 * (4096 // n) + 3}):
            out.append((f"k2-{n}-{nseg}seg-seed{n}", f"seed{n}", n, nseg))
    for n in (4096, 1024):
        for nseg in (1, 2, 6):
            out.append((f"k2-{n}-{nseg}seg-seed{n}", f"seed{n}", n, nseg))
    for n in (4096, 1024, 64):
        for kind in ("zeros", "ones", "offset"):
            out.append((f"k2-{n}-6seg-{kind}", kind, n, 6))
    return out


def run_k2(dev, raw, chunk, nperseg, rows):
    assert dev.welch_rows(raw.size, chunk, nperseg) == rows
    cap, d_psd = dev.alloc(raw.size).upload(raw), dev.alloc(4 * rows * nperseg)
    try:
        dev.welch_dev(cap, raw.size, chunk, nperseg, FS, d_psd)
        dev.synchronize()
        return d_psd.download(np.float32).reshape(rows, nperseg)
    finally:
        cap.free()
        d_psd.free()


def run_k2_batch(dev, raws, chunk, nperseg, rows):
    assert all(r.size == raws[0].size for r in raws) and dev.welch_rows(raws[0].size, chunk, nperseg) == rows
    caps = [dev.alloc(r.size).upload(r) for r in raws]
    outs = [dev.alloc(4 * rows * nperseg) for _ in raws]
    try:
        dev.welch_batch_dev(caps, raws[0].size, chunk, nperseg, FS, outs)
        dev.synchronize()
        return [o.download(np.float32).reshape(rows, nperseg) for o in outs]
    finally:
        for b in caps + outs:
            b.free()


BATCH = [(4096, 6), (1024, 9), (128, 70)]


# ------------------------------------------------------------------------------------------------ recording
def record(dev):
    from gpu_lib import Convention
    hashes = {}
    made = {}

    def raw_of(kind, nbytes):
        if (kind, nbytes) not in made:
            made[(kind, nbytes)] = capture_bytes(dev, kind, nbytes)
        return made[(kind, nbytes)]

    for cid, kind, shape, thr, conv in scan_cases():
        nbytes, chunk_bytes = SCAN_SHAPES[shape]
        with Convention(dev, *CONVENTIONS[conv]):
            for k, b in run_scan(dev, raw_of(kind, nbytes), chunk_bytes, thr).items():
                hashes[f"{cid}/{k}"] = sha(np.frombuffer(b, np.uint8))
    for cid, kind, thr in scan_part_cases():
        for k, b in run_scan_part(dev, raw_of(kind, SCAN_SHAPES["seven_tiles_tpc1"][0]), thr).items():
            hashes[f"{cid}/{k}"] = sha(np.frombuffer(b, np.uint8))
    for cid, kind, n, nseg in k2_cases():
        chunk, ns, rows = k2_geometry(n, nseg)
        hashes[cid] = sha(run_k2(dev, raw_of(kind, 2 * ns), chunk, n, rows))
    for n, nseg in BATCH:
        chunk, ns, rows = k2_geometry(n, nseg)
        for a, psd in enumerate(run_k2_batch(dev, [raw_of(f"seed{n + a}", 2 * ns) for a in range(2)], chunk, n, rows)):
            hashes[f"k2batch-{n}-{nseg}seg-{a}"] = sha(psd)
    return hashes


if __name__ == "__main__":
    here = os.path.dirname(os.path.abspath(__file__))
    for p in (os.path.join(os.path.dirname(here), "gps-jamming_amd"), here):
        sys.path.insert(0, p)
    import gpsjam
    assert len(sys.argv) == 3 and sys.argv[1] == "--write", __doc__
    with gpsjam.Device(0) as device:
        out = record(device)
    with open(sys.argv[2], "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(out)} hashes written to {sys.argv[2]} with {gpsjam.library_path()}")
