"""K2's detrend was rewritten for fewer vector instructions, and the fused scan's block-sum reduction is the next
candidate (profiles/NOTES_valu_diet.md); every output has to be the bytes it was.  tests/golden/valu_diet_hashes.json
holds the SHA-256 of each output below, recorded from the kernels before the rewrite (tests/valu_diet_cases.py --write).

Scan: a full tile (four vectors a trip, four block sums), a tile plus 16 bytes, a capture that
ends inside a 512-sample block, a ragged end of three samples, an odd trailing byte, chunks of one and of three tiles, a
part with a halo and a noise workgroup through the split entry point, both unpack conventions -- each with
rssi_threshold 0 (no first-hit tracking) and with a threshold inside the amplitude range.  Compared: chunk powers, the
noise-floor threshold, amplitude statistics, amplitude tiles (sum and first hit), the part's amplitude record, the onset
record.  Chunk powers and the onset record must also equal the integer-exact restatement, the amplitude statistics agree
with it at its 2e-7.  The 512-sample block sums live in the library's workspace and are not handed out: they are checked
through the onset record's noise level, which over a span of k whole blocks is the sum of the first k of them -- on a
capture quiet enough for that sum to be exact in float32, for every k.

K2: every nperseg from 16 to 4096 at three and at many segments per chunk (three chunks and a shorter last one); 4096
and 1024 at 1, 2, 3 and 6; captures of zeros, of 255s and with a constant offset (I = 200, Q = 40: a large mean for the
detrend to remove); the batched entry with two captures."""
import json
import os

import numpy as np
import pytest

import exact_restatement as er
import valu_diet_cases as vc
from gpu_lib import Convention

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(os.path.dirname(HERE), "golden", "valu_diet_hashes.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def raws(dev):
    """(kind, bytes) -> the capture, made once and left unchanged."""
    made = {}

    def get(kind, nbytes):
        if (kind, nbytes) not in made:
            made[(kind, nbytes)] = vc.capture_bytes(dev, kind, nbytes)
            made[(kind, nbytes)].setflags(write=False)
        return made[(kind, nbytes)]

    yield get
    made.clear()


def same_as_recorded(golden, cid, outputs):
    for k, b in outputs.items():
        assert vc.sha(np.frombuffer(b, np.uint8)) == golden[f"{cid}/{k}"], f"{cid}: {k} is not the bytes it was"


@pytest.mark.parametrize("cid,kind,shape,thr,conv", vc.scan_cases(), ids=[c[0] for c in vc.scan_cases()])
def test_scan_outputs_are_the_recorded_bytes(dev, golden, raws, cid, kind, shape, thr, conv):
    nbytes, chunk_bytes = vc.SCAN_SHAPES[shape]
    raw = raws(kind, nbytes)
    offset, scale = vc.CONVENTIONS[conv]
    with Convention(dev, offset, scale):
        out = vc.run_scan(dev, raw, chunk_bytes, thr)
    same_as_recorded(golden, cid, out)
    # the two entry points agree, and both say what the header promises
    assert out["part_power"] == out["power"]
    o2 = int(round(2 * offset))
    want = er.chunk_power(raw, chunk_bytes, o2=o2)
    assert np.frombuffer(out["power"], np.float32).tobytes() == want.tobytes()
    o, want_o = np.frombuffer(out["onset"], er.ONSET_T)[0], er.onset(raw, vc.NOISE, vc.WINDOW, vc.FACTOR, o2=o2)
    for f in ("start", "guard", "noise", "thr", "hit"):
        assert o[f] == want_o[f], (f, o, want_o)
    tiles = np.frombuffer(out["tiles"], np.dtype([("sum", "<f8"), ("first", "<i8")]))
    assert tiles.size == (raw.size // 2 * 2 + vc.TILE - 1) // vc.TILE
    if conv == "ref":
        a, want_a = np.frombuffer(out["amp"], er.AMP_T)[0], er.amp_stats(raw, thr)
        assert (a["i"], a["c"]) == (want_a["first"], want_a["count"])
        np.testing.assert_allclose(a["s"], want_a["sum"], rtol=2e-7)
        # a tile's first hit, and its sum, are those of its own samples
        for t in range(tiles.size):
            piece = er.amp_stats(raw[t * vc.TILE:(t + 1) * vc.TILE], thr)
            assert tiles["first"][t] == (piece["first"] + t * (vc.TILE // 2) if piece["first"] >= 0 else np.iinfo(np.int64).max)
            np.testing.assert_allclose(tiles["sum"][t], er.amp_stats(raw[t * vc.TILE:(t + 1) * vc.TILE], -1.0)["sum"], rtol=2e-7)


@pytest.mark.parametrize("cid,kind,thr", vc.scan_part_cases(), ids=[c[0] for c in vc.scan_part_cases()])
def test_scan_part_with_halo_and_noise_workgroup(dev, golden, raws, cid, kind, thr):
    raw = raws(kind, vc.SCAN_SHAPES["seven_tiles_tpc1"][0])
    out = vc.run_scan_part(dev, raw, thr)
    same_as_recorded(golden, cid, out)
    own = raw[2 * vc.TILE:]
    assert np.frombuffer(out["part_power"], np.float32).tobytes() == er.chunk_power(own, vc.TILE).tobytes()
    o = np.frombuffer(out["part_onset"], er.ONSET_T)[0]
    assert o["noise"] == er.onset(raw, vc.NOISE, vc.WINDOW, vc.FACTOR)["noise"]


def test_every_block_sum_lands_in_its_block(dev):
    """Two full tiles and one that ends inside its sixth block: the noise level over the first k blocks, k = 1 .. all whole
    blocks, is exact -- a block sum stored to a neighbour's place, or a trip's four sums permuted, changes one of them."""
    nbytes = 2 * vc.TILE + 2 * (512 * 5 + 100)
    raw = vc.quiet_capture(nbytes)
    m = er.msq(raw)
    assert int(m.sum()) < 1 << 24
    cap, d_on = dev.alloc(nbytes).upload(raw), dev.alloc(32)
    got, want = [], []
    try:
        for k in range(1, 2 * 64 + 5 + 1):
            dev.onset_dev(cap, nbytes, 512 * k, 100, vc.FACTOR, d_on)
            dev.synchronize()
            got.append(d_on.download(np.uint8).view(er.ONSET_T)[0]["noise"])
            want.append(np.float32(int(m[:512 * k].sum()) / (4.0 * 512 * k)))
    finally:
        cap.free()
        d_on.free()
    assert len(set(np.diff(np.array([int(m[:512 * k].sum()) for k in range(0, 2 * 64 + 6)])).tolist())) > 60   # the blocks differ
    assert np.array(got, np.float32).tobytes() == np.array(want, np.float32).tobytes()


@pytest.mark.parametrize("cid,kind,nperseg,nseg", vc.k2_cases(), ids=[c[0] for c in vc.k2_cases()])
def test_k2_psd_is_the_recorded_bytes(dev, golden, raws, cid, kind, nperseg, nseg):
    chunk, ns, rows = vc.k2_geometry(nperseg, nseg)
    assert dev.welch_rows(2 * ns, chunk, nperseg) == rows
    psd = vc.run_k2(dev, raws(kind, 2 * ns), chunk, nperseg, rows)
    assert np.all(np.isfinite(psd)) and np.all(psd >= 0)
    assert vc.sha(psd) == golden[cid], f"{cid}: the PSD is not the bytes it was"


@pytest.mark.parametrize("nperseg,nseg", vc.BATCH)
def test_k2_batched_entry_two_captures(dev, golden, raws, nperseg, nseg):
    chunk, ns, rows = vc.k2_geometry(nperseg, nseg)
    both = [raws(f"seed{nperseg + a}", 2 * ns) for a in range(2)]
    for a, psd in enumerate(vc.run_k2_batch(dev, both, chunk, nperseg, rows)):
        assert vc.sha(psd) == golden[f"k2batch-{nperseg}-{nseg}seg-{a}"]
        assert psd.tobytes() == vc.run_k2(dev, both[a], chunk, nperseg, rows).tobytes()
