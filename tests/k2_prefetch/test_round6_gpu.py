"""K2's carried front end (nperseg 4096 and 1024) at the smallest shapes at which a misplaced wait on the prefetched half
segment, or a prefetch past the end of a run, can show: runs of 1, 2 and a few steps, workgroups with idle transform
groups, runs of different lengths inside one workgroup, a ragged last chunk.

Every shape is a capture of three full chunks plus a shorter last chunk that still holds at least one segment (where a
chunk is exactly one segment long no shorter chunk can hold one: there the capture is four chunks and a tail that gives
no row).  Inputs come from the device generator with the seeds of test_gpu_parity.test_k2_all_sizes_vs_oracle
(seed = nperseg), plus a saturated capture (all bytes 255).

Checks, per shape and capture: the PSD against the float64 oracle at the tolerance of the K2 parity tests (1e-4 relative
on the linear PSD; for the saturated capture, whose true spectrum is empty, the absolute bound of
test_extremes_gpu.test_extreme_k2_welch); two launches one after the other byte-equal; the same launch while a second
context's stream runs the fused scan over the same capture, byte-equal to the launch alone."""
import numpy as np
import pytest

import gpsjam
from gpsjam.synth import StreamSpec
from oracle import gpsjam_oracle as orc

pytestmark = pytest.mark.gpu

FS = 2.048e6
# (nperseg, segments per full chunk).  4096: 1, 2, 6 (two workgroups per chunk) and 46 segments.  1024: four transform
# groups per workgroup, so 1, 3 segments leave groups idle, 4 fills them once, 5 and 9 give runs of unequal length.
SHAPES = [(4096, 1), (4096, 2), (4096, 6), (4096, 46), (1024, 1), (1024, 3), (1024, 4), (1024, 5), (1024, 9)]
KINDS = ["synth", "saturated"]


def geometry(nperseg, nseg):
    chunk = nperseg + (nperseg // 2) * (nseg - 1)
    if nseg == 1:
        return chunk, 4 * chunk + 101, 4                       # four one-segment chunks and a tail that gives no row
    last = max(nperseg + 101, chunk - nperseg // 2 - 3)        # ragged, at least one segment, fewer than a full chunk
    assert nperseg <= last < chunk
    return chunk, 3 * chunk + last, 4


@pytest.fixture(scope="module")
def cases(dev):
    """(nperseg, nseg, kind) -> the capture resident in HBM and its float64 PSD, made once and left unchanged."""
    made = {}

    def get(nperseg, nseg, kind):
        key = (nperseg, nseg, kind)
        if key not in made:
            chunk, ns, rows = geometry(nperseg, nseg)
            cap = dev.alloc(2 * ns)
            if kind == "saturated":
                raw = np.full(2 * ns, 255, np.uint8)
                cap.upload(raw)
            else:
                spec = StreamSpec(seed=nperseg, jam_start=ns // 3, jam_end=(2 * ns) // 3, jam_sigma=30.0, dc_i_q8=600, dc_q_q8=-900)
                dev.synth_dev(spec, ns, cap)
                dev.synchronize()
                raw = cap.download(np.uint8)
            lin, _, _ = orc.widmo_waterfall(raw, nperseg=nperseg, chunk_samples=chunk)
            assert lin.shape == (rows, nperseg)
            lin.setflags(write=False)
            made[key] = (cap, lin, chunk, ns, rows)
        return made[key]

    yield get
    made.clear()


@pytest.fixture(scope="module")
def side():
    """A second context: its stream runs beside the session context's."""
    with gpsjam.Device(0) as d:
        yield d


def launch(dev, cap, ns, chunk, nperseg, rows):
    d_psd = dev.alloc(4 * rows * nperseg)
    dev.welch_dev(cap, 2 * ns, chunk, nperseg, FS, d_psd)
    dev.synchronize()
    return d_psd.download(np.float32).reshape(rows, nperseg)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("nperseg,nseg", SHAPES)
def test_k2_carried_front_end(dev, side, cases, nperseg, nseg, kind):
    cap, lin, chunk, ns, rows = cases(nperseg, nseg, kind)
    assert dev.welch_rows(2 * ns, chunk, nperseg) == rows
    psd = launch(dev, cap, ns, chunk, nperseg, rows)
    assert np.all(np.isfinite(psd)) and np.all(psd >= 0)
    scale = lin.max(axis=1, keepdims=True)
    big = lin > 1e-6 * np.maximum(scale, 1e-30)
    full_scale = 1.0 / (FS * 0.375 * nperseg) * nperseg ** 2 * 2.0
    err = float(np.max(np.abs(psd[big] - lin[big]) / lin[big])) if big.any() else 0.0
    absd = float(np.max(np.abs(psd - lin)))
    print(f"nperseg {nperseg}, {nseg} segments per chunk, {kind}: {int(big.sum())} bins, largest relative error {err:.2e}, "
          f"largest absolute difference {absd:.2e}")
    if kind == "synth":
        keep = lin > 1e-12                                         # rel_err of the K2 parity tests
        assert float(np.max(np.abs(psd[keep] - lin[keep]) / lin[keep])) < 1e-4
    else:
        assert absd < 2e-5 * max(float(scale.max()), 5e-8 * full_scale)
    # two launches one after the other
    again = launch(dev, cap, ns, chunk, nperseg, rows)
    assert again.tobytes() == psd.tobytes()
    # the same launch beside the fused scan of the same capture on a second context's stream
    nch = side.chunk_count(2 * ns, 65536)
    d_pow, d_amp, d_on = side.alloc(4 * nch), side.alloc(32), side.alloc(32)
    d_psd = dev.alloc(4 * rows * nperseg)
    for _ in range(4):
        side.stream_scan_dev(cap, 2 * ns, 65536, d_pow, 0.0, d_amp, 1000, 100, 50.0, d_on)
    dev.welch_dev(cap, 2 * ns, chunk, nperseg, FS, d_psd)
    for _ in range(4):
        side.stream_scan_dev(cap, 2 * ns, 65536, d_pow, 0.0, d_amp, 1000, 100, 50.0, d_on)
    dev.synchronize()
    side.synchronize()
    beside = d_psd.download(np.float32).reshape(rows, nperseg)
    assert beside.tobytes() == psd.tobytes()
