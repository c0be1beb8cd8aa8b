"""The short-time spectral ridge (gj_ridge_dev, Device.ridge) and classify.characterise on the GPU.

This file sits in a package of its own on purpose: the suite orders GPU files by basename (tests/conftest.py
SUITE_ORDER, which tests/test_suite_order.py holds every GPU file to), and under the name test_round6_gpu.py it runs
in stage 2, behind the parity tests of K2 whose transform it shares.

Yardstick: the float64 restatement of the definition in include/gpsjam.h (tests/ridge_restatement.py).  peak_bin is
equal on EVERY frame (tests/test_ridge_host.py shows that no input has a frame with a margin under 1e-4); total and peak
within rtol 1e-5, the project's figure for a K2 PSD value summed in another order (tests/test_gpu_parity.py); second
within 1e-5 * peak.  Translation invariance and repeatability are bit-exact."""
import numpy as np
import pytest

import gpsjam
import ridge_restatement as rr
from gpsjam import classify
from gpu_lib import GJ_ERR_INVALID, GJ_ERR_UNSUPPORTED, Guarded, refused
from gpu_lib import run_ridge as run

pytestmark = pytest.mark.gpu

REC = gpsjam.RIDGE_DTYPE.itemsize


@pytest.fixture(scope="module")
def cap(dev):
    c = dev.capture(rr.parity_capture())
    yield c
    c.free()


@pytest.mark.parametrize("nfft", rr.PARITY_NFFT)
def test_parity_with_the_restatement(dev, cap, nfft):
    for hop in rr.parity_hops(nfft):
        for first in (0, 1):
            for guard in (0, 2):
                want, _ = rr.parity_reference(nfft, hop, first, guard)
                got = run(dev, cap, cap.nbytes, nfft, hop, first, want.size, guard)
                rr.compare(got, want, (nfft, hop, first, guard))


@pytest.mark.parametrize("nfft", rr.PARITY_NFFT)
def test_frame_counts_that_do_not_fill_a_workgroup_step(dev, cap, nfft):
    per_step = 4096 // nfft
    hop, first = nfft // 2 + 37, 1
    raw = rr.parity_capture()
    for n_frames in sorted({1, per_step - 1, per_step + 1, 2 * per_step + 3} - {0}):
        # exactly all that fit: the last frame ends on the capture's last byte
        nbytes = 2 * (first + (n_frames - 1) * hop + nfft)
        assert gpsjam.ridge_frames(nbytes, first, nfft, hop) == n_frames and gpsjam.ridge_frames(nbytes - 2, first, nfft, hop) == n_frames - 1
        with dev.capture(raw[:nbytes]) as exact:
            got = run(dev, exact, nbytes, nfft, hop, first, n_frames, 2)
        want, _ = rr.ridge(raw[:nbytes], nfft, hop, first, n_frames, 2)
        rr.compare(got, want, (nfft, n_frames, "exact"))
        # the same frames as the head of the long capture: same bits
        head = run(dev, cap, cap.nbytes, nfft, hop, first, n_frames, 2)
        assert head.tobytes() == got.tobytes(), (nfft, n_frames)


@pytest.mark.parametrize("nfft", [64, 1024, 4096])    # a group inside a wave, a whole wave, the whole workgroup
def test_translation_invariance_and_repeatability_are_bit_exact(dev, cap, nfft):
    hop, first, guard = nfft // 2 + 37, 3, 2
    n = gpsjam.ridge_frames(cap.nbytes, first, nfft, hop)
    a = run(dev, cap, cap.nbytes, nfft, hop, first, n, guard)
    assert run(dev, cap, cap.nbytes, nfft, hop, first, n, guard).tobytes() == a.tobytes()
    for k in (1, 4096 // nfft + 1, 7):
        b = run(dev, cap, cap.nbytes, nfft, hop, first + k * hop, n - k, guard)
        assert b.tobytes() == a[k:].tobytes(), (nfft, k)
    # fewer frames in the call: another grid, the same bits
    assert run(dev, cap, cap.nbytes, nfft, hop, first, n // 3, guard).tobytes() == a[:n // 3].tobytes()


def test_unpack_convention(dev, cap):
    try:
        dev.set_unpack(128.0, 1.0 / 128.0)
        with dev.capture(np.full(2 * 5000, 128, np.uint8)) as flat:
            for nfft in (16, 256, 2048):
                n = gpsjam.ridge_frames(flat.nbytes, 1, nfft, nfft // 2)
                got = run(dev, flat, flat.nbytes, nfft, nfft // 2, 1, n, 2)
                assert not got["total"].any() and not got["peak"].any() and not got["second"].any() and not got["peak_bin"].any()
        for nfft in rr.PARITY_NFFT:
            hop = nfft // 2 + 37
            want, _ = rr.parity_reference(nfft, hop, 1, 2, 128.0, 1.0 / 128.0)
            rr.compare(run(dev, cap, cap.nbytes, nfft, hop, 1, want.size, 2), want, (nfft, "gnssdec convention"))
    finally:
        dev.set_unpack()
    assert dev.get_unpack() == (127.5, 1.0 / 127.5)
    want, _ = rr.parity_reference(256, 128, 0, 2)
    rr.compare(run(dev, cap, cap.nbytes, 256, 128, 0, want.size, 2), want, "default convention restored")


def test_refusals_enqueue_nothing(dev, cap):
    fit = gpsjam.ridge_frames(cap.nbytes, 0, 256, 128)
    cases = [  # nfft, hop, first, n_frames, guard, status
        (8, 4, 0, 4, 0, GJ_ERR_UNSUPPORTED), (8192, 4096, 0, 4, 2, GJ_ERR_UNSUPPORTED), (48, 24, 0, 4, 2, GJ_ERR_UNSUPPORTED),
        (256, 0, 0, 4, 2, GJ_ERR_INVALID),
        (256, 128, 0, 4, 128, GJ_ERR_INVALID), (256, 128, 0, 4, -1, GJ_ERR_INVALID), (16, 8, 0, 4, 8, GJ_ERR_INVALID),
        (256, 128, 0, 0, 2, GJ_ERR_INVALID), (256, 128, 0, fit + 1, 2, GJ_ERR_INVALID),
        (256, 128, cap.nsamples, 1, 2, GJ_ERR_INVALID),
    ]
    out = Guarded(dev, (fit + 1) * REC, pad=64 * REC)
    try:
        calls = [((cap, cap.nbytes, first, nfft, hop, n_frames, guard, out), status) for nfft, hop, first, n_frames, guard, status in cases]
        refused(dev, dev.ridge_dev, calls + [((0, cap.nbytes, 0, 256, 128, 4, 2, out), GJ_ERR_INVALID)], out)
        # guard at its largest (2 guard + 1 < nfft) and a call that just fits are accepted
        dev.ridge_dev(cap, cap.nbytes, 0, 16, 8, 4, 7, out)
        dev.ridge_dev(cap, cap.nbytes, 0, 256, 128, fit, 2, out)
        dev.synchronize()
        out.check_pads("records")
    finally:
        out.free()


def test_device_ridge_takes_host_bytes_and_captures(dev, cap):
    want, _ = rr.parity_reference(256, 128, 0, 2)
    a = dev.ridge(cap)
    b = dev.ridge(rr.parity_capture(), nfft=256, hop=128, guard=2)
    assert (a.nfft, a.hop, a.first_sample, a.guard, len(a)) == (256, 128, 0, 2, want.size)
    assert a.records.tobytes() == b.records.tobytes()
    rr.compare(a.records, want, "Device.ridge")
    part = dev.ridge(cap, nfft=64, hop=100, first_sample=5, n_frames=10, guard=1)
    assert len(part) == 10 and part[4:].first_sample == 405
    np.testing.assert_allclose(a.concentration, want["peak"] / want["total"], rtol=3e-5)
    assert len(dev.ridge(np.zeros(100, np.uint8))) == 0


@pytest.mark.parametrize("case", rr.CASES)
def test_characterise_end_to_end(dev, case):
    with dev.capture(rr.classifier_capture(case)) as c:
        res = classify.characterise(dev, c, fs=rr.FS, nfft=256, **rr.ONSET_ARGS)
    if case == "none":
        assert res.evidence["onset"] == -1
    else:
        half = rr.CLASSIFIER_SAMPLES // 2
        assert half - 1000 <= res.evidence["onset"] <= half + 1000, res.evidence
        assert res.evidence["floor_from"] == "noise frames"
    rr.check_interference(case, res)
