"""The chirp-rate search (gj_chirp_dev, Device.chirp) and classify.characterise_swept on the GPU.

This file sits in a package of its own for the reason tests/ridge/test_round6_gpu.py gives: the suite orders GPU files by
basename (tests/conftest.py SUITE_ORDER), and under this name it runs in stage 2, behind the parity tests of K2.

Yardstick: the float64 restatement of the definition in include/gpsjam.h (tests/chirp_restatement.py).  rate_index and
peak_bin are equal on EVERY frame (tests/test_chirp_host.py shows that no frame of any input used here beats its
runner-up rate or bin by less than 1e-4); total and peak within rtol 1e-5, the project's figure for a K2 value summed in
another order, which a float32 evaluation of the definition stays inside by a factor of 25 (same file); second within
1e-5 * peak.  The single rate 0 against gj_ridge_dev, d_peaks against single-rate calls, translation and repetition are
bit-exact."""
import numpy as np
import pytest

import chirp_restatement as cr
import gpsjam
import ridge_restatement as rr
from gpsjam import classify
from gpu_lib import GJ_ERR_INVALID, GJ_ERR_UNSUPPORTED, Guarded, freed, refused
from gpu_lib import run_chirp as run

pytestmark = pytest.mark.gpu

REC = gpsjam.CHIRP_DTYPE.itemsize
RTOL = cr.RTOL


@pytest.fixture(scope="module")
def caps(dev):
    """parity_capture(nfft) resident, one per size, uploaded on first use."""
    held = {}

    def get(nfft):
        if nfft not in held:
            held[nfft] = dev.capture(cr.parity_capture(nfft))
        return held[nfft]
    yield get
    for c in held.values():
        c.free()


@pytest.mark.parametrize("nfft", cr.PARITY_NFFT)
def test_parity_with_the_restatement(dev, caps, nfft):
    cap = caps(nfft)
    for rates in cr.parity_rate_sets(nfft):
        for first in (0, 1):
            want = cr.parity_reference(nfft, rates, first)
            got, peaks = run(dev, cap, cap.nbytes, nfft, cr.parity_hop(nfft), first, want.records.size, rates)
            cr.compare(got, peaks, want, (nfft, rates, first))
    # guard 0: only `second` changes
    want = cr.parity_reference(nfft, (-3, 2, 5), 1, 0)
    got, _ = run(dev, cap, cap.nbytes, nfft, cr.parity_hop(nfft), 1, want.records.size, (-3, 2, 5), guard=0, want_peaks=False)
    cr.compare(got, None, want, (nfft, "guard 0"))
    print(f"nfft {nfft}: largest relative errors so far {cr.WORST} (tolerance {RTOL:.0e})")


@pytest.mark.parametrize("nfft", [64, 1024, 4096])
def test_single_rate_zero_is_gj_ridge_dev_byte_for_byte(dev, caps, nfft):
    cap, hop = caps(nfft), cr.parity_hop(nfft)
    for first in (0, 1):
        n = gpsjam.ridge_frames(cap.nbytes, first, nfft, hop)
        got, peaks = run(dev, cap, cap.nbytes, nfft, hop, first, n, (0, 1, 1))
        out = dev.alloc(n * gpsjam.RIDGE_DTYPE.itemsize)
        try:
            dev.ridge_dev(cap, cap.nbytes, first, nfft, hop, n, 2, out)
            ridge = out.download(np.uint8)
        finally:
            out.free()
        head = np.ascontiguousarray(got.view(np.uint8).reshape(n, REC)[:, :16])
        assert head.tobytes() == ridge.tobytes(), (nfft, first)
        assert not got["rate_index"].any()
        assert peaks[:, 0].tobytes() == got["peak"].tobytes()


@pytest.mark.parametrize("nfft", [32, 256, 2048])
def test_peaks_equal_single_rate_calls_bit_for_bit(dev, caps, nfft):
    """Anything carried from one rate to the next would show here: the five rates one by one against the call with all."""
    cap, rates, hop, first = caps(nfft), (-3, 2, 5), cr.parity_hop(nfft), 1
    n = gpsjam.ridge_frames(cap.nbytes, first, nfft, hop)
    full, peaks = run(dev, cap, cap.nbytes, nfft, hop, first, n, rates)
    for r, q in enumerate(cr.rate_values(rates)):
        one, p1 = run(dev, cap, cap.nbytes, nfft, hop, first, n, (q, 1, 1))
        assert one["peak"].tobytes() == peaks[:, r].tobytes() == p1[:, 0].tobytes(), (nfft, q)
        won = full["rate_index"] == r
        a, b = full[won], one[won]
        for key in ("total", "peak", "second", "peak_bin"):
            assert a[key].tobytes() == b[key].tobytes(), (nfft, q, key)
    # d_peaks = NULL: the same records
    again, none = run(dev, cap, cap.nbytes, nfft, hop, first, n, rates, want_peaks=False)
    assert none is None and again.tobytes() == full.tobytes()


@pytest.mark.parametrize("nfft", cr.PARITY_NFFT)
def test_frame_counts_that_do_not_fill_a_workgroup_step(dev, caps, nfft):
    per_step = 4096 // nfft
    hop, first, rates = cr.parity_hop(nfft), 1, (-3, 2, 5)
    raw, cap = cr.parity_capture(nfft), caps(nfft)
    for n_frames in sorted({1, per_step - 1, per_step + 1, 2 * per_step + 3} - {0}):
        # exactly all that fit: the last frame ends on the capture's last byte
        nbytes = 2 * (first + (n_frames - 1) * hop + nfft)
        assert gpsjam.ridge_frames(nbytes, first, nfft, hop) == n_frames and gpsjam.ridge_frames(nbytes - 2, first, nfft, hop) == n_frames - 1
        with dev.capture(raw[:nbytes]) as exact:
            got, peaks = run(dev, exact, nbytes, nfft, hop, first, n_frames, rates)
        want = cr.parity_reference(nfft, rates, first)
        head = cr.Scan(want.records[:n_frames], want.peaks[:n_frames], None, None)
        cr.compare(got, peaks, head, (nfft, n_frames, "exact"))
        # the same frames as the head of the long capture: same bits
        long, lpeaks = run(dev, cap, cap.nbytes, nfft, hop, first, n_frames, rates)
        assert long.tobytes() == got.tobytes() and lpeaks.tobytes() == peaks.tobytes(), (nfft, n_frames)


@pytest.mark.parametrize("nfft", [64, 1024, 2048, 4096])
def test_translation_invariance_and_repeatability_are_bit_exact(dev, caps, nfft):
    cap, hop, first, rates = caps(nfft), cr.parity_hop(nfft), 1, (-3, 2, 5)
    n = gpsjam.ridge_frames(cap.nbytes, first, nfft, hop)
    a, pa = run(dev, cap, cap.nbytes, nfft, hop, first, n, rates)
    b, pb = run(dev, cap, cap.nbytes, nfft, hop, first, n, rates)
    assert a.tobytes() == b.tobytes() and pa.tobytes() == pb.tobytes()
    for k in (1, 4096 // nfft + 1, 7):
        b, pb = run(dev, cap, cap.nbytes, nfft, hop, first + k * hop, n - k, rates)
        assert b.tobytes() == a[k:].tobytes() and pb.tobytes() == pa[k:].tobytes(), (nfft, k)
    # fewer frames in the call: another grid, the same bits
    b, pb = run(dev, cap, cap.nbytes, nfft, hop, first, n // 3, rates)
    assert b.tobytes() == a[:n // 3].tobytes() and pb.tobytes() == pa[:n // 3].tobytes()


def test_unpack_convention(dev):
    nfft, rates, first = 256, (-3, 2, 5), 1
    with dev.capture(cr.parity_capture(nfft)) as cap:
        try:
            dev.set_unpack(128.0, 1.0 / 128.0)
            with dev.capture(np.full(2 * 5000, 128, np.uint8)) as flat:
                n = gpsjam.ridge_frames(flat.nbytes, 1, nfft, 128)
                got, peaks = run(dev, flat, flat.nbytes, nfft, 128, 1, n, rates)
                assert not got["total"].any() and not got["peak"].any() and not got["peak_bin"].any() and not got["rate_index"].any()
                assert not peaks.any()
            want = cr.parity_reference(nfft, rates, first, 2, 128.0, 1.0 / 128.0)
            got, peaks = run(dev, cap, cap.nbytes, nfft, cr.parity_hop(nfft), first, want.records.size, rates)
            cr.compare(got, peaks, want, "gnssdec convention")
        finally:
            dev.set_unpack()
        assert dev.get_unpack() == (127.5, 1.0 / 127.5)
        want = cr.parity_reference(nfft, rates, first)
        got, peaks = run(dev, cap, cap.nbytes, nfft, cr.parity_hop(nfft), first, want.records.size, rates)
        cr.compare(got, peaks, want, "default convention restored")


def test_refusals_enqueue_nothing(dev, caps):
    cap = caps(64)
    fit = gpsjam.ridge_frames(cap.nbytes, 0, 256, 128)
    ok = (0, 1, 1)
    cases = [  # nfft, hop, first, n_frames, guard, (rate_first, rate_step, n_rates), status
        (256, 128, 0, 4, 2, (0, 1, 0), GJ_ERR_INVALID), (256, 128, 0, 4, 2, (0, 1, 257), GJ_ERR_UNSUPPORTED),
        (256, 128, 0, 4, 2, (0, 0, 2), GJ_ERR_INVALID), (256, 128, 0, 4, 2, (0, -1, 2), GJ_ERR_INVALID),
        (256, 128, 0, 4, 2, (32768 - 1, 2, 2), GJ_ERR_INVALID), (256, 128, 0, 4, 2, (-32769, 1, 2), GJ_ERR_INVALID),
        (16, 8, 0, 4, 2, (129, 1, 1), GJ_ERR_INVALID), (4096, 2048, 0, 4, 2, (-8388609, 1, 1), GJ_ERR_INVALID),
        (8, 4, 0, 4, 0, ok, GJ_ERR_UNSUPPORTED), (8192, 4096, 0, 4, 2, ok, GJ_ERR_UNSUPPORTED), (48, 24, 0, 4, 2, ok, GJ_ERR_UNSUPPORTED),
        (256, 0, 0, 4, 2, ok, GJ_ERR_INVALID),
        (256, 128, 0, 4, 128, ok, GJ_ERR_INVALID), (256, 128, 0, 4, -1, ok, GJ_ERR_INVALID), (16, 8, 0, 4, 8, ok, GJ_ERR_INVALID),
        (256, 128, 0, 0, 2, ok, GJ_ERR_INVALID), (256, 128, 0, fit + 1, 2, ok, GJ_ERR_INVALID),
        (256, 128, cap.nsamples, 1, 2, ok, GJ_ERR_INVALID),
    ]
    out, pk = Guarded(dev, (fit + 1) * REC, pad=64 * REC), Guarded(dev, (fit + 1) * 2 * 4)
    try:
        calls = [((cap, cap.nbytes, first, nfft, hop, n_frames, guard, q0, dq, nq, out, pk), status)
                 for nfft, hop, first, n_frames, guard, (q0, dq, nq), status in cases]
        for d_iq, d_out, d_pk in ((0, out, pk), (cap, 0, pk), (cap.ptr + 1, out, pk), (cap, out.ptr + 2, pk), (cap, out, pk.ptr + 2)):
            calls.append(((d_iq, cap.nbytes - 2, 0, 256, 128, 4, 2, 0, 1, 1, d_out, d_pk), GJ_ERR_INVALID))
        refused(dev, dev.chirp_dev, calls, out, pk)
        # the limits themselves are accepted: 256 rates, both ends of the rate range, the largest guard, every frame that fits
        big = dev.alloc(4 * 256 * 4)
        try:
            dev.chirp_dev(cap, cap.nbytes, 0, 256, 128, 4, 2, -128, 1, 256, out, big)
            dev.chirp_dev(cap, cap.nbytes, 0, 256, 128, 4, 2, -32768, 65536, 2, out, pk)
            dev.chirp_dev(cap, cap.nbytes, 0, 16, 8, 4, 7, 128, 1, 1, out, None)
            dev.chirp_dev(cap, cap.nbytes, 0, 4096, 2048, 1, 2, -8388608, 1, 1, out, None)
            dev.chirp_dev(cap, cap.nbytes, 0, 256, 128, fit, 2, 0, 1, 2, out, pk)
            dev.synchronize()
            out.check_pads("records")
            pk.check_pads("peaks")
        finally:
            big.free()
    finally:
        freed(out, pk)
        pk.free()


def test_device_chirp_takes_host_bytes_and_captures(dev, caps):
    nfft, rates = 64, (-3, 2, 5)
    cap, hop = caps(nfft), cr.parity_hop(nfft)
    want = cr.parity_reference(nfft, rates, 0)
    a = dev.chirp(cap, nfft=nfft, hop=hop, rates=rates, want_peaks=True)
    b = dev.chirp(cr.parity_capture(nfft), nfft=nfft, hop=hop, rates=rates, guard=2)
    assert (a.nfft, a.hop, a.first_sample, a.guard, a.rates, len(a)) == (nfft, hop, 0, 2, rates, want.records.size)
    assert a.records.tobytes() == b.records.tobytes() and b.peaks is None
    cr.compare(a.records, a.peaks, want, "Device.chirp")
    np.testing.assert_array_equal(a.rate, -3 + 2 * want.records["rate_index"])
    part = dev.chirp(cap, nfft=nfft, hop=100, rates=(1, 1, 2), first_sample=5, n_frames=10, guard=1)
    assert len(part) == 10 and part[4:].first_sample == 405 and part.hop == 100
    np.testing.assert_allclose(a.concentration, want.records["peak"] / want.records["total"], rtol=3e-5)
    empty = dev.chirp(np.zeros(100, np.uint8), rates=rates, want_peaks=True)
    assert len(empty) == 0 and empty.peaks.shape == (0, 5)
    assert len(dev.chirp(cap, nfft=256).records) == gpsjam.ridge_frames(cap.nbytes, 0, 256, 128)      # the defaults: rate 0 alone


def test_characterise_swept_finds_the_fast_chirp(dev):
    with dev.capture(cr.fast_chirp_capture()) as c:
        plain = classify.characterise(dev, c, fs=cr.FS, nfft=256, **rr.ONSET_ARGS)
        res = classify.characterise_swept(dev, c, fs=cr.FS, nfft=256, max_sweep_hz_per_s=2.0e9, **rr.ONSET_ARGS)
    assert plain.kind == "broadband", plain                 # what the ridge alone says
    assert res.kind == "chirp", res
    print(f"fast chirp: {res.sweep_hz_per_s:.4g} Hz/s against {cr.FAST_SWEEP:.4g}; one unit is {cr.RATE_UNIT:.4g}")
    assert abs(res.sweep_hz_per_s - cr.FAST_SWEEP) <= cr.RATE_UNIT, res
    half = rr.CLASSIFIER_SAMPLES // 2
    assert half - 1000 <= res.evidence["onset"] <= half + 1000
    assert res.evidence["rates"] == (-32, 1, 65) and res.evidence["ridge"]["concentration"] == plain.evidence["concentration"]
    assert res.evidence["floor_from"] == "noise frames"


@pytest.mark.parametrize("case", ["chirp", "cw", "pulsed", "none"])
def test_characterise_swept_leaves_the_other_kinds_alone(dev, case):
    """The simulator-rate chirp, the tone, the pulse train and the noise-only capture: exactly characterise's answer."""
    with dev.capture(rr.classifier_capture(case)) as c:
        plain = classify.characterise(dev, c, fs=rr.FS, nfft=256, **rr.ONSET_ARGS)
        calls = dict(dev.kernel_calls)
        res = classify.characterise_swept(dev, c, fs=rr.FS, nfft=256, **rr.ONSET_ARGS)
    assert res.kind == plain.kind == case
    assert res[:6] == plain[:6] and res.evidence == plain.evidence
    assert dev.kernel_calls.get("chirp", 0) == calls.get("chirp", 0), "the search ran although the ridge's answer stood"
    rr.check_interference(case, res)


def test_characterise_swept_keeps_gaussian_broadband(dev):
    with dev.capture(rr.classifier_capture("broadband")) as c:
        res = classify.characterise_swept(dev, c, fs=rr.FS, nfft=256, max_sweep_hz_per_s=2.0e9, **rr.ONSET_ARGS)
    rr.check_interference("broadband", res)
    assert res.evidence["swept"]["dechirped_line"] is False and res.evidence["swept"]["rates"] == (-32, 1, 65)
