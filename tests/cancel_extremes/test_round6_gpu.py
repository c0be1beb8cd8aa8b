"""The two cancellers (gj_cancel_dev, gj_cancel2_dev) where they alone among the cleaners can go wrong: weights of modulus
above 1, which make samples larger than the input and drive the output clamp from both sides; the saturated and
degenerate captures of tests/extremes_inputs.py in the roles a | b (| c), frames without any power among them; capture
ranges past byte 2^32; frames_per_set and n_sets at the ends of size_t; and the host's singular-matrix branch fed from
the device's own sums.

This file sits in a package of its own for the reason tests/cancel/test_round6_gpu.py gives: the suite orders GPU files
by basename (tests/conftest.py SUITE_ORDER), and under this name it runs in stage 2.

Yardsticks: a closed form with no transform in it (constant weights), the float64 restatements of
tests/cancel_restatement.py and tests/cancel2_restatement.py, and bit-identity between calls that the header defines as
equal -- never the GPU's own result.  The tie bands, record tolerances and thresholds are those of
tests/cancel_extremes_inputs.py, each measured and asserted on the CPU by tests/test_cancel_extremes_host.py.  Every
gj_cancel*_dev call goes through the run() helpers of the two canceller files: sentinel-filled buffers, nothing written
behind d_out[2 n_samples] or d_frames[F]."""
import numpy as np
import pytest

import cancel2_restatement as c2
import cancel_extremes_inputs as ce
import cancel_restatement as cr
import excise_restatement as er
import extremes_inputs as xi
import gpsjam
from gpsjam import _bands, coherence
from gpu_lib import GJ_ERR_INVALID, Convention, Guarded, Resident, freed, refused, run_cancel, run_cancel2

pytestmark = pytest.mark.gpu

REC = gpsjam.CANCEL_DTYPE.itemsize
f32 = c2.f32


@pytest.fixture(scope="module")
def res(dev):
    r = Resident(dev)
    yield r
    r.free()


@pytest.fixture(scope="module")
def caps(dev):
    """Host bytes resident once, uploaded on first use."""
    held = {}

    def get(raw):
        key = raw.tobytes()
        if key not in held:
            held[key] = dev.capture(raw)
        return held[key]
    yield get
    for c in held.values():
        c.free()


def run(dev, captures, firsts, n_samples, nfft, d_w, frames_per_set, n_sets, d_thr):
    """(bytes, records) through gj_cancel_dev for a pair and gj_cancel2_dev for a triple, by gpu_lib's run_cancel and run_cancel2."""
    if len(captures) == 2:
        (a, b), (fa, fb) = captures, firsts[:2]
        return run_cancel(dev, a, a.nbytes, fa, b, b.nbytes, fb, n_samples, nfft, d_w, frames_per_set, n_sets, d_thr)
    return run_cancel2(dev, tuple(captures), tuple(firsts), n_samples, nfft, d_w, frames_per_set, n_sets, d_thr)


def compare(got, rec, want, d_f, band, tol, what):
    """GPU bytes and records against a cr.Cancelled: the mask's count on every frame; total_in within tol of the restated
    total_in, total and removed within tol of D_f, element by element and without a division, so that a frame without
    power must give exact zeros; the copied edges; bytes within 1 everywhere and equal outside the tie band.  Returns the
    share of values inside the band."""
    assert rec.size == want.records.size and got.size == want.out.size, what
    np.testing.assert_array_equal(rec["n_excised"], want.records["n_excised"], err_msg=str(what))
    print(f"{what}: records within {ce.record_ratio(rec, want.records, d_f):.2e} (tolerance {tol:.2e})")
    assert ce.record_errors(rec, want.records, d_f, tol) == [], what
    quiet = want.records["total_in"] == 0
    none = quiet & (d_f == 0)
    assert not rec["total_in"][quiet].any(), (what, "total_in of a frame without power in a")
    for key in ("total", "removed", "n_excised"):
        assert not rec[key][none].any(), (what, key, "a frame without any power")
    assert np.array_equal(got[:want.lo], want.out[:want.lo]) and np.array_equal(got[want.hi:], want.out[want.hi:]), (what, "edges")
    body, ref = got[want.lo:want.hi].astype(np.int16), want.out[want.lo:want.hi].astype(np.int16)
    clear = er.tie_distance(want.value) > band
    diff = np.abs(body - ref)
    share = float(np.mean(~clear))
    print(f"{what}: {int(np.sum(diff != 0))} of {diff.size} bytes differ, {int(np.sum(~clear))} lie in the tie band ({share:.2e}), "
          f"{int(np.sum((ref == 0) | (ref == 255)))} on a rail")
    assert not diff[clear].any(), (what, int(np.sum(diff[clear] != 0)), "bytes differ outside the tie band")
    assert diff.max(initial=0) <= 1, (what, int(diff.max()))
    return share


# ------------------------------------------------------------------------------------------- 1. constant weights
@pytest.mark.parametrize("nfft", ce.CLOSED_NFFT)
def test_constant_weights_have_a_closed_form(dev, caps, res, nfft):
    """W = c on every bin and no bin cut: y = x_a - c x_b (- c2 x_c) on samples [N/2, F N/2), integers all, of which 12 %
    to 48 % lie beyond each rail (tests/test_cancel_extremes_host.py).  Byte for byte, with no tie band."""
    captures = [caps(raw) for raw in ce.closed_captures()]
    inf = res(np.full(nfft, np.inf))
    n = ce.CLOSED_SAMPLES
    for cases, n_aux in ((ce.CLOSED_CASES, 1), (ce.CLOSED_CASES2, 2)):
        for i, (c, offset, scale) in enumerate(cases):
            want_bytes = ce.closed_bytes(c, offset, nfft)
            want, d_f = ce.closed_reference(c, offset, scale, nfft)
            shapes = [(1, ce.FRAMES_PER_SET)] + ([(3, ce.FRAMES_PER_SET)] if i == ce.CLOSED_THREE_SETS else [])
            for n_sets, fps in shapes:
                what = (c, offset, nfft, n_sets)
                with Convention(dev, offset, scale):
                    got, rec = run(dev, captures[:1 + n_aux], ce.FIRSTS, n, nfft, res(f32(ce.closed_weights(c, nfft, n_sets))), fps, n_sets, inf)
                differ = np.flatnonzero(got != want_bytes)
                assert differ.size == 0, (what, differ.size, "bytes differ from clip(rint(closed form))", differ[:4].tolist(),
                                          got[differ[:4]].tolist(), want_bytes[differ[:4]].tolist())
                assert (got[want.lo:want.hi] == 0).mean() >= ce.CLOSED_RAIL_SHARE_MIN and (got[want.lo:want.hi] == 255).mean() >= ce.CLOSED_RAIL_SHARE_MIN
                assert not rec["n_excised"].any() and not rec["removed"].any(), what
                print(f"{what}: records within {ce.record_ratio(rec, want.records, d_f):.2e} (tolerance {ce.closed_record_tol(nfft):.2e})")
                assert ce.record_errors(rec, want.records, d_f, ce.closed_record_tol(nfft)) == [], what


# ------------------------------------------------------------------------------ 2. extreme captures, |W| up to 4
@pytest.mark.parametrize("nfft", ce.EXTREME_NFFT)
@pytest.mark.parametrize("names", ce.PAIRS + ce.TRIPLES, ids=" | ".join)
def test_extreme_captures_under_large_weights(dev, caps, res, names, nfft):
    """Both conventions, the case's own thresholds and +inf; weights of modulus up to 4, a set per five frames."""
    captures = [caps(xi.capture(name)) for name in names]
    w = ce.extreme_weights(len(names) - 1, nfft)
    d_w = res(f32(w))
    for offset, scale in ce.CONVENTIONS:
        for kind in ce.KINDS:
            thr = ce.extreme_threshold(names, nfft, offset, scale, kind)
            want, d_f = ce.extreme_reference(names, nfft, offset, scale, kind)
            what = (names, nfft, offset, kind)
            with Convention(dev, offset, scale):
                got, rec = run(dev, captures, ce.FIRSTS, ce.EXTREME_SAMPLES, nfft, d_w, ce.FRAMES_PER_SET, w.shape[0],
                               res(np.full(nfft, np.inf) if thr is None else thr))
            share = compare(got, rec, want, d_f, ce.tie_band(nfft), ce.record_tol(nfft), what)
            assert (share <= ce.TIE_SHARE_MAX) == ce.under_the_cap(names, nfft, offset, kind), (what, share)
            if kind == "cut":
                assert want.cut.any() and not want.cut.all()
            else:
                assert not rec["n_excised"].any() and not rec["removed"].any(), what
            none = (want.records["total_in"] == 0) & (d_f == 0)
            h = nfft // 2
            for f in np.flatnonzero(none[:-1] & none[1:])[:64]:       # hop f + 1 is the sum of frames f and f + 1: mid-level
                assert np.all(got[2 * (f + 1) * h:2 * (f + 2) * h] == 128), (what, int(f))


# ------------------------------------------------------------------------------ 3. past byte 2^32
@pytest.fixture(scope="module")
def far(dev):
    """(big, small): one allocation of 4 GiB + 1 MiB, never filled, with ce.far_capture() at byte 2^32, and the same
    bytes as a capture of their own."""
    raw = ce.far_capture()
    small = dev.capture(raw)
    big = dev.alloc(ce.FAR_BYTES)
    try:
        assert big.ptr and big.nbytes == ce.FAR_BYTES
        big.upload(raw, offset=2 * ce.FAR_S0)
        assert big.download(np.uint8, 64, offset=2 * ce.FAR_S0).tobytes() == raw[:64].tobytes()
        yield big, small
    finally:
        big.free()
        small.free()


def refused_and_wrote_nothing(dev, launch, args_of, n_samples, nfft):
    """launch(*args_of(out, rec)) is GJ_ERR_INVALID and leaves sentinel-filled buffers as they were."""
    out, rec = Guarded(dev, 2 * n_samples), Guarded(dev, gpsjam.excise_frames(n_samples, nfft) * REC)
    try:
        refused(dev, launch, [(args_of(out, rec), GJ_ERR_INVALID)], out, rec)
    finally:
        freed(out, rec)


@pytest.mark.parametrize("nfft", ce.FAR_NFFT)
@pytest.mark.parametrize("n_aux", (1, 2))
def test_past_byte_2_32(dev, far, res, n_aux, nfft):
    """a, b (and c) are the windows at samples 2^31 + 1, 2^31 + 4 (and 2^31 + 9) of the big allocation: the bits of the
    same bytes uploaded as a small capture, which give the restatement's result by the parity comparison."""
    big, small = far
    mod = cr if n_aux == 1 else c2
    n, fps, s0 = ce.FAR_SAMPLES, cr.PARITY_FRAMES_PER_SET, ce.FAR_S0
    w = mod.parity_weights(nfft)
    d_w, n_sets, d_thr = res(f32(w)), w.shape[0], res(ce.far_threshold(n_aux, nfft))
    firsts = ce.FIRSTS[:1 + n_aux]
    assert 2 * (s0 + firsts[0]) > 2 ** 32 and 2 * (s0 + firsts[-1] + n) <= ce.FAR_BYTES and firsts[-1] + n <= small.nsamples

    def call(*where):
        """where: per capture, True for the window inside the big allocation."""
        return run(dev, [big if far_ else small for far_ in where], [s0 + f if far_ else f for far_, f in zip(where, firsts)], n, nfft,
                   d_w, fps, n_sets, d_thr)

    near_b, near_r = call(*[False] * (1 + n_aux))
    mod.compare(near_b, near_r, ce.far_reference(n_aux, nfft), (n_aux, nfft, "the window as a capture of its own"))
    mixes = [[True] * (1 + n_aux)] + [[i == j for j in range(1 + n_aux)] for i in range(1 + n_aux)]
    if n_aux == 1:
        assert mixes == [[True, True], [True, False], [False, True]]
    for where in mixes:
        got_b, got_r = call(*where)
        assert got_b.tobytes() == near_b.tobytes() and got_r.tobytes() == near_r.tobytes(), (n_aux, nfft, where)
    # a range that ends one sample past the big allocation, in any one of the captures
    launch = dev.cancel_dev if n_aux == 1 else dev.cancel2_dev
    for i in range(1 + n_aux):
        at = [s0 + f for f in firsts]
        at[i] = ce.FAR_BYTES // 2 - n + 1
        ins = [v for f in at for v in (big, ce.FAR_BYTES, f)]
        refused_and_wrote_nothing(dev, launch, lambda out, rec: (*ins, n, nfft, d_w, fps, n_sets, d_thr, out, rec), n, nfft)


# ------------------------------------------------------------------------------ 4. size_t's ends
@pytest.mark.parametrize("n_aux", (1, 2))
def test_set_arithmetic_at_the_ends_of_size_t(dev, caps, res, n_aux):
    """set(f) = min(f // frames_per_set, n_sets - 1) at frames_per_set = 2^64 - 1 and at a set per frame with more sets
    than frames: bit for bit what the same sets give at ordinary values."""
    nfft = ce.SET_NFFT
    mod = cr if n_aux == 1 else c2
    raws = cr.parity_pair() if n_aux == 1 else c2.parity_triple()
    captures = [caps(raw) for raw in raws]
    firsts = (c2.PARITY_FIRST_A, c2.PARITY_FIRST_B, c2.PARITY_FIRST_C)
    n = cr.PARITY_SAMPLES
    nf = gpsjam.excise_frames(n, nfft)
    w = mod.parity_weights(nfft)
    d_w, d_thr = res(f32(w)), res(mod.parity_threshold(nfft))
    assert w.shape[0] >= 3 and nf == 255

    def call(d_sets, fps, n_sets):
        return run(dev, captures, firsts, n, nfft, d_sets, fps, n_sets, d_thr)

    ref_b, ref_r = call(d_w, nf, 1)
    assert ref_r["n_excised"].any() and np.all(ref_r["total"] > 0)
    for fps, n_sets in ((2 ** 64 - 1, 1), (2 ** 64 - 1, 3), (1, 1)):
        got_b, got_r = call(d_w, fps, n_sets)
        assert got_b.tobytes() == ref_b.tobytes() and got_r.tobytes() == ref_r.tobytes(), (n_aux, fps, n_sets)
    # a set per frame, and three sets of NaN behind the F-th: set(f) <= F - 1, they are never read
    per = ce.per_frame_weights(n_aux, nfft, nf, 3)
    each_b, each_r = call(res(f32(per[:nf])), 1, nf)
    assert each_r.tobytes() != ref_r.tobytes() and each_b.tobytes() != ref_b.tobytes()
    got_b, got_r = call(res(f32(per)), 1, nf + 3)
    assert got_b.tobytes() == each_b.tobytes() and got_r.tobytes() == each_r.tobytes(), (n_aux, "sets behind the last frame's")
    for key in ("total_in", "total", "removed"):
        assert np.isfinite(got_r[key]).all(), (n_aux, key)
    # the first five frames of a set per frame are those of five frames per set wherever the sets agree: frame 0 in both
    five_b, five_r = call(d_w, cr.PARITY_FRAMES_PER_SET, w.shape[0])
    assert each_r[:1].tobytes() == five_r[:1].tobytes()


# ------------------------------------------------------------------------------ 5. one degenerate chain
def test_a_repeated_auxiliary_is_the_two_antenna_canceller(dev, caps):
    """The device's sums of (a, b, b) through the host's singular-matrix branch: every flagged cell falls back to b, every
    W2 is exactly 0, and Device.cancel2 writes what Device.cancel(a, b, W1) writes -- the header's W2 = 0 anchor."""
    a, b, _ = (caps(raw) for raw in c2.parity_triple())
    nfft, m = 256, 16
    matrix = coherence.spectral_matrix(dev, a, b, b, nfft=nfft, frames_per_row=m)
    assert len(matrix.ab) >= 8 and matrix.ac.sab.tobytes() == matrix.ab.sab.tobytes() and matrix.ac.sbb.tobytes() == matrix.ab.sbb.tobytes()
    flagged = np.abs(_bands.signed_bins(nfft)) > 1
    w = coherence.cancel_weights2(matrix, flagged)
    assert w.shape == (len(matrix.ab), 2, nfft) and w.dtype == np.complex64
    assert not w[:, 1].any(), "W2 is exactly 0 in every cell"
    assert np.all(w[:, 0][:, flagged] != 0) and not w[:, 0][:, ~flagged].any()
    assert w[:, 0].tobytes() == coherence.cancel_weights(matrix.ab, coherence.Detection(flagged, 0.0, 1e-6)).tobytes(), "every flagged cell fell back to b"
    thr = c2.parity_threshold(nfft)
    x, rec_x = dev.cancel2(a, b, b, w, thr, nfft=nfft, frames_per_set=2 * m)
    y, rec_y = dev.cancel(a, b, np.ascontiguousarray(w[:, 0]), thr, nfft=nfft, frames_per_set=2 * m)
    try:
        assert x.nbytes == y.nbytes == 2 * min(a.nsamples, b.nsamples) and rec_x.size == gpsjam.excise_frames(x.nsamples, nfft)
        assert x.download().tobytes() == y.download().tobytes(), "bytes of Device.cancel"
        assert rec_x.tobytes() == rec_y.tobytes(), "records of Device.cancel"
        assert rec_x["n_excised"].any() and rec_x["total"].sum() < rec_x["total_in"].sum(), "the mask cut something, the weights cancelled something"
    finally:
        x.free()
        y.free()
