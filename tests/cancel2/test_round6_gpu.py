"""The three-antenna per-bin canceller (gj_cancel2_dev, Device.cancel2, gpsjam.mitigate.clean_spatial2) on the GPU.

This file sits in a package of its own on purpose, as tests/cancel/ does: the suite orders GPU files by basename
(tests/conftest.py SUITE_ORDER, which tests/test_suite_order.py holds every GPU file to), and under the name
test_round6_gpu.py it runs in stage 2, behind the parity tests of K2 whose transform it shares.

Yardstick: the float64 restatement of the definition in include/gpsjam.h (tests/cancel2_restatement.py).  The mask is
equal on EVERY bin of every frame (tests/test_cancel2_host.py shows that no input has a bin within 1e-4 of its
threshold); total_in, total and removed within rtol 1e-5 of total_in; bytes equal wherever the float64 value is further
than TIE_BAND from a rounding tie and within 1 elsewhere.  The anchors (W2 = 0 and W1 = 0 against gj_cancel_dev, both 0
against gj_excise_dev, a capture against itself in halves, every bin cut), translation, repetition and the run seams are
bit-exact.  Every call writes into sentinel-filled buffers whose bytes behind 2 * n_samples and behind d_frames[F] must
stay untouched."""
import numpy as np
import pytest

import cancel2_restatement as c2
import cancel_restatement as cr
import excise_restatement as er
import gpsjam
import stft_scale_inputs as si
from gpsjam import gnss, mitigate
from gpu_lib import GJ_ERR_INVALID, GJ_ERR_UNSUPPORTED, Guarded, Resident, freed, refused, run_cancel, run_excise
from gpu_lib import run_cancel2 as run

pytestmark = pytest.mark.gpu

REC = gpsjam.CANCEL_DTYPE.itemsize
RTOL = cr.RTOL
FA, FB, FC, N = c2.PARITY_FIRST_A, c2.PARITY_FIRST_B, c2.PARITY_FIRST_C, c2.PARITY_SAMPLES
FPS = c2.PARITY_FRAMES_PER_SET


@pytest.fixture(scope="module")
def triple(dev):
    caps = [dev.capture(r) for r in c2.parity_triple()]
    yield tuple(caps)
    for c in caps:
        c.free()


@pytest.fixture(scope="module")
def res(dev):
    r = Resident(dev)
    yield r
    r.free()


def run_triple(dev, triple, nfft, d_w, frames_per_set, n_sets, d_thr, firsts=(FA, FB, FC), n_samples=N, want_frames=True):
    return run(dev, triple, firsts, n_samples, nfft, d_w, frames_per_set, n_sets, d_thr, want_frames)


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("nfft", c2.NFFT)
def test_parity_with_the_restatement(dev, triple, res, nfft):
    try:
        for offset, scale in c2.CONVENTIONS:
            dev.set_unpack(offset, scale)
            want = c2.parity_reference(nfft, offset, scale)
            w = c2.parity_weights(nfft, offset)
            got, rec = run_triple(dev, triple, nfft, res(c2.f32(w)), FPS, w.shape[0], res(c2.parity_threshold(nfft, scale)))
            c2.compare(got, rec, want, (nfft, offset))
            assert want.cut.any() and not want.cut.all(), "the mask is neither empty nor full"
    finally:
        dev.set_unpack()
    assert dev.get_unpack() == (127.5, 1.0 / 127.5)


# ------------------------------------------------------------------------------------------------ 2. anchors
@pytest.mark.parametrize("nfft", c2.NFFT)
def test_anchors_are_bit_exact(dev, triple, res, nfft):
    a, b, c = triple
    h = nfft // 2
    d_thr = res(c2.parity_threshold(nfft))
    w = c2.parity_weights(nfft)
    n_sets = w.shape[0]
    w1_only, w2_only = w.copy(), w.copy()
    w1_only[:, 1], w2_only[:, 0] = 0, 0
    # W2 = 0: gj_cancel_dev(a, b, W1), whatever c is;  W1 = 0: gj_cancel_dev(a, c, W2), whatever b is
    for ws, aux, first_aux, others in ((w1_only, b, FB, ((a, b, c), (a, b, a))), (w2_only, c, FC, ((a, b, c), (a, a, c)))):
        single = np.ascontiguousarray(ws[:, 0] + ws[:, 1])                       # the one set that is not zero
        ref_b, ref_r = run_cancel(dev, a, a.nbytes, FA, aux, aux.nbytes, first_aux, N, nfft, res(c2.f32(single)), FPS, n_sets, d_thr)
        assert ref_r["n_excised"].any() and ref_r["total"].tobytes() != ref_r["total_in"].tobytes()
        for caps in others:
            firsts = (FA, FB if caps[1] is b else 0, FC if caps[2] is c else 0)
            got, rec = run(dev, caps, firsts, N, nfft, res(c2.f32(ws)), FPS, n_sets, d_thr)
            assert got.tobytes() == ref_b.tobytes(), (nfft, "bytes of gj_cancel_dev")
            assert rec.tobytes() == ref_r.tobytes(), (nfft, "records of gj_cancel_dev")
    # both zero: gj_excise_dev on capture a
    ex_b, ex_r = run_excise(dev, a, a.nbytes, FA, N, nfft, d_thr)
    got, rec = run_triple(dev, triple, nfft, res(np.zeros(4 * nfft)), 3, 1, d_thr)
    assert ex_r["n_excised"].any() and got.tobytes() == ex_b.tobytes(), (nfft, "bytes of gj_excise_dev")
    for key in ("total", "removed", "n_excised"):
        assert rec[key].tobytes() == ex_r[key].tobytes(), (nfft, key)
    assert rec["total_in"].tobytes() == rec["total"].tobytes()
    # b = c = a with W1 = W2 = (0.5, 0): nothing is left
    inf, halves = res(np.full(nfft, np.inf)), res(np.tile(np.float32([0.5, 0.0]), 2 * nfft))
    try:
        for offset, scale in c2.CONVENTIONS:
            dev.set_unpack(offset, scale)
            got, rec = run(dev, (a, a, a), (FA, FA, FA), N, nfft, halves, 1, 1, inf)
            nf = rec.size
            assert not rec["total"].any() and not rec["removed"].any() and not rec["n_excised"].any() and np.all(rec["total_in"] > 0)
            if offset == 127.5:
                assert np.all(got[2 * h:nf * nfft] == 128), (nfft, "rint(127.5) = 128")
            raw = c2.parity_triple()[0]
            assert got[:nfft].tobytes() == raw[2 * FA:2 * FA + nfft].tobytes()
            assert got[nf * nfft:].tobytes() == raw[2 * FA + nf * nfft:2 * (FA + N)].tobytes()
    finally:
        dev.set_unpack()
    # every threshold negative: everything that is left is removed
    got, rec = run_triple(dev, triple, nfft, res(c2.f32(w)), FPS, n_sets, res(np.full(nfft, -1.0)))
    assert np.all(rec["n_excised"] == nfft) and rec["removed"].tobytes() == rec["total"].tobytes() and np.all(rec["total"] > 0)
    assert np.all(got[2 * h:rec.size * nfft] == 128)


# ------------------------------------------------------------------------------------------------ 3. translation
@pytest.mark.parametrize("nfft", c2.NFFT)
def test_translation_null_records_and_repetition(dev, triple, res, nfft):
    h = nfft // 2
    d_thr = res(c2.parity_threshold(nfft))
    w = c2.parity_weights(nfft)
    d_w, n_sets, set_bytes = res(c2.f32(w)), w.shape[0], 16 * nfft
    long_b, long_r = run_triple(dev, triple, nfft, d_w, FPS, n_sets, d_thr)
    again_b, again_r = run_triple(dev, triple, nfft, d_w, FPS, n_sets, d_thr)
    assert again_b.tobytes() == long_b.tobytes() and again_r.tobytes() == long_r.tobytes(), "two identical calls"
    no_rec, _ = run_triple(dev, triple, nfft, d_w, FPS, n_sets, d_thr, want_frames=False)
    assert no_rec.tobytes() == long_b.tobytes(), "d_frames = NULL changes no byte"
    nf = long_r.size

    def shifted(k, d_sets, per_set, sets, ref_b, ref_r):
        got_b, got_r = run_triple(dev, triple, nfft, d_sets, per_set, sets, d_thr, (FA + k * h, FB + k * h, FC + k * h), N - k * h)
        assert got_r.tobytes() == ref_r[k:].tobytes(), (nfft, k, per_set, "records of the shared frames")
        assert got_b[nfft:(nf - k) * nfft].tobytes() == ref_b[(k + 1) * nfft:nf * nfft].tobytes(), (nfft, k, per_set, "interior bytes")

    # k a multiple of frames_per_set, the sets shifted alike
    for sets_off in (1, 2):
        k = sets_off * FPS
        if k + 2 <= nf and sets_off < n_sets:
            shifted(k, d_w.ptr + set_bytes * sets_off, FPS, n_sets - sets_off, long_b, long_r)
    # one set: every k
    one_b, one_r = run_triple(dev, triple, nfft, d_w, FPS, 1, d_thr)
    for k in (1, 2, 3, 4):
        if k + 2 <= nf:
            shifted(k, d_w, 2, 1, one_b, one_r)
    # a set per frame
    each_b, each_r = run_triple(dev, triple, nfft, d_w, 1, n_sets, d_thr)
    assert each_r[:FPS].tobytes() != long_r[:FPS].tobytes() or n_sets == 1
    for k in (1, 3):
        if k + 2 <= nf and k < n_sets:
            shifted(k, d_w.ptr + set_bytes * k, 1, n_sets - k, each_b, each_r)


# ------------------------------------------------------------------------------------------------ 4. run seams
SEAM_FRAMES_PER_SET = 7
SEAM_FIRST_B = si.EXCISE_FIRST + 3              # captures b and c are capture a three and eight samples on (one pointer)
SEAM_FIRST_C = si.EXCISE_FIRST + 8
# csrc/k_cancel2.hip Cancel2Cfg: min_waves and min_run at every size.  They are the excisor's, so a run is as long as
# si.excise_per_run says; were they to change, the run length below must follow them
CANCEL2_MIN_WAVES, CANCEL2_MIN_RUN = 2, 4


def cancel2_per_run(compute_units, nfft, n_frames):
    """cancel2_launch of csrc/k_cancel2.hip: frames per run."""
    slots = compute_units * CANCEL2_MIN_WAVES * si.per_step(nfft)
    return min(max(-(-n_frames // slots), CANCEL2_MIN_RUN), n_frames)


def seam_weights(nfft, n_sets):
    rng = np.random.default_rng(nfft)
    mag = rng.uniform(0.0, 0.7, (n_sets, 2, nfft))
    return (mag * np.exp(2j * np.pi * rng.uniform(0.0, 1.0, (n_sets, 2, nfft)))).astype(np.complex64)


@pytest.fixture(scope="module")
def seam_cap(dev):
    c = dev.capture(si.scale_excise_capture())
    yield c
    c.free()


@pytest.mark.parametrize("nfft", (256, 4096))
def test_runs_longer_than_four_frames(dev, seam_cap, res, nfft):
    cus = dev.info()["compute_units"]
    f, n, h, first = si.excise_frames(nfft), si.excise_samples(nfft), nfft // 2, si.EXCISE_FIRST
    per = cancel2_per_run(cus, nfft, f)
    assert (CANCEL2_MIN_WAVES, CANCEL2_MIN_RUN) == (si.EXCISE_MIN_WAVES, si.EXCISE_MIN_RUN) and per == si.excise_per_run(cus, nfft, f)
    assert per > CANCEL2_MIN_RUN and f % per != 0, (f"{nfft}: {f} frames are sized for runs of five on {si.SIZED_FOR_CUS} CUs; on this "
                                                    f"device's {cus} a run holds {per} frames")
    assert f == 2048 * (4096 // nfft) + 1 and (si.SIZED_FOR_CUS != cus or per == 5)
    cap, fps = seam_cap, SEAM_FRAMES_PER_SET
    assert gpsjam.excise_frames(n, nfft) == f and SEAM_FIRST_C + n <= cap.nsamples
    n_sets = -(-f // fps)
    w = seam_weights(nfft, n_sets)
    d_w, d_thr = res(c2.f32(w)), res(si.excise_thresholds(nfft))

    def call(first_frame, n_samples, want_frames=True):
        assert first_frame % fps == 0
        s, at = first_frame // fps, first_frame * h
        return run(dev, (cap, cap, cap), (first + at, SEAM_FIRST_B + at, SEAM_FIRST_C + at), n_samples, nfft,
                   d_w.ptr + 16 * nfft * s, fps, n_sets - s, d_thr, want_frames)

    long_b, long_r = call(0, n)
    assert long_r["n_excised"].sum() > 0 and np.all(long_r["total"] > 0)
    again_b, again_r = call(0, n)
    assert again_b.tobytes() == long_b.tobytes() and again_r.tobytes() == long_r.tobytes(), "the long call repeated"
    raw = si.scale_excise_capture()
    assert long_b[:nfft].tobytes() == raw[2 * first:2 * first + nfft].tobytes(), "the first half frame is capture a's"
    assert f * nfft < 2 * n and long_b[f * nfft:].tobytes() == raw[2 * first + f * nfft:2 * (first + n)].tobytes(), "the tail is capture a's"
    # two overlapping halves with runs of another length, the second one started on a set's first frame
    k2 = (f // 2 - 2) // fps * fps
    covered = np.zeros(f, bool)
    for k, m in ((0, f // 2 + 2), (k2, f - k2)):
        half_per = cancel2_per_run(cus, nfft, m)
        assert half_per != per and half_per >= CANCEL2_MIN_RUN, (nfft, per, half_per)
        piece_b, piece_r = call(k, (m - 1) * h + nfft if k == 0 else n - k * h)
        assert piece_r.size == m and piece_r.tobytes() == long_r[k:k + m].tobytes(), (nfft, k, "records")
        assert piece_b[nfft:m * nfft].tobytes() == long_b[(k + 1) * nfft:(k + m) * nfft].tobytes(), (nfft, k, "interior bytes")
        covered[k + 1:k + m] = True
    assert covered[1:].all(), "every hop of the long call lies inside a half"
    # a float64 restatement of the frames around the first run seam, from their own bytes and sets
    w0 = (5 * (4096 // nfft)) // fps * fps
    frames = 3 * fps
    sets = slice(w0 // fps, w0 // fps + 3)
    ns = (frames - 1) * h + nfft
    want = c2.cancel2(raw, raw, raw, w[sets], si.excise_thresholds(nfft), nfft, first + w0 * h, SEAM_FIRST_B + w0 * h,
                      SEAM_FIRST_C + w0 * h, ns, fps)
    assert er.threshold_margin(want.power, si.excise_thresholds(nfft)) >= c2.NEAR_TIE, "an input with a bin at its threshold"
    np.testing.assert_array_equal(long_r["n_excised"][w0:w0 + frames], want.records["n_excised"])
    for key in ("total_in", "total", "removed"):
        assert np.max(np.abs(long_r[key][w0:w0 + frames] - want.records[key]) / want.records["total_in"]) <= RTOL, (nfft, key)
    diff = np.abs(long_b[(w0 + 1) * nfft:(w0 + frames) * nfft].astype(np.int16) - want.out[nfft:frames * nfft].astype(np.int16))
    assert diff.max() <= 1 and not diff[er.tie_distance(want.value) > c2.TIE_BAND].any(), (nfft, "bytes around the first seam")


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals_enqueue_nothing(dev, triple, res):
    a, b, c = triple
    n = 8 * 256
    t256, t16 = res(np.full(256, -1.0)), res(np.full(16, -1.0))
    w256 = res(np.zeros(2 * 2 * 2 * 256))
    out, rec = Guarded(dev, a.nbytes), Guarded(dev, 4096 * REC)

    def args(d_a=a, nbytes_a=a.nbytes, first_a=0, d_b=b, nbytes_b=b.nbytes, first_b=0, d_c=c, nbytes_c=c.nbytes, first_c=0, n_samples=n,
             nfft=256, d_w=w256, fps=4, n_sets=2, d_thr=t256, d_out=out, d_rec=rec):
        return (d_a, nbytes_a, first_a, d_b, nbytes_b, first_b, d_c, nbytes_c, first_c, n_samples, nfft, d_w, fps, n_sets, d_thr, d_out, d_rec)
    try:
        cases = [
            (args(nfft=8), GJ_ERR_UNSUPPORTED),
            (args(nfft=8192, n_samples=3 * 8192), GJ_ERR_UNSUPPORTED),
            (args(nfft=48), GJ_ERR_UNSUPPORTED),
            (args(nfft=0), GJ_ERR_UNSUPPORTED),
            (args(n_samples=255), GJ_ERR_INVALID),                                   # n_samples < nfft
            (args(n_samples=0), GJ_ERR_INVALID),
            (args(first_a=FA + 1, n_samples=N), GJ_ERR_INVALID),                     # runs past capture a
            (args(first_b=FB + 1, n_samples=N), GJ_ERR_INVALID),                     # ... past capture b alone
            (args(first_c=FC + 1, n_samples=N), GJ_ERR_INVALID),                     # ... past capture c alone
            (args(first_a=a.nsamples + 1), GJ_ERR_INVALID),
            (args(first_c=c.nsamples + 1), GJ_ERR_INVALID),
            (args(first_b=2 ** 63, n_samples=2 ** 63 + 256), GJ_ERR_INVALID),        # first + n wraps
            (args(first_c=2 ** 63, n_samples=2 ** 63 + 256), GJ_ERR_INVALID),
            (args(d_a=0), GJ_ERR_INVALID),                                           # null captures
            (args(d_b=0), GJ_ERR_INVALID),
            (args(d_c=0), GJ_ERR_INVALID),
            (args(d_a=a.ptr + 1, nbytes_a=a.nbytes - 2), GJ_ERR_INVALID),            # odd captures
            (args(d_b=b.ptr + 1, nbytes_b=b.nbytes - 2), GJ_ERR_INVALID),
            (args(d_c=c.ptr + 1, nbytes_c=c.nbytes - 2), GJ_ERR_INVALID),
            (args(d_out=0), GJ_ERR_INVALID),                                         # null d_out, d_threshold
            (args(d_thr=0), GJ_ERR_INVALID),
            (args(d_thr=t256.ptr + 2), GJ_ERR_INVALID),                              # misaligned d_threshold, d_frames
            (args(d_rec=rec.ptr + 2), GJ_ERR_INVALID),
            (args(fps=0), GJ_ERR_INVALID),                                           # the sets
            (args(n_sets=0), GJ_ERR_INVALID),
            (args(d_w=0), GJ_ERR_INVALID),
            (args(d_w=w256.ptr + 4), GJ_ERR_INVALID),                                # d_weights: 8 bytes
            (args(d_w=w256.ptr + 2), GJ_ERR_INVALID),
            # d_out overlapping capture a, b, c (in place, shifted, touching the last byte), a capture inside d_out
            (args(d_a=out, nbytes_a=a.nbytes), GJ_ERR_INVALID),
            (args(d_b=out, nbytes_b=b.nbytes), GJ_ERR_INVALID),
            (args(d_c=out, nbytes_c=c.nbytes), GJ_ERR_INVALID),
            (args(d_a=out, nbytes_a=a.nbytes, d_out=out.ptr + 2 * n), GJ_ERR_INVALID),
            (args(d_b=out, nbytes_b=a.nbytes, d_out=out.ptr + a.nbytes - 1), GJ_ERR_INVALID),
            (args(d_c=out, nbytes_c=a.nbytes, d_out=out.ptr + a.nbytes - 1), GJ_ERR_INVALID),
            (args(d_c=out.ptr + 512, nbytes_c=1024, n_samples=256, d_out=out.ptr + 1), GJ_ERR_INVALID),
        ]
        refused(dev, dev.cancel2_dev, cases, out, rec)
        # accepted: a call that just fits all three captures, the output right behind an input's last byte, one pointer
        # at odd and different firsts, no records, 16 points at the captures' ends
        dev.cancel2_dev(*args(first_a=FA, first_b=FB, first_c=FC, n_samples=N))
        dev.cancel2_dev(*args(d_a=out, nbytes_a=2 * n, d_out=out.ptr + 2 * n, d_rec=None))
        dev.cancel2_dev(*args(d_b=a, nbytes_b=a.nbytes, d_c=a, nbytes_c=a.nbytes, first_a=1, first_b=5, first_c=8, d_rec=None))
        dev.cancel2_dev(*args(first_a=a.nsamples - 16, first_b=b.nsamples - 16, first_c=c.nsamples - 16, n_samples=16, nfft=16, d_thr=t16))
        dev.synchronize()
        out.check_pads("output")
        rec.check_pads("records")
    finally:
        freed(out, rec)


# ------------------------------------------------------------------------------------------------ Device.cancel2
def test_device_cancel2_takes_host_bytes_and_captures(dev, triple):
    ra, rb, rc = c2.parity_triple()
    nfft = 256
    w, thr = c2.parity_weights(nfft), c2.parity_threshold(nfft)
    want = c2.parity_reference(nfft)
    uploads = gpsjam.Capture.uploads
    x, rec_x = dev.cancel2(*triple, w, thr, nfft=nfft, first_a=FA, first_b=FB, first_c=FC, frames_per_set=FPS)
    assert gpsjam.Capture.uploads == uploads, "a cleaned capture is no host->device pass"
    y, rec_y = dev.cancel2(ra, rb, rc, w, thr, nfft=nfft, first_a=FA, first_b=FB, first_c=FC, frames_per_set=FPS)
    assert gpsjam.Capture.uploads == uploads + 3, "host bytes are uploaded once each"
    try:
        assert isinstance(x, gpsjam.Capture) and x.nbytes == 2 * N and rec_x.dtype == gpsjam.CANCEL_DTYPE
        assert x.download().tobytes() == y.download().tobytes() and rec_x.tobytes() == rec_y.tobytes()
        c2.compare(x.download(), rec_x, want, "Device.cancel2")
        # one set, no threshold, the defaults: the whole of what all three hold from sample 0
        z, rec_z = dev.cancel2(*triple, w[0], nfft=nfft)
        assert z.nsamples == min(c.nsamples for c in triple) and not rec_z["n_excised"].any()
        z.free()
        with pytest.raises(ValueError):
            dev.cancel2(*triple, w, nfft=nfft)                          # several sets need frames_per_set
        with pytest.raises(ValueError):
            dev.cancel2(*triple, np.zeros((2, nfft + 1), np.complex64), nfft=nfft)
    finally:
        x.free()
        y.free()


# ------------------------------------------------------------------------------------------------ 6. end to end
@pytest.fixture(scope="module")
def search(dev):
    s = gnss.AcqSearch(dev, prns=[p for p, *_ in er.E2E_SATS])
    yield s
    s.close()


def test_end_to_end_two_jammers_need_two_auxiliaries(dev, search):
    """Three C/A signals of 1.5 LSB in noise of sigma 10 LSB at each of three antennas; from sample 2^17 on two independent
    full-band Gaussian jammers of sigma 30 LSB from different directions.  The raw capture acquires none
    (tests/test_cancel2_host.py asserts that on the CPU, and that all three acquire jammer-free);
    mitigate.clean_spatial with either auxiliary alone leaves at least two of the three unacquired;
    mitigate.clean_spatial2 brings all three back."""
    free_a = c2.e2e_triple(False)[0]
    raw_a, raw_b, raw_c = c2.e2e_triple(True)
    lead, nfft, m = er.E2E_LEAD, c2.E2E_NFFT, c2.E2E_FRAMES_PER_ROW
    with dev.capture(free_a) as c:
        free = search.search(c, first_sample=lead)
    assert all(r.acquired for r in free), free
    singles = []
    with dev.capture(raw_a) as ca, dev.capture(raw_b) as cb, dev.capture(raw_c) as cc:
        before = search.search(ca, first_sample=lead)
        got = mitigate.clean_spatial2(dev, ca, cb, cc, nfft=nfft, frames_per_row=m, p_fa=c2.E2E_P_FA, lags=(0, 0))
        for aux in (cb, cc):
            one = mitigate.clean_spatial(dev, ca, aux, nfft=nfft, frames_per_row=m, p_fa=c2.E2E_P_FA, lag=0)
            try:
                singles.append((one.cancelled, search.search(one.capture, first_sample=lead)))
            finally:
                one.capture.free()
    try:
        assert isinstance(got, mitigate.CleanedSpatial2) and got.cancelled and got.note == "" and got.capture.nbytes == raw_a.size
        after = search.search(got.capture, first_sample=lead)
        cleaned = got.capture.download()
    finally:
        got.capture.free()
    assert not any(r.acquired for r in before), before
    for cancelled, found in singles:
        assert cancelled and sum(not r.acquired for r in found) >= 2, ("one auxiliary has one null per bin", found)
    assert got.weights.shape == (5, 2, nfft) and not got.weights[:4].any(), "nothing is flagged in the quiet rows: W = 0 there"
    flagged = np.any(got.weights[4] != 0, axis=0)
    w1, w2 = got.weights[4, 0][flagged], got.weights[4, 1][flagged]
    assert flagged.sum() >= nfft - 8 and not flagged[[0, 1, -1]].any()
    assert 0.55 < np.median(np.abs(w1)) < 0.8 and 0.55 < np.median(np.abs(w2)) < 0.8          # 0.666 and 0.665 in float64
    print(f"{int(flagged.sum())} bins cancelled, median |W1| {np.median(np.abs(w1)):.3f}, |W2| {np.median(np.abs(w2)):.3f}, "
          f"suppression {got.suppression_db}")
    assert len(got.bands) >= 1 and all(7.0 < s < 11.0 for s in got.suppression_db)            # 9.1 dB in float64
    for r, ref, (psi_b, psi_c) in zip(after, free, c2.E2E_SAT_PHASE):
        want = ref.cn0 + c2.e2e_predicted_db(w1, w2, psi_b, psi_c)
        print(f"PRN {r.prn}: C/N0 {r.cn0:.2f} cleaned, {ref.cn0:.2f} jammer-free, predicted {want:.2f}, peak ratio {r.peak_ratio:.2f}")
        assert r.acquired and r.code_index == ref.code_index and abs(r.freq_index - ref.freq_index) <= 1, (r, ref)
        assert abs(r.cn0 - want) <= c2.E2E_CN0_TOL_DB, (r, ref, want)
    quiet = 2 * (lead - nfft)                                  # every frame that ends in front of the jammers
    assert cleaned[:quiet].tobytes() == raw_a[:quiet].tobytes(), "the quiet lead-in comes back byte-identical"
    assert cleaned[2 * lead:].tobytes() != raw_a[2 * lead:].tobytes()


def test_clean_spatial2_with_nothing_to_cancel_returns_a_copy(dev):
    free_a, free_b, free_c = c2.e2e_triple(False)
    head = 2 * er.E2E_LEAD
    got = mitigate.clean_spatial2(dev, free_a[:head], free_b[:head], free_c[:head], nfft=c2.E2E_NFFT,
                                  frames_per_row=c2.E2E_FRAMES_PER_ROW, lags=(0, 0))
    try:
        assert not got.cancelled and "copy of main" in got.note and got.bands == [] and got.suppression_db == []
        assert got.capture.download().tobytes() == free_a[:head].tobytes()
        assert got.records["total"].tobytes() == got.records["total_in"].tobytes() and not got.weights.any()
    finally:
        got.capture.free()
