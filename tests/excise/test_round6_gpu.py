"""The frequency-domain excisor (gj_excise_dev, Device.excise, gpsjam.mitigate) on the GPU.

This file sits in a package of its own on purpose, as tests/ridge/ does: the suite orders GPU files by basename
(tests/conftest.py SUITE_ORDER, which tests/test_suite_order.py holds every GPU file to), and under the name
test_round6_gpu.py it runs in stage 2, behind the parity tests of K2 whose transform it shares.

Yardstick: the float64 restatement of the definition in include/gpsjam.h (tests/excise_restatement.py).  n_excised is
equal on EVERY frame (tests/test_excise_host.py shows that no input has a bin within 1e-4 of its threshold); total and
removed within rtol 1e-5 of total, the project's figure for a K2 value summed in another order; bytes equal wherever
the float64 value is further than TIE_BAND from a rounding tie and within 1 elsewhere.  Identity, translation and
repetition are bit-exact.  Every call writes into a sentinel-filled buffer whose bytes behind 2 * n_samples and
behind d_frames[F] must stay untouched."""
import numpy as np
import pytest

import excise_restatement as er
import gpsjam
from gpsjam import gnss, mitigate
from gpu_lib import GJ_ERR_INVALID, GJ_ERR_UNSUPPORTED, Guarded, Resident, freed, refused
from gpu_lib import run_excise as run

pytestmark = pytest.mark.gpu

REC = gpsjam.EXCISE_DTYPE.itemsize


@pytest.fixture(scope="module")
def cap(dev):
    c = dev.capture(er.parity_capture())
    yield c
    c.free()


@pytest.fixture(scope="module")
def thr(dev):
    t = Resident(dev)
    yield t
    t.free()


@pytest.mark.parametrize("nfft", er.NFFT)
def test_identity_is_byte_exact(dev, cap, thr, nfft):
    raw = er.parity_capture()
    inf = thr(np.full(nfft, np.inf))
    for first, n in ((0, cap.nsamples), (1, cap.nsamples - 1), (3, min(9 * nfft + nfft // 2 + 5, cap.nsamples - 3)), (cap.nsamples - nfft - 7, nfft + 7)):
        got, rec = run(dev, cap, cap.nbytes, first, n, nfft, inf)
        assert got.tobytes() == raw[2 * first:2 * (first + n)].tobytes(), (nfft, first, n)
        assert rec.size == gpsjam.excise_frames(n, nfft) and not rec["n_excised"].any() and not rec["removed"].any()
        assert np.all(rec["total"] > 0) and not rec["reserved"].any()
    nan = thr(np.full(nfft, np.nan))
    got, rec = run(dev, cap, cap.nbytes, 1, 7 * nfft, nfft, nan, want_frames=False)      # NaN never excises; no records asked for
    assert got.tobytes() == raw[2:2 * (1 + 7 * nfft)].tobytes() and rec.size == 13


@pytest.mark.parametrize("nfft", er.NFFT)
def test_parity_with_the_restatement(dev, cap, thr, nfft):
    try:
        for offset, scale in er.CONVENTIONS:
            dev.set_unpack(offset, scale)
            want = er.parity_reference(nfft, offset, scale)
            got, rec = run(dev, cap, cap.nbytes, er.PARITY_FIRST, cap.nsamples - er.PARITY_FIRST, nfft, thr(er.parity_threshold(nfft, scale)))
            er.compare(got, rec, want, (nfft, offset))
    finally:
        dev.set_unpack()
    assert dev.get_unpack() == (127.5, 1.0 / 127.5)


@pytest.mark.parametrize("nfft", er.NFFT)
def test_frame_counts_that_do_not_fill_a_workgroup_step_and_run_seams(dev, cap, thr, nfft):
    per_step, h, first = 4096 // nfft, nfft // 2, er.PARITY_FIRST
    raw = er.parity_capture()
    d_thr = thr(er.parity_threshold(nfft))
    want = er.parity_reference(nfft)
    n_long = cap.nsamples - first
    long_b, long_r = run(dev, cap, cap.nbytes, first, n_long, nfft, d_thr)
    again_b, again_r = run(dev, cap, cap.nbytes, first, n_long, nfft, d_thr)
    assert again_b.tobytes() == long_b.tobytes() and again_r.tobytes() == long_r.tobytes()
    for nf in sorted({1, 2, per_step - 1, per_step + 1, 2 * per_step + 3} - {0}):
        # exactly nf frames, the last one ending on the capture's last byte
        n = (nf - 1) * h + nfft
        if n > n_long:
            continue
        assert gpsjam.excise_frames(n, nfft) == nf and gpsjam.excise_frames(n - 1, nfft) == nf - 1
        with dev.capture(raw[:2 * (first + n)]) as exact:
            got, rec = run(dev, exact, exact.nbytes, first, n, nfft, d_thr)
        # the same range as the head of the long capture: same bits
        head_b, head_r = run(dev, cap, cap.nbytes, first, n, nfft, d_thr)
        assert head_b.tobytes() == got.tobytes() and head_r.tobytes() == rec.tobytes(), (nfft, nf)
        # and the long call's own frames and interior bytes
        assert rec.tobytes() == long_r[:nf].tobytes(), (nfft, nf)
        assert got[nfft:nf * nfft].tobytes() == long_b[nfft:nf * nfft].tobytes(), (nfft, nf)
        np.testing.assert_array_equal(rec["n_excised"], want.records["n_excised"][:nf])
        assert got[:nfft].tobytes() == raw[2 * first:2 * first + nfft].tobytes()
        assert got[nf * nfft:].tobytes() == raw[2 * first + nf * nfft:2 * (first + n)].tobytes()
    # starts shifted by k h: the shared frames' records and the overlapping interior bytes, bit for bit
    nf_long = long_r.size
    for k in (1, per_step + 1, 7):
        if k + 2 > nf_long:
            continue
        sh_b, sh_r = run(dev, cap, cap.nbytes, first + k * h, n_long - k * h, nfft, d_thr)
        assert sh_r.tobytes() == long_r[k:].tobytes(), (nfft, k)
        # shifted call's samples [h, F' h) = long call's samples [(k + 1) h, F h)
        assert sh_b[nfft:(nf_long - k) * nfft].tobytes() == long_b[(k + 1) * nfft:nf_long * nfft].tobytes(), (nfft, k)


@pytest.mark.parametrize("nfft", er.NFFT)
def test_fixed_notch(dev, cap, thr, nfft):
    raw = er.parity_capture()
    first, n = 1, min(cap.nsamples - 1, 40 * nfft + 3)
    band = np.full(nfft, np.inf, np.float32)
    band[2:6] = -1.0
    band[nfft - 3:] = -1e-30
    got, rec = run(dev, cap, cap.nbytes, first, n, nfft, thr(band))
    assert np.all(rec["n_excised"] == 7) and np.all(rec["removed"] > 0) and np.all(rec["removed"] < rec["total"])
    everywhere = thr(np.full(nfft, -1.0))
    try:
        for offset, scale in er.CONVENTIONS:
            dev.set_unpack(offset, scale)
            got, rec = run(dev, cap, cap.nbytes, first, n, nfft, everywhere)
            assert np.all(rec["n_excised"] == nfft) and np.array_equal(rec["removed"], rec["total"])
            nf = rec.size
            assert np.all(got[nfft:nf * nfft] == 128), (nfft, offset)             # rint(127.5) = rint(128) = 128
            assert got[:nfft].tobytes() == raw[2 * first:2 * first + nfft].tobytes()
            assert got[nf * nfft:].tobytes() == raw[2 * first + nf * nfft:2 * (first + n)].tobytes()
    finally:
        dev.set_unpack()


@pytest.mark.parametrize("nfft", er.CLAMP_NFFT)
def test_overshoot_is_clamped_not_wrapped(dev, thr, nfft):
    raw = er.clamp_capture()
    want = er.excise(raw, er.clamp_threshold(nfft), nfft)
    with dev.capture(raw) as c:
        got, rec = run(dev, c, c.nbytes, 0, c.nsamples, nfft, thr(er.clamp_threshold(nfft)))
    body = got[want.lo:want.hi]
    assert np.all(body[want.value > 256.0] == 255) and np.all(body[want.value < -1.0] == 0)
    assert np.sum(body == 255) > body.size // 20 and np.sum(body == 0) > body.size // 20
    er.compare(got, rec, want, ("clamp", nfft))


def test_refusals_enqueue_nothing(dev, cap, thr):
    n = 8 * 256
    t256, t16 = thr(np.full(256, -1.0)), thr(np.full(16, -1.0))
    out, rec = Guarded(dev, cap.nbytes), Guarded(dev, 4096 * REC)
    try:
        cases = [  # d_iq, nbytes, first, n_samples, nfft, d_thr, d_out, d_frames, status
            (cap, cap.nbytes, 0, n, 8, t256, out, rec, GJ_ERR_UNSUPPORTED),
            (cap, cap.nbytes, 0, 3 * 8192, 8192, t256, out, rec, GJ_ERR_UNSUPPORTED),
            (cap, cap.nbytes, 0, n, 48, t256, out, rec, GJ_ERR_UNSUPPORTED),
            (cap, cap.nbytes, 0, n, 0, t256, out, rec, GJ_ERR_UNSUPPORTED),
            (cap, cap.nbytes, 0, 255, 256, t256, out, rec, GJ_ERR_INVALID),              # n_samples < nfft
            (cap, cap.nbytes, 0, 0, 256, t256, out, rec, GJ_ERR_INVALID),
            (cap, cap.nbytes, 1, cap.nsamples, 256, t256, out, rec, GJ_ERR_INVALID),     # runs past the capture
            (cap, cap.nbytes, cap.nsamples + 1, 256, 256, t256, out, rec, GJ_ERR_INVALID),
            (cap, cap.nbytes, 2 ** 63, 2 ** 63 + 256, 256, t256, out, rec, GJ_ERR_INVALID),   # first + n wraps
            (0, cap.nbytes, 0, n, 256, t256, out, rec, GJ_ERR_INVALID),                  # null d_iq
            (cap.ptr + 1, cap.nbytes - 2, 0, n, 256, t256, out, rec, GJ_ERR_INVALID),    # odd d_iq
            (cap, cap.nbytes, 0, n, 256, t256, 0, rec, GJ_ERR_INVALID),                  # null d_out
            (cap, cap.nbytes, 0, n, 256, 0, out, rec, GJ_ERR_INVALID),                   # null d_threshold
            (cap, cap.nbytes, 0, n, 256, t256.ptr + 2, out, rec, GJ_ERR_INVALID),        # misaligned d_threshold
            (cap, cap.nbytes, 0, n, 256, t256, out, rec.ptr + 2, GJ_ERR_INVALID),        # misaligned d_frames
            # d_out inside the capture: in place, shifted, touching the last byte; the capture inside d_out
            (out, cap.nbytes, 0, n, 256, t256, out, rec, GJ_ERR_INVALID),
            (out, cap.nbytes, 0, n, 256, t256, out.ptr + 2 * n, rec, GJ_ERR_INVALID),
            (out, cap.nbytes, 0, n, 256, t256, out.ptr + cap.nbytes - 1, rec, GJ_ERR_INVALID),
            (out.ptr + 512, 1024, 0, 256, 256, t256, out.ptr + 1, rec, GJ_ERR_INVALID),
        ]
        refused(dev, dev.excise_dev, [(c[:-1], c[-1]) for c in cases], out, rec)
        # accepted: a call that just fits (the whole capture; the output right behind the input's last byte), 16 points
        dev.excise_dev(cap, cap.nbytes, 0, cap.nsamples, 256, t256, out, rec)
        dev.excise_dev(out, 2 * n, 0, n, 256, t256, out.ptr + 2 * n, None)
        dev.excise_dev(cap, cap.nbytes, cap.nsamples - 16, 16, 16, t16, out, rec)
        dev.synchronize()
        out.check_pads("output")
        rec.check_pads("records")
    finally:
        freed(out, rec)


def test_device_excise_and_mitigate_clean(dev, cap):
    raw = er.parity_capture()
    nfft = 256
    want = er.excise(raw, er.parity_threshold(nfft), nfft)
    uploads = gpsjam.Capture.uploads
    a, rec_a = dev.excise(cap, er.parity_threshold(nfft), nfft=nfft)
    assert gpsjam.Capture.uploads == uploads, "a cleaned capture is no host->device pass"
    b, rec_b = dev.excise(raw, er.parity_threshold(nfft), nfft=nfft)
    try:
        assert isinstance(a, gpsjam.Capture) and a.nbytes == cap.nbytes and a.ptr != cap.ptr
        assert a.download().tobytes() == b.download().tobytes() and rec_a.tobytes() == rec_b.tobytes()
        er.compare(a.download(), rec_a, want, "Device.excise")
        part, rec_p = dev.excise(cap, er.parity_threshold(nfft), nfft=nfft, first_sample=128 * 3, n_samples=5000)
        assert part.nbytes == 10000 and rec_p.tobytes() == rec_a[3:3 + rec_p.size].tobytes()
        part.free()
        # the resident result goes wherever a Capture goes
        ridge = dev.ridge(a, nfft=nfft)
        assert len(ridge) == gpsjam.ridge_frames(a.nbytes, 0, nfft, nfft // 2)
        assert ridge.total.sum() < 0.5 * dev.ridge(cap, nfft=nfft).total.sum()         # the tone and the chirp are gone
        psd, _ = dev.welch(a, chunk_samples=a.nsamples, nperseg=nfft, want_db=False)
        raw_psd, _ = dev.welch(cap, chunk_samples=cap.nsamples, nperseg=nfft, want_db=False)
        assert psd.shape == raw_psd.shape and psd.shape[1] == nfft and psd.sum() < 0.5 * raw_psd.sum()
        with pytest.raises(ValueError):
            dev.excise(cap, np.zeros(nfft + 1), nfft=nfft)
    finally:
        a.free()
        b.free()
    # mitigate.clean: host bytes and a resident capture give the same bytes; no onset here, so the floor is flat
    args = dict(nfft=nfft, rise_db=12.0, noise_samples=4096, window=500, factor=1e6)
    c1, c2 = mitigate.clean(dev, cap, **args), mitigate.clean(dev, raw, **args)
    try:
        assert c1.floor_from == c2.floor_from == "flat median" and np.unique(c1.threshold).size == 1
        assert c1.capture.download().tobytes() == c2.capture.download().tobytes() and c1.records.tobytes() == c2.records.tobytes()
        assert np.array_equal(c1.threshold, c2.threshold) and 0.0 < c1.removed_share == c2.removed_share < 1.0
        given = mitigate.clean(dev, cap, nfft=nfft, threshold=er.parity_threshold(nfft))
        assert given.floor_from == "given" and given.records.tobytes() == rec_a.tobytes()
        given.capture.free()
    finally:
        c1.capture.free()
        c2.capture.free()


@pytest.fixture(scope="module")
def search(dev):
    s = gnss.AcqSearch(dev, prns=[p for p, *_ in er.E2E_SATS])
    yield s
    s.close()


@pytest.fixture(scope="module")
def jammer_free(dev, search):
    with dev.capture(er.e2e_capture(None)) as c:
        res = search.search(c, first_sample=er.E2E_LEAD)
    assert all(r.acquired for r in res), res
    return res


@pytest.mark.parametrize("jammer", ["tone", "chirp"])
def test_end_to_end_the_satellites_come_back(dev, search, jammer_free, jammer):
    """Three C/A signals of 3 LSB in noise of sigma 10 LSB; from sample 2^17 on a 60-LSB tone at 137 kHz (or the
    simulator's chirp: the float64 restatement with the oracle's acquisition re-acquires all three under it too, C/N0
    within 0.2 dB of the tone case).  mitigate.clean at 1024 points and 12 dB."""
    raw = er.e2e_capture(jammer)
    with dev.capture(raw) as c:
        before = search.search(c, first_sample=er.E2E_LEAD)
        res = mitigate.clean(dev, c, nfft=er.E2E_NFFT, rise_db=er.E2E_RISE_DB, fs=er.FS, **er.E2E_ONSET_ARGS)
    try:
        assert res.floor_from == "quiet part" and res.capture.nbytes == raw.size
        after = search.search(res.capture, first_sample=er.E2E_LEAD)
        cleaned = res.capture.download()
        series = search.series(res.capture, first_sample=er.E2E_LEAD, n_epochs=1)      # the consumer the issue names
    finally:
        res.capture.free()
    assert not any(r.acquired for r in before), before
    for r, ref in zip(after, jammer_free):
        print(f"{jammer} PRN {r.prn}: C/N0 {r.cn0:.2f} cleaned, {ref.cn0:.2f} jammer-free, peak ratio {r.peak_ratio:.2f}")
        assert r.acquired and (r.code_index, r.freq_index) == (ref.code_index, ref.freq_index), (r, ref)
        assert abs(r.cn0 - ref.cn0) <= er.E2E_CN0_TOL_DB, (r, ref)
    assert series.acquired.all()
    lead = 2 * (er.E2E_LEAD - er.E2E_NFFT)                 # every frame that ends in front of the jammer
    assert cleaned[:lead].tobytes() == raw[:lead].tobytes()
    assert 0.5 < res.removed_share < 1.0
