"""The chirp-domain excisor (gj_excise_chirp_dev, gj_chirp_rates_dev, Device.excise_chirp, mitigate.clean_swept) on the GPU.

In a package of its own, as tests/excise/ is: the suite orders GPU files by basename (tests/conftest.py SUITE_ORDER), and
under the name test_round6_gpu.py this file runs in stage 2, behind the parity tests of K2 whose transform it shares.

Yardstick: the float64 restatement of the definition in include/gpsjam.h (tests/excise_chirp_restatement.py).  n_excised
is equal on EVERY frame (tests/test_excise_chirp_host.py shows that no input has a bin within 1e-4 of its threshold); total
and removed within rtol 1e-5 of total; bytes equal wherever the float64 value is further than TIE_BAND from a rounding tie
and within 1 elsewhere, with at most TIE_SHARE_CAP = 1.1e-3 of the bytes inside the band.  Rate 0, identity, translation
and repetition are bit-exact, the picker's rates exact integers.  Every call writes into sentinel-filled buffers whose bytes
behind 2 * n_samples and behind d_frames[F] must stay untouched."""
import numpy as np
import pytest

import excise_chirp_restatement as xr
import excise_restatement as er
import gpsjam
from gpsjam import gnss, mitigate
from gpu_lib import GJ_ERR_INVALID, GJ_ERR_UNSUPPORTED, Guarded, Resident, freed, refused
from gpu_lib import run_excise_chirp as run

pytestmark = pytest.mark.gpu

REC = gpsjam.EXCISE_DTYPE.itemsize
EXACT_NFFT = (16, 64, 1024, 2048, 4096)         # rate 0 against gj_excise_dev
SHIFT_NFFT = (64, 1024, 2048, 4096)             # translation and repetition


@pytest.fixture(scope="module")
def res(dev):
    r = Resident(dev)
    yield r
    r.free()


@pytest.fixture(scope="module")
def caps(dev):
    held = {}

    def get(nfft):
        if nfft not in held:
            held[nfft] = dev.capture(xr.parity_capture(nfft))
        return held[nfft]
    yield get
    for c in held.values():
        c.free()


@pytest.mark.parametrize("nfft", xr.NFFT)
def test_parity_with_the_restatement(dev, caps, res, nfft):
    cap = caps(nfft)
    d_rate = res(xr.parity_rates(nfft), np.int32)
    try:
        for offset, scale in (xr.CONVENTIONS if nfft == 1024 else xr.CONVENTIONS[:1]):
            dev.set_unpack(offset, scale)
            want = xr.parity_reference(nfft, offset, scale)
            got, rec = run(dev, cap, cap.nbytes, xr.PARITY_FIRST, cap.nsamples - xr.PARITY_FIRST, nfft, d_rate,
                           res(xr.parity_threshold(nfft, scale)))
            xr.compare(got, rec, want, (nfft, offset))
    finally:
        dev.set_unpack()
    assert dev.get_unpack() == (127.5, 1.0 / 127.5)


@pytest.mark.parametrize("nfft", EXACT_NFFT)
def test_rate_zero_and_whole_periods_are_the_plain_excisor_bit_for_bit(dev, caps, res, nfft):
    cap, first = caps(nfft), xr.PARITY_FIRST
    n = cap.nsamples - first
    nf = gpsjam.excise_frames(n, nfft)
    d_thr = res(xr.parity_threshold(nfft))
    want_b, want_r = run(dev, cap, cap.nbytes, first, n, nfft, None, d_thr, plain=True)
    assert want_r["n_excised"].sum() > 0
    period = 2 * nfft * nfft
    mixed = np.array([(0, period, -period, 2 * period)[f % 4] if 2 * period < 2 ** 31 else (0, period, -period)[f % 3]
                      for f in range(nf)], np.int64)
    for rates in (np.zeros(nf), np.full(nf, period), mixed):
        got_b, got_r = run(dev, cap, cap.nbytes, first, n, nfft, res(rates, np.int32), d_thr)
        assert got_b.tobytes() == want_b.tobytes() and got_r.tobytes() == want_r.tobytes(), (nfft, int(rates[1]))


@pytest.mark.parametrize("nfft", xr.NFFT)
def test_identity_is_byte_exact_whatever_the_rates(dev, caps, res, nfft):
    cap, raw = caps(nfft), xr.parity_capture(nfft)
    inf = res(np.full(nfft, np.inf))
    for first, n in ((0, cap.nsamples), (1, cap.nsamples - 1), (3, min(9 * nfft + nfft // 2 + 5, cap.nsamples - 3)),
                     (cap.nsamples - nfft - 7, nfft + 7)):
        nf = gpsjam.excise_frames(n, nfft)
        got, rec = run(dev, cap, cap.nbytes, first, n, nfft, res(xr.parity_rates(nfft, nf), np.int32), inf)
        assert got.tobytes() == raw[2 * first:2 * (first + n)].tobytes(), (nfft, first, n)
        assert rec.size == nf and not rec["n_excised"].any() and not rec["removed"].any()
        assert np.all(rec["total"] > 0) and not rec["reserved"].any()
    nan = res(np.full(nfft, np.nan))
    got, rec = run(dev, cap, cap.nbytes, 1, 7 * nfft, nfft, res(xr.parity_rates(nfft, 13), np.int32), nan, want_frames=False)
    assert got.tobytes() == raw[2:2 * (1 + 7 * nfft)].tobytes() and rec.size == 13


@pytest.mark.parametrize("nfft", xr.REMOVAL_NFFT)
def test_complete_removal_of_a_noiseless_sweep(dev, res, nfft):
    """A noiseless chirp of an even integer rate from sample 0: behind the de-chirp every frame holds a line on a bin
    centre, three bins of a Hann window, and what is left is the quantiser's half LSB.  The plain excisor with the same
    threshold leaves the sweep standing."""
    raw, d_thr = xr.removal_capture(nfft), res(xr.removal_threshold(nfft))
    nf = xr.REMOVAL_FRAMES
    with dev.capture(raw) as c:
        got, rec = run(dev, c, c.nbytes, 0, c.nsamples, nfft, res(np.full(nf, xr.REMOVAL_Q[nfft]), np.int32), d_thr)
        plain, _ = run(dev, c, c.nbytes, 0, c.nsamples, nfft, None, d_thr, plain=True)
    assert rec.size == nf and np.all(rec["n_excised"] == 3)
    np.testing.assert_allclose(rec["removed"] / rec["total"], 1.0, atol=1e-3)
    body, pbody = got[nfft:nf * nfft], plain[nfft:nf * nfft]
    assert np.all((body == 127) | (body == 128)), np.unique(body)
    assert np.mean((pbody == 127) | (pbody == 128)) < 0.5
    assert got[:nfft].tobytes() == raw[:nfft].tobytes() and got[nf * nfft:].tobytes() == raw[nf * nfft:].tobytes()


@pytest.mark.parametrize("nfft", xr.NFFT)
def test_frame_counts_run_seams_translation_and_repetition(dev, caps, res, nfft):
    per_step, h, first = 4096 // nfft, nfft // 2, xr.PARITY_FIRST
    cap, raw = caps(nfft), xr.parity_capture(nfft)
    d_thr = res(xr.parity_threshold(nfft))
    want = xr.parity_reference(nfft)
    rates = xr.parity_rates(nfft)
    d_rate = res(rates, np.int32)
    n_long = cap.nsamples - first
    long_b, long_r = run(dev, cap, cap.nbytes, first, n_long, nfft, d_rate, d_thr)
    again_b, again_r = run(dev, cap, cap.nbytes, first, n_long, nfft, d_rate, d_thr)
    assert again_b.tobytes() == long_b.tobytes() and again_r.tobytes() == long_r.tobytes()
    no_rec, _ = run(dev, cap, cap.nbytes, first, n_long, nfft, d_rate, d_thr, want_frames=False)
    assert no_rec.tobytes() == long_b.tobytes(), "d_frames = NULL changes no byte"
    # 1 frame, counts around the runs of at least four frames, counts that do not fill a workgroup step
    for nf in sorted({1, 2, 3, 4, 5, 7, 8, 9, per_step - 1, per_step + 1, 2 * per_step + 3} - {0}):
        n = (nf - 1) * h + nfft                      # exactly nf frames, the last one ending on the capture's last byte
        if n > n_long:
            continue
        assert gpsjam.excise_frames(n, nfft) == nf and gpsjam.excise_frames(n - 1, nfft) == nf - 1
        with dev.capture(raw[:2 * (first + n)]) as exact:
            got, rec = run(dev, exact, exact.nbytes, first, n, nfft, d_rate, d_thr)
        head_b, head_r = run(dev, cap, cap.nbytes, first, n, nfft, d_rate, d_thr)
        assert head_b.tobytes() == got.tobytes() and head_r.tobytes() == rec.tobytes(), (nfft, nf)
        assert rec.tobytes() == long_r[:nf].tobytes(), (nfft, nf)
        assert got[nfft:nf * nfft].tobytes() == long_b[nfft:nf * nfft].tobytes(), (nfft, nf)
        np.testing.assert_array_equal(rec["n_excised"], want.records["n_excised"][:nf])
        assert got[:nfft].tobytes() == raw[2 * first:2 * first + nfft].tobytes()
        assert got[nf * nfft:].tobytes() == raw[2 * first + nf * nfft:2 * (first + n)].tobytes()
    if nfft not in SHIFT_NFFT:
        return
    # starts shifted by k h with d_rate + k: the shared frames' records and the overlapping interior bytes, bit for bit
    nf_long = long_r.size
    for k in (1, per_step + 1, 7):
        if k + 2 > nf_long:
            continue
        sh_b, sh_r = run(dev, cap, cap.nbytes, first + k * h, n_long - k * h, nfft, d_rate.ptr + 4 * k, d_thr)
        assert sh_r.tobytes() == long_r[k:].tobytes(), (nfft, k)
        assert sh_b[nfft:(nf_long - k) * nfft].tobytes() == long_b[(k + 1) * nfft:nf_long * nfft].tobytes(), (nfft, k)


def test_refusals_enqueue_nothing(dev, caps, res):
    cap = caps(256)
    n = 8 * 256
    t256, t16 = res(np.full(256, -1.0)), res(np.full(16, -1.0))
    rt = res(np.arange(4096) % 7, np.int32)
    out, rec = Guarded(dev, cap.nbytes), Guarded(dev, 4096 * REC)
    try:
        cases = [  # d_iq, nbytes, first, n_samples, nfft, d_rate, d_thr, d_out, d_frames, status
            (cap, cap.nbytes, 0, n, 8, rt, t256, out, rec, GJ_ERR_UNSUPPORTED),
            (cap, cap.nbytes, 0, 3 * 8192, 8192, rt, t256, out, rec, GJ_ERR_UNSUPPORTED),
            (cap, cap.nbytes, 0, n, 48, rt, t256, out, rec, GJ_ERR_UNSUPPORTED),
            (cap, cap.nbytes, 0, n, 0, rt, t256, out, rec, GJ_ERR_UNSUPPORTED),
            (cap, cap.nbytes, 0, 255, 256, rt, t256, out, rec, GJ_ERR_INVALID),              # n_samples < nfft
            (cap, cap.nbytes, 0, 0, 256, rt, t256, out, rec, GJ_ERR_INVALID),
            (cap, cap.nbytes, 1, cap.nsamples, 256, rt, t256, out, rec, GJ_ERR_INVALID),     # runs past the capture
            (cap, cap.nbytes, cap.nsamples + 1, 256, 256, rt, t256, out, rec, GJ_ERR_INVALID),
            (cap, cap.nbytes, 2 ** 63, 2 ** 63 + 256, 256, rt, t256, out, rec, GJ_ERR_INVALID),   # first + n wraps
            (0, cap.nbytes, 0, n, 256, rt, t256, out, rec, GJ_ERR_INVALID),                  # null d_iq
            (cap.ptr + 1, cap.nbytes - 2, 0, n, 256, rt, t256, out, rec, GJ_ERR_INVALID),    # odd d_iq
            (cap, cap.nbytes, 0, n, 256, rt, t256, 0, rec, GJ_ERR_INVALID),                  # null d_out
            (cap, cap.nbytes, 0, n, 256, rt, 0, out, rec, GJ_ERR_INVALID),                   # null d_threshold
            (cap, cap.nbytes, 0, n, 256, rt, t256.ptr + 2, out, rec, GJ_ERR_INVALID),        # misaligned d_threshold
            (cap, cap.nbytes, 0, n, 256, rt, t256, out, rec.ptr + 2, GJ_ERR_INVALID),        # misaligned d_frames
            (cap, cap.nbytes, 0, n, 256, 0, t256, out, rec, GJ_ERR_INVALID),                 # null d_rate
            (cap, cap.nbytes, 0, n, 256, rt.ptr + 2, t256, out, rec, GJ_ERR_INVALID),        # misaligned d_rate
            (cap, cap.nbytes, 0, n, 256, rt.ptr + 1, t256, out, rec, GJ_ERR_INVALID),
            # d_out inside the capture: in place, shifted, touching the last byte; the capture inside d_out
            (out, cap.nbytes, 0, n, 256, rt, t256, out, rec, GJ_ERR_INVALID),
            (out, cap.nbytes, 0, n, 256, rt, t256, out.ptr + 2 * n, rec, GJ_ERR_INVALID),
            (out, cap.nbytes, 0, n, 256, rt, t256, out.ptr + cap.nbytes - 1, rec, GJ_ERR_INVALID),
            (out.ptr + 512, 1024, 0, 256, 256, rt, t256, out.ptr + 1, rec, GJ_ERR_INVALID),
        ]
        refused(dev, dev.excise_chirp_dev, [(c[:-1], c[-1]) for c in cases], out, rec)
        # the picker: d_scan, n_frames, rate_first, rate_step, min_concentration, d_rate (the record buffer stands in for both)
        picks = ((0, 8, 0, 1, 0.1, out), (rec, 8, 0, 1, 0.1, 0), (rec.ptr + 2, 8, 0, 1, 0.1, out),
                 (rec, 8, 0, 1, 0.1, out.ptr + 2), (rec, 0, 0, 1, 0.1, out), (rec, 8, 0, 0, 0.1, out),
                 (rec, 8, 0, -1, 0.1, out))
        refused(dev, dev.chirp_rates_dev, [(c, GJ_ERR_INVALID) for c in picks], out, rec)
        # accepted: a call that just fits (the whole capture; the output right behind the input's last byte), 16 points
        dev.excise_chirp_dev(cap, cap.nbytes, 0, cap.nsamples, 256, rt, t256, out, rec)
        dev.excise_chirp_dev(out, 2 * n, 0, n, 256, rt, t256, out.ptr + 2 * n, None)
        dev.excise_chirp_dev(cap, cap.nbytes, cap.nsamples - 16, 16, 16, rt, t16, out, rec)
        dev.synchronize()
        out.check_pads("output")
        rec.check_pads("records")
    finally:
        freed(out, rec)


def pick(dev, records, rate_first, rate_step, minc):
    """gj_chirp_rates_dev on host records, into a sentinel-filled buffer."""
    records = np.ascontiguousarray(records, gpsjam.CHIRP_DTYPE)
    scan, out = dev.alloc(records.nbytes), Guarded(dev, 4 * records.size)
    try:
        scan.upload(records)
        dev.chirp_rates_dev(scan, records.size, rate_first, rate_step, minc, out)
        out.check_pads("rates")
        return out.read(np.int32)
    finally:
        freed(scan, out)


def test_rate_picker_gives_the_restatements_integers(dev, caps):
    # made-up records: the float32 product, one ulp either side of it, no power, NaN, a sum that wraps
    minc = xr.MIN_CONCENTRATION
    rng = np.random.default_rng(3)
    n = 5000                                                        # more than one workgroup
    rec = np.zeros(n, gpsjam.CHIRP_DTYPE)
    total = rng.uniform(1.0, 1e6, n).astype(np.float32)
    need = np.float32(minc) * total
    rec["total"] = total
    rec["peak"] = np.where(np.arange(n) % 3 == 0, need, np.where(np.arange(n) % 3 == 1, np.nextafter(need, np.float32(0)),
                                                                 (minc * total.astype(np.float64)).astype(np.float32)))
    rec["rate_index"] = rng.integers(0, 256, n)
    rec["total"][[5, 6]], rec["peak"][[5, 6]] = (0.0, np.nan), (0.0, 1.0)
    rec["total"][7], rec["peak"][7] = 1.0, np.nan
    rec["rate_index"][8], rec["total"][8], rec["peak"][8] = 2 ** 31 - 1, 1.0, 1.0
    for first, step in ((-9, 1), (2 ** 31 - 100, 3), (-2 ** 31, 2 ** 24)):
        want = xr.chirp_rates(rec, first, step, minc)
        assert 0.2 < np.mean(want != 0) < 0.8
        np.testing.assert_array_equal(pick(dev, rec, first, step, minc), want)
    # a real scan of the parity input on the excisor's frames, resident from the search to the rates
    for nfft in (64, 1024):
        cap = caps(nfft)
        first, step, n_rates = xr.parity_scan_rates(nfft)
        nf = gpsjam.excise_frames(cap.nsamples - xr.PARITY_FIRST, nfft)
        scan, out = dev.alloc(nf * gpsjam.CHIRP_DTYPE.itemsize), dev.alloc(4 * nf)
        try:
            dev.chirp_dev(cap, cap.nbytes, xr.PARITY_FIRST, nfft, nfft // 2, nf, 2, first, step, n_rates, scan)
            dev.chirp_rates_dev(scan, nf, first, step, minc, out)
            got, records = out.download(np.int32), scan.download(gpsjam.CHIRP_DTYPE, nf)
        finally:
            scan.free()
            out.free()
        np.testing.assert_array_equal(got, xr.chirp_rates(records, first, step, minc))
        np.testing.assert_array_equal(got, xr.chirp_rates(xr.parity_scan(nfft).records, first, step, minc))
    # no power at all: an all-128 capture under the 128 convention has total 0 in every frame, and every rate is 0
    try:
        dev.set_unpack(128.0, 1.0 / 128.0)
        scan = dev.chirp(np.full(2 * 64 * 9, 128, np.uint8), nfft=64, rates=(3, 1, 4))
    finally:
        dev.set_unpack()
    assert len(scan.records) == 17 and not scan.records["total"].any()
    assert not pick(dev, scan.records, 3, 1, minc).any() and not pick(dev, scan.records, 3, 1, 0.0).any()


def test_device_excise_chirp(dev, caps):
    nfft = 256
    cap, raw = caps(nfft), xr.parity_capture(nfft)
    nf = gpsjam.excise_frames(cap.nsamples, nfft)
    rates, thr = xr.parity_rates(nfft, nf), xr.parity_threshold(nfft)
    want = xr.excise_chirp(raw, thr, rates, nfft)
    uploads, calls = gpsjam.Capture.uploads, dev.kernel_calls.get("excise_chirp", 0)
    a, rec_a = dev.excise_chirp(cap, thr, rates, nfft=nfft)
    assert gpsjam.Capture.uploads == uploads, "a cleaned capture is no host->device pass"
    b, rec_b = dev.excise_chirp(raw, thr, rates.tolist(), nfft=nfft)
    try:
        assert dev.kernel_calls["excise_chirp"] == calls + 2
        assert isinstance(a, gpsjam.Capture) and a.nbytes == cap.nbytes and a.ptr != cap.ptr
        assert a.download().tobytes() == b.download().tobytes() and rec_a.tobytes() == rec_b.tobytes()
        xr.compare(a.download(), rec_a, want, "Device.excise_chirp")
        part, rec_p = dev.excise_chirp(cap, thr, rates[3:3 + gpsjam.excise_frames(5000, nfft)], nfft=nfft, first_sample=128 * 3,
                                       n_samples=5000)
        assert part.nbytes == 10000 and rec_p.tobytes() == rec_a[3:3 + rec_p.size].tobytes()
        part.free()
        ridge = dev.ridge(a, nfft=nfft)                                    # the resident result goes wherever a Capture goes
        assert len(ridge) == gpsjam.ridge_frames(a.nbytes, 0, nfft, nfft // 2)
        assert ridge.total.sum() < dev.ridge(cap, nfft=nfft).total.sum()
        with pytest.raises(ValueError):
            dev.excise_chirp(cap, thr, rates[:-1], nfft=nfft)
        with pytest.raises(ValueError):
            dev.excise_chirp(cap, np.zeros(nfft + 1), rates, nfft=nfft)
    finally:
        a.free()
        b.free()


def test_clean_swept_leaves_a_tone_to_clean(dev):
    """The e2e capture of the plain excisor's test: a steady tone is no sweep, clean_swept returns clean's bytes and makes no
    call of the chirp-domain excisor."""
    raw = er.e2e_capture("tone")
    args = dict(nfft=er.E2E_NFFT, rise_db=er.E2E_RISE_DB, fs=er.FS, **er.E2E_ONSET_ARGS)
    with dev.capture(raw) as c:
        calls = dict(dev.kernel_calls)
        got = mitigate.clean_swept(dev, c, max_sweep_hz_per_s=xr.E2E_MAX_SWEEP, **args)
        after = dict(dev.kernel_calls)
        want = mitigate.clean(dev, c, **args)
    try:
        assert isinstance(got, mitigate.CleanedSwept) and not got.swept and got.sweep_hz_per_s is None
        assert after.get("excise_chirp", 0) == calls.get("excise_chirp", 0) and after["excise"] == calls.get("excise", 0) + 1
        assert got.capture.download().tobytes() == want.capture.download().tobytes()
        assert got.records.tobytes() == want.records.tobytes() and np.array_equal(got.threshold, want.threshold)
        assert got.floor_from == want.floor_from == "quiet part" and got.removed_share == want.removed_share > 0.5
        assert got.rates.dtype == np.int32 and got.rates.size == got.records.size and not got.rates.any()
    finally:
        got.capture.free()
        want.capture.free()


@pytest.fixture(scope="module")
def search(dev):
    s = gnss.AcqSearch(dev, prns=[p for p, *_ in er.E2E_SATS])
    yield s
    s.close()


def test_end_to_end_the_satellites_come_back_from_under_a_fast_sweep(dev, search):
    """Three C/A signals of 3 LSB in noise of sigma 10 LSB; from sample 2^17 on a 60-LSB saw-tooth of 4.008 GHz/s over
    1.6 MHz, whose period is shorter than a frame of 1024 points.  clean_swept finds the sweep itself; the tolerance is twice
    the 1.01 dB the CPU restatement lost (tests/test_excise_chirp_host.py), and mitigate.clean on the same capture must be
    worse by half the 11.97 dB the CPU measured."""
    raw, nfft, lead = xr.e2e_capture(True), xr.E2E_NFFT, er.E2E_LEAD
    args = dict(nfft=nfft, rise_db=er.E2E_RISE_DB, fs=xr.FS, **er.E2E_ONSET_ARGS)
    with dev.capture(xr.e2e_capture(False)) as c:
        free = search.search(c, first_sample=lead)
    assert all(r.acquired for r in free), free
    with dev.capture(raw) as c:
        before = search.search(c, first_sample=lead)
        res = mitigate.clean_swept(dev, c, max_sweep_hz_per_s=xr.E2E_MAX_SWEEP, **args)
        plain = mitigate.clean(dev, c, **args)
    try:
        after, worse = search.search(res.capture, first_sample=lead), search.search(plain.capture, first_sample=lead)
        cleaned = res.capture.download()
    finally:
        res.capture.free()
        plain.capture.free()
    assert not any(r.acquired for r in before), before
    unit256 = (xr.FS / xr.E2E_CHARACTERISE_NFFT) ** 2
    print(f"sweep {res.sweep_hz_per_s:.4g} Hz/s (truth {xr.E2E_SWEEP:.4g}), floor from the {res.floor_from}, "
          f"{100 * res.removed_share:.1f} % removed; rates {np.unique(res.rates)}")
    assert res.swept and abs(res.sweep_hz_per_s - xr.E2E_SWEEP) <= unit256
    h = nfft // 2
    quiet, on = lead // h - 1, lead // h          # frames that end in front of the onset; the first frame that starts behind it
    assert res.rates.size == res.records.size == gpsjam.excise_frames(raw.size // 2, nfft)
    assert not res.rates[:quiet].any()
    # nearly every frame of 1024 points holds a fly-back here and the CPU still found a rate on all of them; one frame in
    # eight may go without
    assert np.mean(res.rates[on:] != 0) >= 0.875
    assert np.all(np.abs(res.rates[on:][res.rates[on:] != 0] - xr.E2E_Q) <= 2 * xr.RATE_SPAN)
    for r, ref, w in zip(after, free, worse):
        print(f"PRN {r.prn}: C/N0 {r.cn0:.2f} chirp domain, {ref.cn0:.2f} jammer-free, {w.cn0:.2f} plain excisor")
        assert r.acquired and (r.code_index, r.freq_index) == (ref.code_index, ref.freq_index), (r, ref)
        assert abs(r.cn0 - ref.cn0) <= xr.E2E_CN0_TOL_DB, (r, ref)
        assert r.cn0 - w.cn0 >= xr.E2E_MIN_GAP_DB, (r, w)
    head = 2 * (lead - nfft)                      # every frame that ends in front of the jammer
    assert cleaned[:head].tobytes() == raw[:head].tobytes()
    assert 0.5 < res.removed_share < 1.0
