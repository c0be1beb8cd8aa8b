"""The time-domain pulse blanker (gj_blank_dev, Device.blank, mitigate.clean_pulsed) on the GPU.

This file sits in a package of its own on purpose, as tests/excise/ does: the suite orders GPU files by basename
(tests/conftest.py SUITE_ORDER, which tests/test_suite_order.py holds every GPU file to), and under the name
test_round6_gpu.py it runs in stage 2.

Yardstick: the int64 restatement of the definition in include/gpsjam.h (tests/blank_restatement.py, which
tests/test_blank_host.py holds to a per-sample double loop).  Everything is integer arithmetic, so EVERY byte and EVERY
record field is equal.  Every call writes into a sentinel-filled buffer whose bytes behind 2 * n_samples and behind
d_blocks[blocks] must stay untouched."""
import math

import numpy as np
import pytest

import blank_restatement as br
import excise_restatement as er
import gpsjam
from gpsjam import gnss, mitigate
from gpu_lib import GJ_ERR_INVALID, GJ_ERR_UNSUPPORTED, Guarded, freed, refused
from gpu_lib import run_blank as run

pytestmark = pytest.mark.gpu

REC = gpsjam.BLANK_DTYPE.itemsize


@pytest.fixture(scope="module")
def cap(dev):
    c = dev.capture(br.parity_capture())
    yield c
    c.free()


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("guard", br.PARITY_GUARDS)
@pytest.mark.parametrize("window", br.PARITY_WINDOWS)
def test_parity_with_the_restatement(dev, cap, window, guard):
    try:
        for offset, scale in br.CONVENTIONS:
            dev.set_unpack(offset, scale)
            want = br.parity_reference(window, guard, offset)
            got, rec = run(dev, cap, cap.nbytes, br.PARITY_FIRST, br.PARITY_SAMPLES, window, guard, br.PARITY_THRESHOLD)
            br.compare(got, rec, want, (window, guard, offset))
    finally:
        dev.set_unpack()
    assert dev.get_unpack() == (127.5, 1.0 / 127.5)


def test_infinity_never_blanks_and_records_are_optional(dev, cap):
    raw = br.parity_capture()
    body = raw[2 * br.PARITY_FIRST:2 * (br.PARITY_FIRST + br.PARITY_SAMPLES)]
    for thr in (np.inf, 3.0e38):
        got, rec = run(dev, cap, cap.nbytes, br.PARITY_FIRST, br.PARITY_SAMPLES, 1024, 1024, thr)
        assert got.tobytes() == body.tobytes() and not rec["removed"].any() and not rec["n_blanked"].any() and not rec["n_rising"].any()
        np.testing.assert_array_equal(rec["total"], br.parity_reference(16, 8).records["total"])
    want = br.parity_reference(16, 8)
    got, rec = run(dev, cap, cap.nbytes, br.PARITY_FIRST, br.PARITY_SAMPLES, 16, 8, br.PARITY_THRESHOLD, want_blocks=False)
    assert got.tobytes() == want.out.tobytes() and rec.size == 4, "d_blocks = NULL changes no byte"


# ------------------------------------------------------------------------------------------------ 2. strictness
def test_the_comparison_is_strict(dev):
    raw, W, n = br.strict_capture(), br.STRICT_WINDOW, br.STRICT_SAMPLES
    with dev.capture(raw) as c:
        at_b, at_r = run(dev, c, c.nbytes, 0, n, W, 0, br.STRICT_THRESHOLD)
        below = float(np.nextafter(np.float32(br.STRICT_THRESHOLD), np.float32(0)))
        lo_b, lo_r = run(dev, c, c.nbytes, 0, n, W, 0, below)
    want_at, want_lo = br.blank(raw, br.STRICT_THRESHOLD, W, 0), br.blank(raw, below, W, 0)
    br.compare(at_b, at_r, want_at, "threshold = e / 4")
    br.compare(lo_b, lo_r, want_lo, "one ulp below")
    assert not at_r["n_blanked"].any() and at_b.tobytes() == raw.tobytes(), "S = T everywhere in the interior: nothing is blanked"
    interior = slice(2 * W, 2 * (n - W))
    assert set(np.unique(lo_b[interior]).tolist()) == {127, 128} and int(lo_r["n_blanked"].sum()) == n - (W - 1)


# ------------------------------------------------------------------------------------------------ 3. tiny and ragged
@pytest.mark.parametrize("n", [1, 5, 4095, 4096, 4097])
def test_ranges_smaller_than_the_halo(dev, cap, n):
    raw = br.parity_capture()
    for first in (br.PARITY_FIRST, br.PARITY_FIRST + 997):
        for window, guard in ((1024, 1024), (16, 8)):
            want = br.blank(raw, br.PARITY_THRESHOLD, window, guard, first, n)
            got, rec = run(dev, cap, cap.nbytes, first, n, window, guard, br.PARITY_THRESHOLD)
            br.compare(got, rec, want, (n, first, window, guard))


# ------------------------------------------------------------------------------------------------ 4. sub-range, repetition
@pytest.mark.parametrize("window,guard", [(1, 0), (16, 8), (63, 1), (1024, 1024)])
def test_a_sub_range_reproduces_the_interior_and_a_repeated_call_every_byte(dev, cap, window, guard):
    first, n = br.PARITY_FIRST, br.PARITY_SAMPLES
    whole_b, whole_r = run(dev, cap, cap.nbytes, first, n, window, guard, br.PARITY_THRESHOLD)
    again_b, again_r = run(dev, cap, cap.nbytes, first, n, window, guard, br.PARITY_THRESHOLD)
    assert again_b.tobytes() == whole_b.tobytes() and again_r.tobytes() == whole_r.tobytes()
    try:
        for offset, scale in br.CONVENTIONS:                # under 127.5 the dither's parity is the absolute index's
            dev.set_unpack(offset, scale)
            whole_b, _ = run(dev, cap, cap.nbytes, first, n, window, guard, br.PARITY_THRESHOLD)
            for k, m in ((1001, 2 * br.BLOCK + 777), (4096, n - 4096), (8191, 4099)):      # odd k among them
                part_b, _ = run(dev, cap, cap.nbytes, first + k, m, window, guard, br.PARITY_THRESHOLD)
                lo, hi = window // 2 + guard, m - (window + guard)
                assert hi > lo and part_b[2 * lo:2 * hi].tobytes() == whole_b[2 * (k + lo):2 * (k + hi)].tobytes(), (window, guard, offset, k, m)
    finally:
        dev.set_unpack()


# ------------------------------------------------------------------------------------------------ 5. past 4 GiB
BIG = 2 ** 32 + 2 ** 20
WINDOW_AT = 2 ** 32 + 2                         # byte offset of the range: sample 2^31 + 1, an odd one
S0 = WINDOW_AT // 2
FAR_SAMPLES = 3 * br.BLOCK


@pytest.fixture(scope="module")
def big(dev):
    """4 GiB + 1 MiB, never filled: only the range that the test uploads is ever read.  An allocation failure fails."""
    b = dev.alloc(BIG)
    assert b.ptr and b.nbytes == BIG
    yield b
    b.free()


def test_a_range_past_sample_2_31(dev, big):
    assert WINDOW_AT > 2 ** 32 and S0 > 2 ** 31 and S0 % 2 == 1 and WINDOW_AT + 2 * FAR_SAMPLES <= BIG
    raw = br.parity_capture()[2 * br.PARITY_FIRST:2 * (br.PARITY_FIRST + FAR_SAMPLES)]
    big.upload(raw, offset=WINDOW_AT)
    assert big.download(np.uint8, 64, offset=WINDOW_AT).tobytes() == raw[:64].tobytes()
    for window, guard in ((16, 8), (1024, 1024)):
        want = br.blank(raw, br.PARITY_THRESHOLD, window, guard, 0, FAR_SAMPLES)
        odd = br.blank(np.concatenate((np.zeros(2, np.uint8), raw)), br.PARITY_THRESHOLD, window, guard, 1, FAR_SAMPLES)
        assert odd.out.tobytes() != want.out.tobytes(), "the dither tells an odd first_sample from an even one"
        got, rec = run(dev, big, BIG, S0, FAR_SAMPLES, window, guard, br.PARITY_THRESHOLD)
        br.compare(got, rec, odd, ("past 2^31", window, guard))
    # one sample past the buffer's end: refused, nothing written
    out = Guarded(dev, 2 * FAR_SAMPLES)
    try:
        refused(dev, dev.blank_dev, [((big, BIG, first, FAR_SAMPLES, 16, 8, br.PARITY_THRESHOLD, out, None), GJ_ERR_INVALID)
                                     for first in (BIG // 2 - FAR_SAMPLES + 1, BIG // 2)], out)
    finally:
        out.free()


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_enqueue_nothing(dev, cap):
    n, thr = 3 * 4096, br.PARITY_THRESHOLD
    out, rec = Guarded(dev, cap.nbytes), Guarded(dev, 8 * REC)
    try:
        cases = [  # d_iq, nbytes, first, n_samples, window, guard, threshold, d_out, d_blocks, status
            (cap, cap.nbytes, 0, n, 0, 8, thr, out, rec, GJ_ERR_UNSUPPORTED),
            (cap, cap.nbytes, 0, n, -16, 8, thr, out, rec, GJ_ERR_UNSUPPORTED),
            (cap, cap.nbytes, 0, n, 1025, 8, thr, out, rec, GJ_ERR_UNSUPPORTED),
            (cap, cap.nbytes, 0, n, 16, -1, thr, out, rec, GJ_ERR_UNSUPPORTED),
            (cap, cap.nbytes, 0, n, 16, 1025, thr, out, rec, GJ_ERR_UNSUPPORTED),
            (cap, cap.nbytes, 0, 0, 16, 8, thr, out, rec, GJ_ERR_INVALID),                    # n_samples == 0
            (cap, cap.nbytes, 1, cap.nsamples, 16, 8, thr, out, rec, GJ_ERR_INVALID),         # runs past the capture
            (cap, cap.nbytes, cap.nsamples + 1, 16, 16, 8, thr, out, rec, GJ_ERR_INVALID),
            (cap, cap.nbytes, 2 ** 63, 2 ** 63 + 16, 16, 8, thr, out, rec, GJ_ERR_INVALID),    # first + n wraps
            (0, cap.nbytes, 0, n, 16, 8, thr, out, rec, GJ_ERR_INVALID),                      # null d_iq
            (cap.ptr + 1, cap.nbytes - 2, 0, n, 16, 8, thr, out, rec, GJ_ERR_INVALID),        # odd d_iq
            (cap, cap.nbytes, 0, n, 16, 8, thr, 0, rec, GJ_ERR_INVALID),                      # null d_out
            (cap, cap.nbytes, 0, n, 16, 8, thr, out, rec.ptr + 4, GJ_ERR_INVALID),            # d_blocks not 8-byte aligned
            (cap, cap.nbytes, 0, n, 16, 8, float("nan"), out, rec, GJ_ERR_INVALID),
            (cap, cap.nbytes, 0, n, 16, 8, -1.0, out, rec, GJ_ERR_INVALID),
            (cap, cap.nbytes, 0, n, 16, 8, -np.inf, out, rec, GJ_ERR_INVALID),
            # d_out inside the capture: in place, shifted, touching the last byte; the capture inside d_out
            (out, cap.nbytes, 0, n, 16, 8, thr, out, rec, GJ_ERR_INVALID),
            (out, cap.nbytes, 0, n, 16, 8, thr, out.ptr + 2 * n, rec, GJ_ERR_INVALID),
            (out, cap.nbytes, 0, n, 16, 8, thr, out.ptr + cap.nbytes - 1, rec, GJ_ERR_INVALID),
            (out.ptr + 512, 1024, 0, 256, 16, 8, thr, out.ptr + 1, rec, GJ_ERR_INVALID),
        ]
        refused(dev, dev.blank_dev, [(c[:-1], c[-1]) for c in cases], out, rec)
        # accepted: the whole capture; the output right behind the input's last byte; the limits; one sample
        dev.blank_dev(cap, cap.nbytes, 0, cap.nsamples, 1024, 1024, 0.0, out, rec)
        assert 4 * 4096 <= cap.nbytes
        dev.blank_dev(out, 2 * 4096, 0, 4096, 1, 0, thr, out.ptr + 2 * 4096, None)
        dev.blank_dev(cap, cap.nbytes, cap.nsamples - 1, 1, 16, 8, thr, out, rec)
        dev.synchronize()
        out.check_pads("output")
        rec.check_pads("records")
    finally:
        freed(out, rec)


def test_an_output_that_is_not_16_byte_aligned(dev, cap):
    """The kernel stores 16 bytes at a time into an aligned d_out and byte by byte into any other."""
    n = br.PARITY_SAMPLES
    want = br.parity_reference(16, 8)
    for shift in (1, 2, 8):
        out = Guarded(dev, 2 * n, offset=shift)
        try:
            dev.blank_dev(cap, cap.nbytes, br.PARITY_FIRST, n, 16, 8, br.PARITY_THRESHOLD, out, None)
            assert out.read().tobytes() == want.out.tobytes(), shift
            out.check_pads(f"output, {shift} bytes off alignment")
        finally:
            out.free()


# ------------------------------------------------------------------------------------------------ 7. the Python layers
def test_device_blank_and_mitigate_clean_pulsed(dev, cap):
    raw = br.parity_capture()
    want = br.blank(raw, br.PARITY_THRESHOLD, 16, 8)
    uploads = gpsjam.Capture.uploads
    a, rec_a = dev.blank(cap, br.PARITY_THRESHOLD)
    assert gpsjam.Capture.uploads == uploads, "a cleaned capture is no host->device pass"
    b, rec_b = dev.blank(raw, br.PARITY_THRESHOLD)
    try:
        assert isinstance(a, gpsjam.Capture) and a.nbytes == cap.nbytes and a.ptr != cap.ptr
        assert a.download().tobytes() == b.download().tobytes() and rec_a.tobytes() == rec_b.tobytes()
        br.compare(a.download(), rec_a, want, "Device.blank")
        part, rec_p = dev.blank(cap, br.PARITY_THRESHOLD, window=63, guard=1, first_sample=br.PARITY_FIRST, n_samples=br.PARITY_SAMPLES)
        assert part.nbytes == 2 * br.PARITY_SAMPLES
        br.compare(part.download(), rec_p, br.parity_reference(63, 1), "Device.blank on a range")
        part.free()
        # the resident result goes wherever a Capture goes
        ridge = dev.ridge(a, nfft=256)
        assert len(ridge) == gpsjam.ridge_frames(a.nbytes, 0, 256, 128)
        assert ridge.total.sum() < dev.ridge(cap, nfft=256).total.sum()
        psd, _ = dev.welch(a, chunk_samples=a.nsamples, nperseg=256, want_db=False)
        raw_psd, _ = dev.welch(cap, chunk_samples=cap.nsamples, nperseg=256, want_db=False)
        assert psd.shape == raw_psd.shape and psd.shape[1] == 256 and psd.sum() < raw_psd.sum()
    finally:
        a.free()
        b.free()

    # clean_pulsed: the three sources of the floor, each against the host arithmetic on K4's and K1's own outputs
    jammed = br.e2e_capture("gated noise")
    with dev.capture(jammed) as c:
        on = dev.onset(c, **er.E2E_ONSET_ARGS)
        uploads = gpsjam.Capture.uploads
        quiet = mitigate.clean_pulsed(dev, c, **br.E2E_ONSET_ARGS)
        assert gpsjam.Capture.uploads == uploads
        host = mitigate.clean_pulsed(dev, jammed, **br.E2E_ONSET_ARGS)
        given = mitigate.clean_pulsed(dev, c, window=32, guard=4, threshold=1234.5)
    try:
        assert on.start_index >= er.E2E_ONSET_ARGS["noise_samples"]
        assert quiet.floor_from == host.floor_from == "quiet part"
        assert quiet.threshold == float(np.float32(float(on.noise_power) * 10.0 ** 0.6))
        assert isinstance(quiet.capture, gpsjam.Capture) and quiet.capture.nbytes == jammed.size
        assert quiet.capture.download().tobytes() == host.capture.download().tobytes() and quiet.records.tobytes() == host.records.tobytes()
        assert quiet[2:] == host[2:]
        br.compare(quiet.capture.download(), quiet.records, br.blank(jammed, quiet.threshold, 16, 8), "clean_pulsed, quiet part")
        assert quiet.removed_share == int(quiet.records["removed"].sum()) / int(quiet.records["total"].sum())
        assert quiet.blanked_share == int(quiet.records["n_blanked"].sum()) / (jammed.size // 2)
        assert given.floor_from == "given" and given.threshold == 1234.5
        br.compare(given.capture.download(), given.records, br.blank(jammed, 1234.5, 32, 4), "clean_pulsed, given")
    finally:
        for r in (quiet, host, given):
            r.capture.free()
    # jammed from sample 0: K4 finds no onset behind its noise estimate, the floor is K1's 25th percentile
    always = jammed[2 * er.E2E_LEAD:]
    with dev.capture(always) as c:
        low = mitigate.clean_pulsed(dev, c, **br.E2E_ONSET_ARGS)
        n_chunks = always.size // 128
        d_pow, d_stats = dev.alloc(4 * n_chunks), dev.alloc(12)
        try:
            dev.chunk_power_dev(c, always.size // 128 * 128, 128, d_pow, eps=0.0)
            dev.power_threshold_dev(d_pow, n_chunks, d_stats, None, pct=25.0, rise_db=0.0)
            power, floor = d_pow.download(np.float32, n_chunks), float(d_stats.download(np.float32, 3)[0])
        finally:
            d_pow.free()
            d_stats.free()
    try:
        true = 2.0 * er.E2E_SIGMA ** 2 + 27.0
        print(f"low percentile: floor {floor:.2f} LSB^2 against {true:.0f} ({10 * math.log10(floor / true):+.2f} dB), threshold {low.threshold:.2f}, "
              f"blanked share {low.blanked_share:.4f}")
        assert low.floor_from == "low percentile" and low.threshold == float(np.float32(floor * 10.0 ** 0.6))
        assert floor == pytest.approx(float(np.percentile(power, 25.0)), rel=1e-6) and -0.5 < 10 * math.log10(floor / true) < 0.0
        br.compare(low.capture.download(), low.records, br.blank(always, low.threshold, 16, 8), "clean_pulsed, low percentile")
        assert 0.25 < low.blanked_share < 0.4
    finally:
        low.capture.free()


# ------------------------------------------------------------------------------------------------ 8. end to end
@pytest.fixture(scope="module")
def search(dev):
    s = gnss.AcqSearch(dev, prns=[p for p, *_ in er.E2E_SATS])
    yield s
    s.close()


@pytest.fixture(scope="module")
def jammer_free(dev, search):
    with dev.capture(br.e2e_capture(None)) as c:
        res = search.search(c, first_sample=er.E2E_LEAD)
    assert all(r.acquired for r in res), res
    return res


@pytest.mark.parametrize("kind", br.E2E_KINDS)
def test_end_to_end_the_satellites_come_back(dev, search, jammer_free, kind):
    """Three C/A signals of 3 LSB in noise of sigma 10 LSB; from sample 2^17 on a 110-LSB jammer gated at 1 kHz and 30 %
    duty: a carrier (the simulator's pulsedJammer.py), noise, or a sweep of 20 MHz in 10 us.  mitigate.clean_pulsed at
    its defaults.  What is left of the C/N0 loss once the blanked samples are accounted for, 10 log10(1 - share), must
    lie within br.E2E_CN0_TOL_DB: twice the 0.435 dB that the restatement and the oracle's acquisition gave on the CPU
    (tests/test_blank_host.py)."""
    raw = br.e2e_capture(kind)
    n, lead, window, guard = raw.size // 2, er.E2E_LEAD, 16, 8
    with dev.capture(raw) as c:
        before = search.search(c, first_sample=lead)
        res = mitigate.clean_pulsed(dev, c, **br.E2E_ONSET_ARGS)
        plain = mitigate.clean(dev, c, nfft=br.E2E_EXCISOR_NFFT, rise_db=br.E2E_EXCISOR_RISE_DB, fs=er.FS, **er.E2E_ONSET_ARGS) if kind != "gated carrier" else None
    try:
        assert res.floor_from == "quiet part" and res.capture.nbytes == raw.size
        after = search.search(res.capture, first_sample=lead)
        cleaned = res.capture.download()
        excised = search.search(plain.capture, first_sample=lead) if plain is not None else None
    finally:
        res.capture.free()
        if plain is not None:
            plain.capture.free()
    quiet = 2 * (lead - window - guard)
    assert cleaned[:quiet].tobytes() == raw[:quiet].tobytes(), "no quiet sample is blanked"
    share = br.e2e_blanked_share(res.records, n)
    predicted = 10.0 * math.log10(1.0 - share)
    print(f"{kind}: threshold {res.threshold:.1f} LSB^2, {100 * share:.2f} % of the jammed part blanked on {int(res.records['n_rising'].sum())} "
          f"rising edges: {predicted:.2f} dB predicted")
    for k, (r, ref, b) in enumerate(zip(after, jammer_free, before)):
        resid = br.e2e_residual_db(r.cn0, ref.cn0, share)
        print(f"{kind} PRN {r.prn}: C/N0 {ref.cn0:.2f} jammer-free, {b.cn0:.2f} jammed, {r.cn0:.2f} blanked (residual {resid:+.3f} dB)"
              + (f", {excised[k].cn0:.2f} after mitigate.clean" if excised is not None else ""))
        assert ref.cn0 - b.cn0 >= br.E2E_MIN_LOSS_DB, (b, ref)
        assert r.acquired and r.code_index == ref.code_index and abs(r.freq_index - ref.freq_index) <= 1, (r, ref)
        assert abs(resid) <= br.E2E_CN0_TOL_DB, (r, ref, share, resid)
        if excised is not None:
            assert r.cn0 > excised[k].cn0, (r, excised[k])
