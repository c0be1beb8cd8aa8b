"""The pair alignment on the GPU (gj_align_dev, Device.align) and what is built on it: align.estimate and align.to.

This file sits in a package of its own on purpose, as tests/subtract/ does: the suite orders GPU files by basename
(tests/conftest.py SUITE_ORDER, which tests/test_suite_order.py holds every GPU file to), and under the name
test_round6_gpu.py it runs in stage 2.

Yardstick: the integer restatement of the definition in include/gpsjam.h (tests/align_restatement.py, which
tests/test_align_host.py holds to a per-sample Python-int loop).  Everything the kernel makes is integer arithmetic, so
EVERY byte and EVERY record is equal, bit for bit.  Every call writes into sentinel-filled buffers whose 256 bytes in
front of and behind the call's output must stay untouched.  The figures of the end-to-end test are held to what
tests/test_align_host.py measures on the CPU with the same host code on restated integers.  No capture here is longer
than 2^16 samples: the 64-bit products of the position are covered by the "far" cases, whose pos0 is the limit's.  More
tiles than workgroups, and n_out = 2^28, the limit itself, run in tests/tile_loops/."""
import numpy as np
import pytest

import align_restatement as ar
import gpsjam
from gpsjam import align, coherence
from gpu_lib import GJ_ERR_INVALID, GJ_ERR_UNSUPPORTED, PAD, SENTINEL, Guarded, freed, refused
from gpu_lib import run_align as run

pytestmark = pytest.mark.gpu



@pytest.fixture(scope="module")
def caps(dev):
    held = {kind: dev.capture(ar.parity_capture(kind)) for kind in ("random", "zeros", "full")}
    yield held
    for c in held.values():
        c.free()


@pytest.fixture(scope="module")
def d_tables(dev):
    """kind -> (taps, rot) on the device, both 256-byte aligned."""
    held = {}
    for kind in ("wide", "mid", "worst", "delta"):
        t, r = ar.tables(kind)
        held[kind] = (dev.alloc(t.nbytes).upload(t), dev.alloc(r.nbytes).upload(r))
    yield held
    for t, r in held.values():
        t.free()
        r.free()


def compare(dev, cap, raw, case, kind, d_tables, n_out, first=0, **how):
    """The call on samples ``first`` .. of the capture (a slice: d_iq moves, nbytes shrinks) against the restatement."""
    got, rec = run(dev, cap.ptr + 2 * first, cap.nbytes - 2 * first, case, *d_tables[kind], n_out, **how)
    want, wrec = ar.align(raw[2 * first:], *case, *ar.tables(kind), n_out)
    what = f"case {case} tables {kind} n_out {n_out} first {first} {how}"
    np.testing.assert_array_equal(got, want, err_msg=what)
    if rec is not None:
        assert rec.tobytes() == wrec.tobytes(), what
    return got, rec


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("kind", ["wide", "mid"])
def test_every_size_at_every_edge(dev, caps, d_tables, kind):
    raw = ar.parity_capture()
    for n in ar.SIZES:
        for case in ar.CASES.values():
            compare(dev, caps["random"], raw, case, kind, d_tables, n)


@pytest.mark.parametrize("kind", ["wide", "mid"])
def test_output_off_alignment_source_at_an_odd_sample_records_off_and_twice(dev, caps, d_tables, kind):
    raw, n = ar.parity_capture(), 3 * 4096 + 5
    for name in ("fastest step", "slowest step", "rounding carries into k", "ends past the source's end"):
        case = ar.CASES[name]
        got, rec = compare(dev, caps["random"], raw, case, kind, d_tables, n)
        again, _ = run(dev, caps["random"], caps["random"].nbytes, case, *d_tables[kind], n)
        assert got.tobytes() == again.tobytes(), "two calls, identical bytes"
        bare, none = compare(dev, caps["random"], raw, case, kind, d_tables, n, records=False)
        assert none is None and bare.tobytes() == got.tobytes(), "records off: the same bytes"
        for off in (1, 2, 15):
            moved, mrec = compare(dev, caps["random"], raw, case, kind, d_tables, n, out_offset=off)
            assert moved.tobytes() == got.tobytes() and mrec.tobytes() == rec.tobytes(), off
        for first in (1, 7, 300):                              # d_iq is 2, 14 and 8 bytes past a 16-byte boundary
            for size in (17, 4097, n - 300):
                compare(dev, caps["random"], raw, case, kind, d_tables, size, first=first)
                compare(dev, caps["random"], raw, case, kind, d_tables, size, first=first, out_offset=2, records=False)


@pytest.mark.parametrize("capture", ["zeros", "full"])
def test_saturated_captures_reach_the_bounds_and_the_clamp(dev, caps, d_tables, capture):
    raw = ar.parity_capture(capture)
    for kind in ("worst", "wide", "mid"):
        for name in ("identity time base", "negative start", "fastest step"):
            got, rec = compare(dev, caps[capture], raw, ar.CASES[name], kind, d_tables, 4096 + 9)
        if kind != "mid":
            assert int(rec["n_clipped"].sum()) > 4096
    got, rec = compare(dev, caps[capture], raw, (20 << 32, ar.ONE, 0, 0), "worst", d_tables, 40)
    assert np.all(got[0::2] == 128) and set(got[1::2].tolist()) == {0 if capture == "zeros" else 255} and int(rec["n_clipped"][0]) == 40


# ------------------------------------------------------------------------------------------------ 2. properties
def test_identity_whole_sample_shifts_and_a_sub_range(dev, caps, d_tables):
    raw, n = ar.parity_capture(), ar.PARITY_SAMPLES
    for capture in ("random", "zeros", "full"):
        got, rec = compare(dev, caps[capture], ar.parity_capture(capture), ar.CASES["identity time base"], "delta", d_tables, n)
        assert got.tobytes() == ar.parity_capture(capture).tobytes() and not rec["n_clipped"].any() and rec["n_edge"].tolist() == [7, 0, 0, 8]
    for shift in (37, -4100, n - 3):
        got, _ = compare(dev, caps["random"], raw, (shift << 32, ar.ONE, 0, 0), "delta", d_tables, n)
        lo, hi = max(0, -shift), min(n, n - shift)
        assert np.all(got[:2 * lo] == 128) and np.all(got[2 * hi:] == 128) and got[2 * lo:2 * hi].tobytes() == raw[2 * (lo + shift):2 * (hi + shift)].tobytes()
    pos0, step, ph, st = ar.CASES["fastest step"]
    whole, _ = compare(dev, caps["random"], raw, (pos0, step, ph, st), "mid", d_tables, 2 * 4096 + 77)
    for n1, m in ((1, 50), (4095, 3), (4096, 4096 + 77), (5000, 1)):
        part, _ = compare(dev, caps["random"], raw, (pos0 + n1 * step, step, (ph + n1 * st) & 0xFFFFFFFF, st), "mid", d_tables, m)
        assert part.tobytes() == whole[2 * n1:2 * (n1 + m)].tobytes(), (n1, m)


# ------------------------------------------------------------------------------------------------ 3. refusals
def test_refusals_write_nothing(dev, caps, d_tables):
    cap, raw = caps["random"], ar.parity_capture()
    d_taps, d_rot = d_tables["mid"]
    n = 2 * 4096 + 5
    out, d_rec = Guarded(dev, 2 * n), Guarded(dev, 16 * 3)
    try:
        I, U = GJ_ERR_INVALID, GJ_ERR_UNSUPPORTED
        P = gpsjam.AlignParams
        ok = dict(d_iq=cap, nbytes=cap.nbytes, params=P(3 << 32, ar.ONE + 99, 1, 2, 0), d_taps=d_taps, d_rot=d_rot, n=n, d_out=out, d_blocks=d_rec)
        cases = [(dict(d_iq=0), I), (dict(d_taps=0), I), (dict(d_rot=0), I), (dict(d_out=0), I),
                 (dict(d_iq=cap.ptr + 1, nbytes=cap.nbytes - 2), I),                 # odd d_iq
                 (dict(d_taps=d_taps.ptr + 2), I), (dict(d_rot=d_rot.ptr + 2), I),   # tables not 4-byte aligned
                 (dict(d_taps=d_taps.ptr + 1), I), (dict(d_rot=d_rot.ptr + 3), I),
                 (dict(d_blocks=d_rec.ptr + 4), I),                                  # d_blocks not 8-byte aligned
                 (dict(params=P(3 << 32, ar.ONE, 1, 2, 1)), I),                      # reserved
                 (dict(params=P(3 << 32, ar.ONE, 1, 2, 1 << 63)), I),
                 (dict(d_out=cap), I),                                               # in place
                 (dict(d_out=cap.ptr + cap.nbytes - 2), I),                          # the output's first bytes are the source's last
                 (dict(d_iq=out.ptr + 30, nbytes=64, n=16, d_out=out), I),           # the output's last bytes are the source's first
                 (dict(params=P(0, ar.ONE + ar.MAX_DRIFT + 1, 0, 0, 0)), U), (dict(params=P(0, ar.ONE - ar.MAX_DRIFT - 1, 0, 0, 0)), U),
                 (dict(params=P(0, 0, 0, 0, 0)), U), (dict(params=P(0, 2 ** 64 - 1, 0, 0, 0)), U),
                 (dict(params=P(1 << 60, ar.ONE, 0, 0, 0)), U), (dict(params=P(-(1 << 60), ar.ONE, 0, 0, 0)), U),
                 (dict(params=P(-(1 << 63), ar.ONE, 0, 0, 0)), U), (dict(params=P((1 << 63) - 1, ar.ONE, 0, 0, 0)), U),
                 (dict(n=0), U), (dict(n=2 ** 28 + 1), U), (dict(n=2 ** 63), U)]
        def launch(a):
            dev.align_dev(a["d_iq"], a["nbytes"], a["params"], a["d_taps"], a["d_rot"], a["n"], a["d_out"], a["d_blocks"])
        for change, status in cases:                         # nothing written behind each one of them
            refused(dev, launch, [((dict(ok, **change),), status)], out, d_rec)
        assert cap.download().tobytes() == raw.tobytes(), "the capture is as it was"
        # accepted: the limits themselves, and an output that ends where the source begins
        dev.align_dev(cap, cap.nbytes, P((1 << 60) - 1, ar.ONE + ar.MAX_DRIFT, 0, 0, 0), d_taps, d_rot, 1, out, None)
        dev.align_dev(cap, cap.nbytes, P(-(1 << 60) + 1, ar.ONE - ar.MAX_DRIFT, 0, 0, 0), d_taps, d_rot, 16, out.ptr + 64, d_rec)
        dev.align_dev(out.ptr + 96, 64, P(0, ar.ONE, 0, 0, 0), d_taps, d_rot, 16, out.ptr + 64, None)
        dev.synchronize()
        assert np.all(out.download(np.uint8, out.nbytes - 96 + PAD, 96) == SENTINEL) and np.all(d_rec.download(np.uint8, PAD, 16) == SENTINEL)
        out.check_pads("output")
        d_rec.check_pads("records")
    finally:
        freed(out, d_rec)
    # the next valid call gives the parity bytes, and a library refusal through the wrapper raises and leaves the capture alone
    compare(dev, cap, raw, ar.CASES["fastest step"], "mid", d_tables, n)
    with pytest.raises(gpsjam.GpsJamError) as e:
        dev.align(cap, (0, ar.ONE + ar.MAX_DRIFT + 1, 0, 0), *ar.tables("mid"))
    assert e.value.status == GJ_ERR_UNSUPPORTED and cap.ptr


def test_device_align_is_the_restatement(dev, caps):
    raw, cap, tables, case = ar.parity_capture(), caps["random"], ar.tables("mid"), ar.CASES["slowest step"]
    uploads, calls = gpsjam.Capture.uploads, dev.kernel_calls.get("align", 0)
    out, rec = dev.align(cap, case, *tables, n_out=5000)
    assert gpsjam.Capture.uploads == uploads and dev.kernel_calls["align"] == calls + 1
    want, wrec = ar.align(raw, *case, *tables, 5000)
    assert out.nsamples == 5000 and out.download().tobytes() == want.tobytes() and rec.tobytes() == wrec.tobytes()
    out.free()
    host, hrec = dev.align(raw, gpsjam.AlignParams(*case, 0), *tables, n_out=5000)
    assert host.download().tobytes() == want.tobytes() and hrec.tobytes() == wrec.tobytes()
    host.free()
    same, _ = dev.align(cap, align.params(), align.taps(), align.rot_table())
    assert same.nsamples == cap.nsamples and same.download().tobytes() == raw.tobytes(), "the library's own tables: the identity"
    same.free()


# ------------------------------------------------------------------------------------------------ 4. end to end
def test_end_to_end_the_aligned_pair_is_as_coherent_as_a_pair_on_one_clock(dev):
    """estimate + to + coherence.scan on the 2^16-sample pair of tests/align_restatement.py: b is 3.25 samples late, 40
    ppm fast and 300 Hz off.  The bounds are those tests/test_align_host.py holds the same host code to on restated
    integers (it measured 0.006 sample, 0.11 ppm and 0.12 Hz, and a median MSC 0.005 under the one-clock pair's)."""
    raw_a, raw_b, raw_same = ar.e2e_pair()
    bins = ar.band_bins()

    def band_median(x, y):
        scan = coherence.scan(dev, x, y, fs=ar.FS, nfft=ar.E2E_NFFT, frames_per_row=ar.E2E_FRAMES)
        return float(np.median(scan.result.msc[0, bins])), scan

    with dev.capture(raw_a) as a, dev.capture(raw_b) as b, dev.capture(raw_same) as same:
        uploads = gpsjam.Capture.uploads
        est = align.estimate(dev, a, b, fs=ar.FS, max_offset_hz=1000.0)
        print(f"lag {est.lag:.4f} (truth {ar.E2E_LAG}), drift {est.drift * 1e6:.3f} ppm (truth {ar.E2E_DRIFT * 1e6}), offset {est.offset_hz:.3f} Hz "
              f"(truth {ar.E2E_OFFSET_HZ}); search {est.coarse_offset_hz:.2f} Hz, lags {est.coarse_lags}; spread {est.spread:.4f}")
        assert est.ok
        assert abs(est.lag - ar.E2E_LAG) <= ar.E2E_TOL_LAG
        assert abs(est.drift - ar.E2E_DRIFT) <= ar.E2E_TOL_DRIFT
        assert abs(est.offset_hz - ar.E2E_OFFSET_HZ) <= ar.E2E_TOL_OFFSET_HZ
        with align.to(dev, a, b, est, fs=ar.FS) as aligned:
            assert gpsjam.Capture.uploads == uploads, "nothing leaves or enters HBM but tables and records"
            assert aligned.nsamples == a.nsamples
            p = align.params(est.lag, est.drift, est.offset_hz, ar.FS)
            want, _ = ar.align(raw_b, p.pos0, p.pos_step, p.rot_phase, p.rot_step, align.taps(), align.rot_table(), a.nsamples)
            assert aligned.download().tobytes() == want.tobytes()
            raw_msc, raw_scan = band_median(a, b)
            got_msc, got_scan = band_median(a, aligned)
            one_msc, _ = band_median(a, same)
        thr = coherence.threshold(ar.E2E_FRAMES)
        print(f"median MSC in the band: raw pair {raw_msc:.4f} (threshold {thr:.4f}), aligned {got_msc:.4f}, one clock {one_msc:.4f}")
        assert raw_msc < thr and not raw_scan.detection.flagged.any()
        assert abs(got_msc - one_msc) <= ar.E2E_TOL_MSC
        flagged = np.flatnonzero(got_scan.detection.flagged)
        assert set(bins.tolist()) <= set(flagged.tolist()) and flagged.min() >= bins[0] - 3 and flagged.max() <= bins[-1] + 3
