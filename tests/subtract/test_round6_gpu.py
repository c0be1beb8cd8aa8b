"""The counterfeit-signal subtraction on the GPU (gj_subtract_dev, Device.subtract) and what is built on it:
spoof.remove and mitigate.clean_spoofed.

This file sits in a package of its own on purpose, as tests/corr/ does: the suite orders GPU files by basename
(tests/conftest.py SUITE_ORDER, which tests/test_suite_order.py holds every GPU file to), and under the name
test_round6_gpu.py it runs in stage 2.

Yardstick: the integer restatement of the definition in include/gpsjam.h (tests/subtract_restatement.py, which
tests/test_subtract_host.py holds to a per-sample Python-int loop).  Everything the kernel makes is integer arithmetic,
so EVERY byte and EVERY record is equal, bit for bit.  Every call writes into sentinel-filled buffers whose 256 bytes in
front of and behind the call's output must stay untouched.  The float figures of the end-to-end test are held to what
tests/test_subtract_host.py measures on the CPU with the same host code on restated integers.  A range that starts
above sample 2^31 is not run here (no fixture holds such a capture cheaply): the 64-bit dither key is covered on the
CPU, and on the GPU in tests/tile_loops/."""
import numpy as np
import pytest

import corr_restatement as cr
import gpsjam
import peaks_restatement as pr
import subtract_restatement as sr
from gpsjam import gnss, mitigate, spoof
from gpu_lib import GJ_ERR_INVALID, GJ_ERR_UNSUPPORTED, PAD, SENTINEL, Guarded, freed, refused
from gpu_lib import run_subtract as run

pytestmark = pytest.mark.gpu

SIZES = (1, 15, 16, 17, 4095, 4096, 4097, 3 * 4096 + 5)
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


@pytest.fixture(scope="module")
def cap(dev):
    c = dev.capture(cr.parity_capture())
    yield c
    c.free()


@pytest.fixture(scope="module")
def d_codes(dev):
    b = dev.alloc(cr.parity_codes().nbytes).upload(cr.parity_codes())
    yield b
    b.free()


def compare(dev, capture, raw, first, n, B, d_rows, codes, channels, amps, flags, seed, **how):
    got, rec = run(dev, capture, first, n, B, d_rows, len(codes), channels, amps, flags, seed, **how)
    want, wrec = sr.subtract(raw, first, n, B, codes, channels, amps, flags, seed)
    what = f"first {first} n {n} B {B} channels {len(channels)} flags {flags} seed {seed} {how}"
    np.testing.assert_array_equal(got, want, err_msg=what)
    if rec is not None:
        assert rec.tobytes() == wrec.tobytes(), what
    return got, rec


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("flags, seed", [(0, 0), (1, 0), (1, 0xC0FFEE11)])
def test_every_size_and_an_odd_start(dev, cap, d_codes, flags, seed):
    raw, codes, channels = cr.parity_capture(), cr.parity_codes(), cr.parity_channels(6)
    for n in SIZES:
        for first in (0, 7, cap.nsamples - n):                   # even, odd, and ending on the capture's last sample
            compare(dev, cap, raw, first, n, 256, d_codes, codes, channels, sr.random_amps(6, cr.blocks(n, 256), 2 ** 14, seed=n), flags, seed)


@pytest.mark.parametrize("B", [16, 48, 256, 2048, 4096])
def test_every_block_size(dev, cap, d_codes, B):
    """B = 48 does not divide the 4096 samples of a tile: blocks straddle tiles, never a thread's 16 samples."""
    raw, codes, channels = cr.parity_capture(), cr.parity_codes(), cr.parity_channels(4, seed=B)
    n = 3 * 4096 + 5
    amps = sr.random_amps(4, cr.blocks(n, B), 2 ** 14, seed=B)
    for flags in (0, 1):
        compare(dev, cap, raw, 7, n, B, d_codes, codes, channels, amps, flags, 3)
    compare(dev, cap, raw, 0, B + 1, B, d_codes, codes, channels, amps[:, :2], 1, 3)


@pytest.mark.parametrize("n_channels", [1, 2, 64])
def test_channel_counts_records_off_and_an_output_that_is_only_2_byte_aligned(dev, cap, d_codes, n_channels):
    raw, codes, channels = cr.parity_capture(), cr.parity_codes(), cr.parity_channels(n_channels, seed=n_channels)
    n = 3 * 4096 + 5
    amps = sr.random_amps(n_channels, cr.blocks(n, 256), 2 ** 14, seed=1)
    got, rec = compare(dev, cap, raw, 7, n, 256, d_codes, codes, channels, amps, 1, 5)
    again, _ = run(dev, cap, 7, n, 256, d_codes, 4, channels, amps, 1, 5)
    assert got.tobytes() == again.tobytes(), "two calls, identical bytes"
    bare, none = compare(dev, cap, raw, 7, n, 256, d_codes, codes, channels, amps, 1, 5, records=False)
    assert none is None and bare.tobytes() == got.tobytes(), "records off: the same bytes"
    for off in (2, 14, 1):
        moved, mrec = compare(dev, cap, raw, 7, n, 256, d_codes, codes, channels, amps, 1, 5, out_offset=off)
        assert moved.tobytes() == got.tobytes() and mrec.tobytes() == rec.tobytes(), off
    other, _ = compare(dev, cap, raw, 7, n, 256, d_codes, codes, channels, amps, 1, 6)
    assert other.tobytes() != got.tobytes(), "another seed, another dither"


# ------------------------------------------------------------------------------------------------ 2. amplitudes
def test_zero_amplitudes_are_the_identity(dev, cap, d_codes):
    raw, codes, channels = cr.parity_capture(), cr.parity_codes(), cr.parity_channels(64)
    n = 2 * 4096 + 77
    zero = np.zeros((64, cr.blocks(n, 2048), 2), np.int32)
    for flags, seed in ((0, 0), (1, 9)):
        got, rec = compare(dev, cap, raw, 3, n, 2048, d_codes, codes, channels, zero, flags, seed)
        assert got.tobytes() == raw[6:6 + 2 * n].tobytes() and not rec["removed"].any() and not rec["n_clipped"].any()


def test_the_largest_amplitudes_reach_int32s_edge_and_clamp_on_both_sides(dev, cap, d_codes):
    """64 times the same channel -- the all-ones row, a still carrier at table index 2 (C = S = 23) -- with (2^19, 2^19):
    R_I = 64 * 2^19 * 46, the header's bound, with the sign changing from block to block; R + d must not wrap.  Then
    the parity channels with random +-2^19, and INT32_MIN / INT32_MAX in place of -+2^19: the same bytes."""
    raw, codes = cr.parity_capture(), cr.parity_codes()
    n, B = 4096 + 300, 256
    nb = cr.blocks(n, B)
    same = [(0, 0, 2 << 28, 0, 3, 0)] * 64
    sign = np.where(np.arange(nb) % 2 == 0, 1, -1).astype(np.int32)
    edge = np.broadcast_to((sign * 2 ** 19)[None, :, None], (64, nb, 2))
    assert abs(int(sr.replica(0, n, B, codes, same, edge)[:, 0].max())) == sr.R_BOUND == -int(sr.replica(0, n, B, codes, same, edge)[:, 0].min())
    for flags in (0, 1):
        got, rec = compare(dev, cap, raw, 1, n, B, d_codes, codes, same, edge, flags, 0xFFFFFFFF)
        assert set(np.unique(got[0::2])) == {0, 255} and int(rec["n_clipped"].sum()) >= n, "every I byte is clamped, at 0 or at 255"
    channels = cr.parity_channels(64, seed=5)
    rng = np.random.default_rng(12)
    pm = np.where(rng.integers(0, 2, (64, nb, 2)) == 1, 2 ** 19, -2 ** 19).astype(np.int32)
    got, rec = compare(dev, cap, raw, 1, n, B, d_codes, codes, channels, pm, 1, 4)
    assert int(rec["n_clipped"].sum()) > 0 and {0, 255} <= set(np.unique(got))
    wide = np.where(pm > 0, INT32_MAX, INT32_MIN).astype(np.int32)
    clamped, crec = compare(dev, cap, raw, 1, n, B, d_codes, codes, channels, wide, 1, 4)
    assert clamped.tobytes() == got.tobytes() and crec.tobytes() == rec.tobytes(), "the clamp is part of the definition"
    over = np.where(pm > 0, 2 ** 19 + 1, -2 ** 19 - 1).astype(np.int32)
    assert compare(dev, cap, raw, 1, n, B, d_codes, codes, channels, over, 1, 4)[0].tobytes() == got.tobytes()


def test_a_negative_replica_is_floored(dev, cap, d_codes):
    """One channel with R = (32 aI, 0), another amplitude in every 16-sample block, no dither: -32800 + 32768 = -32
    goes to q = -1 where truncation toward zero gives 0."""
    raw, codes = cr.parity_capture(), cr.parity_codes()
    a = [-1, -1024, -1025, -3072, -3073, 1023, 1024, -2 ** 19, 2 ** 19]
    q = [0, 0, -1, -1, -2, 0, 1, -256, 256]
    assert [(32 * v + 32768) // 65536 for v in a] == q
    amps = np.array([[[v, 0] for v in a]], np.int32)
    n = 16 * len(a)
    got, _ = compare(dev, cap, raw, 40, n, 16, d_codes, codes, [(0, 0, 0, 0, 3, 0)], amps, 0, 0)
    src = raw[80:80 + 2 * n].astype(np.int64)
    assert np.array_equal(got[1::2], src[1::2]), "R_Q = 0"
    assert np.array_equal(got[0::2], np.clip(src[0::2] - np.repeat(q, 16), 0, 255))


# ------------------------------------------------------------------------------------------------ 3. refusals
def test_refusals_and_a_bad_channel_write_nothing(dev, cap, d_codes):
    raw, codes, channels = cr.parity_capture(), cr.parity_codes(), cr.parity_channels(64)
    rec = np.array(channels, gpsjam.CORR_CHANNEL_DTYPE)
    n, B = 2 * 4096 + 5, 256
    amps = sr.random_amps(64, cr.blocks(n, B), 2 ** 14)
    out, d_rec, d_ch, d_amp = Guarded(dev, 2 * n), Guarded(dev, 24 * 3), dev.alloc(rec.nbytes + 8), dev.alloc(amps.nbytes + 8)
    try:
        d_ch.upload(rec)
        d_amp.upload(amps)
        I, U = GJ_ERR_INVALID, GJ_ERR_UNSUPPORTED
        ok = dict(d_iq=cap, nbytes=cap.nbytes, first=0, n=n, B=B, d_codes=d_codes, rows=4, d_ch=d_ch, n_ch=64, d_amp=d_amp, flags=1,
                  seed=0, d_out=out, d_blocks=d_rec)
        cases = [(dict(d_iq=0), I), (dict(d_codes=0), I), (dict(d_ch=0), I), (dict(d_amp=0), I), (dict(d_out=0), I),
                 (dict(d_iq=cap.ptr + 1, nbytes=cap.nbytes - 2), I),                 # odd d_iq
                 (dict(d_codes=d_codes.ptr + 1, rows=3), I),                         # odd d_codes
                 (dict(d_ch=d_ch.ptr + 4), I),                                       # d_channels not 8-byte aligned
                 (dict(d_amp=d_amp.ptr + 2), I),                                     # d_amp not 4-byte aligned
                 (dict(d_blocks=d_rec.ptr + 4), I),                                  # d_blocks not 8-byte aligned
                 (dict(rows=0), I),                                                  # no code rows
                 (dict(flags=2), I), (dict(flags=3), I), (dict(flags=-1), I),        # unknown flag bits
                 (dict(first=cap.nsamples - n + 1), I),                              # a range past the capture
                 (dict(first=cap.nsamples + 1, n=1), I),
                 (dict(first=2 ** 64 - 16, n=32), I),                                # first + n wraps
                 (dict(d_out=cap), I),                                               # in place
                 (dict(d_out=cap.ptr + cap.nbytes - 2), I),                          # the output's first bytes are the capture's last
                 (dict(d_iq=out.ptr + 30, nbytes=64, n=16, d_out=out), I),           # the output's last bytes are the capture's first
                 (dict(B=0), U), (dict(B=24), U), (dict(B=4112), U), (dict(B=-256), U),
                 (dict(n_ch=0), U), (dict(n_ch=65), U),
                 (dict(n=0), U), (dict(nbytes=2 ** 40, n=2 ** 28 + 1), U)]
        def launch(a):
            dev.subtract_dev(a["d_iq"], a["nbytes"], a["first"], a["n"], a["B"], a["d_codes"], a["rows"], a["d_ch"], a["n_ch"],
                             a["d_amp"], a["flags"], a["seed"], a["d_out"], a["d_blocks"])
        for change, status in cases:                         # nothing written behind each one of them
            refused(dev, launch, [((dict(ok, **change),), status)], out, d_rec)
        assert cap.download().tobytes() == raw.tobytes(), "the capture is as it was"
        # channel fields live in device memory: the library cannot refuse them with a status, so the launch writes nothing
        bad = [(0, 1, 0, 0, 0, 1), (0, 1, 0, 0, 4, 0), (0, 1, 0, 0, -1, 0), (cr.PERIOD, 1, 0, 0, 0, 0), (0, 2 ** 34, 0, 0, 0, 0)]
        for ch in bad:
            for at in (0, 37, 63):
                table = list(channels)
                table[at] = ch
                d_ch.upload(np.array(table, gpsjam.CORR_CHANNEL_DTYPE))
                dev.subtract_dev(cap, cap.nbytes, 0, n, B, d_codes, 4, d_ch, 64, d_amp, 1, 0, out, d_rec)
                dev.synchronize()
                out.check_untouched(f"channel {ch} at {at}, output")
                d_rec.check_untouched(f"channel {ch} at {at}, records")
            # ... and the wrapper checks them on the host, before anything is uploaded
            with pytest.raises(gpsjam.GpsJamError) as e:
                dev.subtract(cap, channels[:2] + [ch], codes, np.zeros((3, cr.blocks(cap.nsamples, 256), 2), np.int32))
            assert e.value.status == GJ_ERR_INVALID and cap.ptr
        # accepted: the limits themselves, and an output that ends where the capture begins
        d_ch.upload(rec)
        dev.subtract_dev(cap, cap.nbytes, cap.nsamples - 1, 1, 4096, d_codes, 4, d_ch, 1, d_amp, 0, 0, out, None)
        dev.subtract_dev(cap, cap.nbytes, 0, 16, 16, d_codes, 4, d_ch, 64, d_amp, 1, 2 ** 32 - 1, out.ptr + 64, d_rec)
        dev.subtract_dev(out.ptr + 96, 64, 0, 16, 16, d_codes, 4, d_ch, 1, d_amp, 0, 0, out.ptr + 64, None)
        dev.synchronize()
        assert np.all(out.download(np.uint8, out.nbytes - 96 + PAD, 96) == SENTINEL) and np.all(d_rec.download(np.uint8, PAD, 24) == SENTINEL)
        out.check_pads("output")
        d_rec.check_pads("records")
    finally:
        freed(out, d_rec, d_ch, d_amp)
    # the next valid call gives the parity bytes, and a library refusal through the wrapper raises and leaves the capture alone
    compare(dev, cap, raw, 7, n, B, d_codes, codes, channels[:3], amps[:3], 1, 0)
    with pytest.raises(gpsjam.GpsJamError) as e:
        dev.subtract(cap, channels[:3], codes, np.zeros((3, cr.blocks(cap.nsamples, 24), 2), np.int32), block_samples=24)
    assert e.value.status == GJ_ERR_UNSUPPORTED and cap.ptr


def test_device_subtract_is_the_restatement(dev, cap):
    raw, codes, channels = cr.parity_capture(), cr.parity_codes(), cr.parity_channels(5)
    amps = sr.random_amps(5, cr.blocks(5000, 256), 2 ** 15)
    uploads, calls = gpsjam.Capture.uploads, dev.kernel_calls.get("subtract", 0)
    cleaned, rec = dev.subtract(cap, channels, codes, amps, first_sample=3, n_samples=5000, seed=21)
    assert gpsjam.Capture.uploads == uploads and dev.kernel_calls["subtract"] == calls + 1
    want, wrec = sr.subtract(raw, 3, 5000, 256, codes, channels, amps, sr.DITHER, 21)
    assert cleaned.nsamples == 5000 and cleaned.download().tobytes() == want.tobytes() and rec.tobytes() == wrec.tobytes()
    cleaned.free()
    host, hrec = dev.subtract(raw, channels, codes, amps, first_sample=3, n_samples=5000, seed=21)
    assert host.download().tobytes() == want.tobytes() and hrec.tobytes() == wrec.tobytes()
    host.free()
    # a sub-range that starts on a block reproduces the larger call's bytes: advanced channels, offset amplitudes
    from gpsjam import postcorr
    m0 = 6
    moved = [postcorr.advance(postcorr.Channel(*c), m0 * 256) for c in channels]
    part, _ = dev.subtract(cap, moved, codes, amps[:, m0:], first_sample=3 + m0 * 256, n_samples=5000 - m0 * 256, seed=21)
    assert part.download().tobytes() == want[2 * m0 * 256:].tobytes()
    part.free()


# ------------------------------------------------------------------------------------------------ 4. end to end
@pytest.fixture(scope="module")
def search(dev):
    s = gnss.AcqSearch(dev, prns=sorted(cr.E2E_PRNS + (1,)))         # PRNs 1 and 27 are not in the overpowered pair
    yield s
    s.close()


def test_end_to_end_the_receiver_goes_back_to_the_authentic_signals(dev, search):
    """The overpowered pair through the real K-peak search, the bank and the subtraction: ten removals, each within 6 dB
    (a factor of two on the residual amplitude) of the CPU chain's smallest; the plain single-peak acquisition on cleaned
    a then finds all five PRNs where the authentic signals are; spoof.scan on the cleaned pair is not flagged and reads
    their phases and C/N0 within twice the CPU chain's errors.

    Where the authentic signals are: the code index within one sample and the Doppler bin nearest the truth -- for PRNs
    4, 9, 21 and 30 exactly that bin; for PRN 14 alone a bin either side.  The plain search stops at the first step that
    passes its threshold, for PRN 14 the first: one millisecond of coherent integration, whose main lobe is 1 kHz wide,
    where 200 Hz off the centre cost 0.6 dB.  tests/test_subtract_host.py
    (test_one_step_of_the_plain_search_resolves_the_doppler_to_a_bin_either_side) asserts on the oracle's one-step
    surface that PRN 14's +600 cell stands 3 % above its +400 cell on the cleaned capture (and that two steps give
    +400), and that the same yardstick puts PRNs 4 and 30 of the NEVER-spoofed pair one bin off at one step, with
    nothing of the subtraction in the path.  The code index is what tells the authentic signal (77.5) from the copy
    (571.5, in the SAME Doppler bin for this PRN)."""
    prns = [cr.E2E_PRNS[k] for k in pr.E2E_IDX]
    raw_a, raw_b = pr.overpowered_pair()
    freqs = gnss.doppler_bins()
    with dev.capture(raw_a) as a, dev.capture(raw_b) as b:
        before = {r.prn: r for r in search.search(a)}
        print("raw capture, single-peak acquisition:", {p: (before[p].acquired, before[p].code_index, before[p].doppler_hz) for p in prns})
        uploads = gpsjam.Capture.uploads
        res = mitigate.clean_spoofed(dev, a, b, k=2, search=search, tol=cr.E2E_TOL)
        assert gpsjam.Capture.uploads == uploads
        try:
            assert res.report.spoofed is True and sorted(r.prn for r in res.removals_a) == prns == sorted(r.prn for r in res.removals_b)
            for name, rows in (("a", res.removals_a), ("b", res.removals_b)):
                for r in rows:
                    print(f"antenna {name} PRN {r.prn}: code {r.code_index}, Doppler {r.doppler_hz:+.1f} Hz, C/N0 {r.cn0_before:.1f} -> "
                          f"{r.cn0_after:.1f} dB-Hz, suppression {r.suppression_db:.1f} dB (at least {sr.E2E_GPU_MIN_SUPPRESSION_DB:.2f})")
            for r in res.removals_a + res.removals_b:
                k = cr.E2E_PRNS.index(r.prn)
                assert abs(r.code_index - pr.spoof_code_index(k)) <= 1.0, "the counterfeit copy is what was removed"
                assert r.suppression_db >= sr.E2E_GPU_MIN_SUPPRESSION_DB, r
            assert res.capture_a.nsamples == cr.E2E_SAMPLES == res.capture_b.nsamples and res.records_a.size == sr.blocks(cr.E2E_SAMPLES)
            after = {r.prn: r for r in search.search(res.capture_a)}
            for k in pr.E2E_IDX:
                r = after[cr.E2E_PRNS[k]]
                print(f"cleaned PRN {r.prn}: acquired {r.acquired}, code {r.code_index} (truth {cr.E2E_CODE_INDEX[k]}), {r.doppler_hz:+.0f} Hz "
                      f"(truth {cr.E2E_DOPPLER[k]:+.0f}), peak ratio {r.peak_ratio:.2f}")
                assert r.acquired and abs(r.code_index - cr.E2E_CODE_INDEX[k]) <= 1.0, r
                nearest = int(np.argmin(np.abs(freqs - cr.E2E_DOPPLER[k])))
                if r.prn == 14:
                    assert abs(r.freq_index - nearest) <= 1, r
                else:
                    assert r.freq_index == nearest, r
            assert not after[1].acquired
            report = spoof.scan(dev, res.capture_a, res.capture_b, search, tol=cr.E2E_TOL)
            assert report.spoofed is False and report.prns == prns
            for prn, ph, c in zip(report.prns, report.phase, report.cn0):
                k = cr.E2E_PRNS.index(prn)
                e_ph, e_cn0 = abs(float(cr.wrap(ph - cr.E2E_AUTHENTIC[k]))), abs(c - cr.E2E_CN0[k])
                print(f"cleaned PRN {prn}: phase {ph:+.4f} (error {e_ph:.4f}, tolerance {sr.E2E_TOL_PHASE}), C/N0 {c:.2f} (error {e_cn0:.2f} dB, "
                      f"{sr.E2E_TOL_CN0})")
                assert e_ph <= sr.E2E_TOL_PHASE and e_cn0 <= sr.E2E_TOL_CN0, (prn, ph, c)
        finally:
            res.capture_a.free()
            res.capture_b.free()


def test_the_authentic_pair_comes_back_byte_for_byte(dev, search):
    raw_a, raw_b = cr.e2e_pair("authentic")
    res = mitigate.clean_spoofed(dev, raw_a, raw_b, k=2, search=search, tol=cr.E2E_TOL)
    try:
        assert res.report.spoofed is False and res.removals_a == [] == res.removals_b
        assert res.capture_a.download().tobytes() == raw_a.tobytes() and res.capture_b.download().tobytes() == raw_b.tobytes()
        assert not res.records_a["removed"].any() and not res.records_b["removed"].any()
    finally:
        res.capture_a.free()
        res.capture_b.free()
