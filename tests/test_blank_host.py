"""CPU side of the pulse blanker (gj_blank_dev, gj_blank_blocks, Device.blank, mitigate.clean_pulsed): the interface, the
int64 restatement the GPU tests compare with (tests/blank_restatement.py) checked against a per-sample double loop and
against the definition's own consequences, the Python layers on a host double of the library, and the end-to-end figures
the GPU test's tolerance comes from.  No GPU call is made.

The tests under "the restatement" and "end to end" exercise tests/blank_restatement.py alone: they check the yardstick
and do not cover the library.  The interface test and the tests on the host double run the package's code, and
tests/blank/test_round6_gpu.py runs the kernel."""
import ctypes as C
import math

import numpy as np
import pytest

import blank_restatement as br
import excise_restatement as er
import gpsjam
import host_lib
from gpsjam import _ffi, mitigate


# ------------------------------------------------------------------------------------------------ interface
def test_symbols_bindings_and_python_interface():
    lib = _ffi.load()
    assert len(_ffi.SIGNATURES["gj_blank_dev"][1]) == 10 and len(_ffi.SIGNATURES["gj_blank_blocks"][1]) == 1
    for name in ("gj_blank_dev", "gj_blank_blocks"):
        assert callable(getattr(lib, name))
    assert _ffi.GJ_VERSION == 150 and _ffi.GJ_BLANK_BLOCK == gpsjam.BLANK_BLOCK == br.BLOCK == 4096
    assert C.sizeof(_ffi.BlankBlock) == gpsjam.BLANK_DTYPE.itemsize == br.RECORD.itemsize == 24
    assert gpsjam.BLANK_DTYPE == br.RECORD
    assert [(n, gpsjam.BLANK_DTYPE.fields[n][1]) for n in gpsjam.BLANK_DTYPE.names] == [(f[0], getattr(_ffi.BlankBlock, f[0]).offset)
                                                                                           for f in _ffi.BlankBlock._fields_]
    for name in ("blank", "blank_dev"):
        assert callable(getattr(gpsjam.Device, name))
    for name in ("BLANK_DTYPE", "BLANK_BLOCK", "blank_blocks"):
        assert name in gpsjam.__all__
    assert mitigate.CleanedPulsed._fields == ("capture", "records", "threshold", "floor_from", "removed_share", "blanked_share")
    # ceil(n / 4096), host arithmetic: no context, no GPU
    for n in (0, 1, 4095, 4096, 4097, 3 * 4096 + 1234, 2 ** 31 + 1, 2 ** 40 + 4095):
        assert gpsjam.blank_blocks(n) == -(-n // 4096), n
    assert gpsjam.blank_blocks(-1) == 0


# ------------------------------------------------------------------------------------------------ the restatement
def brute(raw, threshold, W, G, first, n, offset):
    """The definition sample by sample: two nested loops, no cumulative sum."""
    o2 = int(2 * offset)
    src = np.asarray(raw, np.uint8)[2 * first:2 * (first + n)].astype(int)
    e = [(2 * src[2 * t] - o2) ** 2 + (2 * src[2 * t + 1] - o2) ** 2 for t in range(n)]
    T = math.floor(4.0 * W * float(np.float32(threshold)))
    D = [sum(e[u] for u in range(t - W // 2, t - W // 2 + W) if 0 <= u < n) > T for t in range(n)]
    B = [any(D[u] for u in range(t - G, t + G + 1) if 0 <= u < n) for t in range(n)]
    out = src.copy()
    for t in range(n):
        if B[t]:
            if o2 % 2 == 0:
                out[2 * t] = out[2 * t + 1] = o2 // 2
            else:
                out[2 * t], out[2 * t + 1] = (o2 - 1) // 2 + ((first + t) & 1), (o2 - 1) // 2 + ((first + t + 1) & 1)
    return out.astype(np.uint8), np.array(B), np.array(e)


@pytest.mark.parametrize("W", [1, 2, 5, 16])
@pytest.mark.parametrize("G", [0, 1, 3])
def test_restatement_equals_the_double_loop(W, G):
    rng = np.random.default_rng(100 * W + G)
    for n, first in ((1, 0), (3, 1), (W - 1 or 1, 2), (W, 0), (61, 3), (200, 1)):     # ranges shorter than W among them
        z = rng.normal(0, 6.0, n + first + 4) + 1j * rng.normal(0, 6.0, n + first + 4)
        z[rng.random(z.size) < 0.06] += 90.0
        raw = ((np.clip(np.round(np.stack([z.real, z.imag], 1)), -128, 127) + 128).astype(np.uint8)).reshape(-1)
        for offset in (127.5, 128.0):
            for thr in (4 * 72.0, 20.0, 2000.0):
                want_out, want_b, want_e = brute(raw, thr, W, G, first, n, offset)
                got = br.blank(raw, thr, W, G, first, n, offset)
                assert np.array_equal(got.out, want_out) and np.array_equal(got.blanked, want_b), (W, G, n, first, offset, thr)
                assert np.array_equal(got.e, want_e) and got.records.size == 1
                assert got.records[0]["total"] == want_e.sum() and got.records[0]["removed"] == want_e[want_b].sum()
                assert got.records[0]["n_blanked"] == want_b.sum()
                assert got.records[0]["n_rising"] == sum(1 for t in range(n) if want_b[t] and (t == 0 or not want_b[t - 1]))


def test_record_blocks_and_rising_edges_across_a_block_seam():
    n = 2 * br.BLOCK + 10
    raw = np.full(2 * n, 128, np.uint8)
    for at, length in ((0, 3), (br.BLOCK - 2, 4), (2 * br.BLOCK, 1), (2 * br.BLOCK + 9, 1)):     # the second crosses the seam: no new edge
        raw[2 * at:2 * (at + length)] = 228
    got = br.blank(raw, 100.0, 1, 0, offset=128.0)
    assert got.records["n_blanked"].tolist() == [5, 2, 2] and got.records["n_rising"].tolist() == [2, 0, 2]
    assert got.records["total"].tolist() == got.records["removed"].tolist() == [5 * 80000, 2 * 80000, 2 * 80000]
    assert np.all(got.out == 128)


def test_infinity_and_huge_thresholds_never_blank():
    raw = br.parity_capture()
    for thr in (np.inf, 3.0e38, 2.0 ** 63 / 4):      # T >= 2^63 at every window
        for W, G in ((1, 0), (16, 8), (1024, 1024)):
            got = br.blank(raw, thr, W, G, br.PARITY_FIRST, br.PARITY_SAMPLES)
            assert got.T is None and not got.blanked.any() and not got.records["removed"].any() and not got.records["n_rising"].any()
            assert got.out.tobytes() == raw[2 * br.PARITY_FIRST:2 * (br.PARITY_FIRST + br.PARITY_SAMPLES)].tobytes()
    assert br.threshold_sum(2.0 ** 52, 1) == 2 ** 54, "below 2^63 the floor is taken"
    with pytest.raises(AssertionError):
        br.threshold_sum(np.nan, 16)
    with pytest.raises(AssertionError):
        br.threshold_sum(-1.0, 16)


def test_a_blanked_stretch_keeps_the_mean():
    n = 4096
    raw = np.random.default_rng(5).integers(0, 256, 2 * n + 8).astype(np.uint8)
    for first in (0, 1):
        got = br.blank(raw, 0.0, 1, 0, first, n, offset=127.5)                   # T = 0: every sample with e > 0, that is all of them
        assert got.blanked.all() and set(np.unique(got.out).tolist()) == {127, 128}
        i, q = got.out[0::2].astype(int), got.out[1::2].astype(int)
        assert np.all(i + q == 255) and np.all(i[:-1] + i[1:] == 255), "I and Q differ, and both alternate"
        assert i[0] == 127 + (first & 1), "the phase of the alternation is the absolute sample index's"
        for a, m in ((0, 2), (7, 2), (3, 64), (100, 1000)):
            assert i[a:a + m].mean() == q[a:a + m].mean() == 127.5, (first, a, m)
        even = br.blank(raw, 0.0, 1, 0, first, n, offset=128.0)
        assert np.all(even.out[even.blanked.repeat(2)] == 128) and np.array_equal(even.out[~even.blanked.repeat(2)], raw[2 * first:2 * (first + n)][~even.blanked.repeat(2)])
        assert even.blanked.sum() >= n - 8, "only a sample of exactly (128, 128) has e = 0"


def test_sub_range_reproduces_the_interior():
    raw = br.parity_capture()
    for W, G in ((1, 0), (16, 8), (63, 1), (1024, 1024)):
        whole = br.blank(raw, br.PARITY_THRESHOLD, W, G, br.PARITY_FIRST, br.PARITY_SAMPLES)
        k, m = 1001, 2 * br.BLOCK + 777
        part = br.blank(raw, br.PARITY_THRESHOLD, W, G, br.PARITY_FIRST + k, m)
        lo, hi = W // 2 + G, m - (W + G)
        assert part.out[2 * lo:2 * hi].tobytes() == whole.out[2 * (k + lo):2 * (k + hi)].tobytes(), (W, G)


def test_parity_input_exercises_what_it_claims():
    raw, f, n = br.parity_capture(), br.PARITY_FIRST, br.PARITY_SAMPLES
    assert f % 2 == 1 and n == 3 * 4096 + 1234 and raw.size == 2 * (f + n + br.PARITY_TAIL)
    body = raw[2 * f:2 * (f + n)]
    assert (body == 0).any() and (body == 255).any()
    ref = br.parity_reference(1, 0)
    assert ref.e.max() == 2 * 255 ** 2 and ref.blanked[0] and ref.blanked[n - 1] and ref.blanked[1000]
    assert ref.blanked[br.BLOCK - 1] and ref.blanked[br.BLOCK] and ref.blanked[2 * br.BLOCK - 1] and ref.blanked[2 * br.BLOCK]
    # at W = 1, two one-sample pulses 2 G apart are joined by the dilation: everything from one to the other is blanked;
    # 2 G + 2 apart their dilations leave the sample half way between them to the noise
    for G, joined, apart in ((1, 1500, 1600), (8, 2000, 2100), (1024, 4500, 9000)):
        ref = br.parity_reference(1, G)
        d = ref.S > ref.T
        assert d[joined] and d[joined + 2 * G] and d[apart] and d[apart + 2 * G + 2]
        assert ref.blanked[joined:joined + 2 * G + 1].all()
        assert ref.blanked[apart + G + 1] == d[apart + 1:apart + 2 * G + 2].any()
    for W in br.PARITY_WINDOWS:                       # every combination blanks something and leaves something
        for G in br.PARITY_GUARDS:
            for offset, _ in br.CONVENTIONS:
                ref = br.parity_reference(W, G, offset)
                assert 0 < ref.blanked.sum() < n or (W, G) == (1024, 1024) or G == 1024, (W, G, offset)
                assert ref.records["n_blanked"].sum() == ref.blanked.sum() and ref.records["total"].sum() == ref.e.sum()
    # the loud bytes outside the range change nothing: the same range cut out as a capture of its own
    alone = br.blank(body, br.PARITY_THRESHOLD, 16, 8, 0, n)
    ref = br.parity_reference(16, 8)
    shift = br.blank(np.concatenate((np.zeros(2, np.uint8), body)), br.PARITY_THRESHOLD, 16, 8, 1, n)
    assert np.array_equal(alone.blanked, ref.blanked) and alone.records.tobytes() == ref.records.tobytes()
    assert np.array_equal(shift.out, ref.out), "an odd first_sample five or one: the same parity, the same bytes"


def test_strictness_input():
    raw = br.strict_capture()
    W, e = br.STRICT_WINDOW, br.STRICT_E
    assert float(np.float32(br.STRICT_THRESHOLD)) == e / 4.0 and br.threshold_sum(br.STRICT_THRESHOLD, W) == W * e
    at = br.blank(raw, br.STRICT_THRESHOLD, W, 0)
    assert np.all(at.S <= W * e) and at.S[W:-W].min() == W * e and not at.blanked.any()
    below = br.blank(raw, np.nextafter(np.float32(br.STRICT_THRESHOLD), np.float32(0)), W, 0)
    assert below.T == W * e - 1
    assert below.blanked[W // 2:br.STRICT_SAMPLES - (W - 1 - W // 2)].all() and not below.blanked[:W // 2].any()
    assert not below.blanked[br.STRICT_SAMPLES - (W - 1 - W // 2):].any()


# ------------------------------------------------------------------------------------------------ the Python layers
def restated_onset(raw, noise_samples, window, factor):
    """K4 (include/gpsjam.h): (start_index, noise_power, threshold)."""
    u = np.asarray(raw, np.uint8).astype(np.float64) - 127.5
    p = u[0::2] ** 2 + u[1::2] ** 2
    if p.size < noise_samples + window:
        return -1, 0.0, 0.0
    noise = p[:noise_samples].mean() or 1e-9
    avg = np.convolve(p, np.ones(window) / window, "valid")
    hit = np.flatnonzero(avg > noise * factor)
    return (int(hit[0]) + window // 2 if hit.size else -1), noise, noise * factor


class HostLib(host_lib.HostLib):
    """The library's entry points that Device.blank and mitigate.clean_pulsed reach, computed by the restatements on host
    memory (tests/host_lib.py)."""

    def __init__(self):
        super().__init__()
        self.offset = 127.5

    def gj_blank_dev(self, ctx, d_iq, nbytes, first, n_samples, window, guard, threshold, d_out, d_blocks):
        self.calls.append(("blank", first, n_samples, window, guard, threshold))
        res = br.blank(self.view(d_iq, nbytes), threshold, window, guard, first, n_samples, self.offset)
        self.view(d_out, 2 * n_samples)[:] = res.out
        if d_blocks:
            self.view(d_blocks, res.records.size, br.RECORD)[:] = res.records
        return 0

    def gj_onset_u8(self, ctx, ptr, nbytes, noise_samples, window, factor, ref, ms):
        self.calls.append(("onset", noise_samples, window, factor))
        start, noise, thr = restated_onset(self.view(ptr, nbytes), noise_samples, window, factor)
        ref._obj.start_index, ref._obj.noise_power, ref._obj.threshold = start, noise, thr
        return 0

    @staticmethod
    def gj_chunk_count(nbytes, chunk_bytes):
        return -(-nbytes // chunk_bytes) if chunk_bytes else 0

    def gj_chunk_power_dev(self, ctx, d_iq, nbytes, chunk_bytes, eps, flags, d_power):
        self.calls.append(("chunk_power", nbytes, chunk_bytes, eps))
        u = self.view(d_iq, nbytes).astype(np.float64) - 127.5
        p = u[0::2] ** 2 + u[1::2] ** 2
        m = chunk_bytes // 2
        self.view(d_power, p.size // m, np.float32)[:] = p[:p.size // m * m].reshape(-1, m).mean(axis=1) + eps
        return 0

    def gj_power_threshold_dev(self, ctx, d_power, n, pct, rise_db, d_stats, d_mask):
        self.calls.append(("power_threshold", n, pct, rise_db))
        base = np.percentile(self.view(d_power, n, np.float32), pct)
        self.view(d_stats, 3, np.float32)[:] = (base, base * 10.0 ** (rise_db / 10.0), 0.0)
        return 0


@pytest.fixture
def host_dev():
    dev = host_lib.host_device(HostLib())
    yield dev
    dev._ctx = None            # a Capture that outlives the test frees nothing


def test_device_blank_on_the_host_double(host_dev):
    raw, lib = br.parity_capture(), host_dev._lib
    want = br.parity_reference(16, 8)
    uploads = gpsjam.Capture.uploads
    cleaned, rec = host_dev.blank(raw, br.PARITY_THRESHOLD, first_sample=br.PARITY_FIRST, n_samples=br.PARITY_SAMPLES)
    assert gpsjam.Capture.uploads == uploads + 1, "host bytes are uploaded once; the cleaned capture is no upload"
    assert isinstance(cleaned, gpsjam.Capture) and cleaned.nbytes == 2 * br.PARITY_SAMPLES and rec.dtype == gpsjam.BLANK_DTYPE
    assert np.array_equal(HostLib.view(cleaned.ptr, cleaned.nbytes), want.out) and rec.tobytes() == want.records.tobytes()
    assert host_dev.kernel_calls == {"blank": 1}
    # the buffers: 2 n bytes out, 24 bytes per block of 4096, the defaults 16 and 8
    assert [c for c in lib.calls if c[0] == "malloc"] == [("malloc", 2 * br.PARITY_SAMPLES), ("malloc", 24 * 4)]
    assert lib.calls[-1][:5] == ("blank", br.PARITY_FIRST, br.PARITY_SAMPLES, 16, 8) and lib.calls[-1][5] == pytest.approx(br.PARITY_THRESHOLD)
    assert list(lib.mem) == [cleaned.ptr], "every buffer but the result is freed"
    # a resident capture: the same bytes, no upload; the range defaults to the rest of the capture
    with gpsjam.Capture(host_dev, raw) as cap:
        uploads = gpsjam.Capture.uploads
        again, rec2 = host_dev.blank(cap, br.PARITY_THRESHOLD, first_sample=br.PARITY_FIRST, n_samples=br.PARITY_SAMPLES)
        assert gpsjam.Capture.uploads == uploads
        assert np.array_equal(HostLib.view(again.ptr, again.nbytes), want.out) and rec2.tobytes() == rec.tobytes()
        rest, rec3 = host_dev.blank(cap, br.PARITY_THRESHOLD, window=63, guard=1, first_sample=7)
        assert rest.nbytes == raw.size - 14 and rec3.size == gpsjam.blank_blocks(raw.size // 2 - 7)
        assert lib.calls[-1][:5] == ("blank", 7, raw.size // 2 - 7, 63, 1)
        for c in (again, rest):
            c.free()
    cleaned.free()
    assert not lib.mem
    freed = gpsjam.Capture(host_dev, raw)
    freed.free()
    with pytest.raises(ValueError, match="freed"):
        host_dev.blank(freed, 1.0)
    assert host_dev.kernel_calls == {"blank": 3}, "a refused call counts nothing"


def test_device_blank_refusals(host_dev):
    raw, lib = br.parity_capture(), host_dev._lib
    host_lib.check_freed(host_dev, raw, lambda cap: host_dev.blank(cap, br.PARITY_THRESHOLD))
    # what the library refuses (a negative threshold, an empty range): the output and the records are allocated, never
    # empty, and freed
    lib.refuse("gj_blank_dev")
    host_lib.check_refused(host_dev, raw, lambda s: host_dev.blank(s, -1.0, first_sample=br.PARITY_FIRST, n_samples=br.PARITY_SAMPLES),
                           gpsjam.GpsJamError, host_lib.REFUSED_TEXT, counted="blank")
    assert host_lib.mallocs(lib) == [2 * br.PARITY_SAMPLES, 24 * 4] * 2
    lib.calls.clear()
    host_lib.check_refused(host_dev, raw, lambda s: host_dev.blank(s, 1.0, first_sample=raw.size // 2), gpsjam.GpsJamError,
                           host_lib.REFUSED_TEXT, counted="blank")
    assert host_lib.mallocs(lib) == [1, 24] * 2 and host_dev.kernel_calls == {"blank": 4}


def shares(res):
    total, removed = int(res.records["total"].sum()), int(res.records["removed"].sum())
    return removed / total, int(res.records["n_blanked"].sum()) / res.capture.nsamples


def test_clean_pulsed_takes_the_floor_from_the_quiet_part(host_dev):
    raw, lib = br.e2e_capture("gated carrier"), host_dev._lib
    start, noise, _ = restated_onset(raw, **er.E2E_ONSET_ARGS)
    assert start >= er.E2E_ONSET_ARGS["noise_samples"] and abs(start - er.E2E_LEAD) < 1000
    res = mitigate.clean_pulsed(host_dev, raw, **br.E2E_ONSET_ARGS)
    try:
        kinds = [c[0] for c in lib.calls if c[0] != "malloc"]
        assert br.E2E_ONSET_ARGS == dict(noise_samples=65536, onset_window=1000, factor=4.0)
        assert lib.calls[0] == ("onset", 65536, 1000, 4.0), "onset_window is K4's window; window stays the blanker's 16"
        assert kinds == ["onset", "blank"] and host_dev.kernel_calls == {"onset": 1, "blank": 1}
        assert isinstance(res, mitigate.CleanedPulsed) and res.floor_from == "quiet part"
        thr = float(np.float32(float(np.float32(noise)) * 10.0 ** 0.6))
        assert res.threshold == thr and lib.calls[-1] == ("blank", 0, raw.size // 2, 16, 8, thr)
        want = br.blank(raw, thr, 16, 8)
        assert np.array_equal(HostLib.view(res.capture.ptr, res.capture.nbytes), want.out) and res.records.tobytes() == want.records.tobytes()
        assert (res.removed_share, res.blanked_share) == shares(res)
        assert 0.25 < res.blanked_share * raw.size / 2 / er.E2E_AFTER < 0.35 and res.removed_share > 0.5
    finally:
        res.capture.free()
    assert not lib.mem, "every buffer but the result is freed"
    # a resident capture gives the same bytes
    with gpsjam.Capture(host_dev, raw) as cap:
        again = mitigate.clean_pulsed(host_dev, cap, **br.E2E_ONSET_ARGS)
        assert np.array_equal(HostLib.view(again.capture.ptr, again.capture.nbytes), want.out) and again[2:] == res[2:]
        again.capture.free()


def test_clean_pulsed_falls_back_to_a_low_percentile_and_takes_a_given_threshold(host_dev):
    raw, lib = br.e2e_capture("gated noise")[2 * er.E2E_LEAD:], host_dev._lib          # jammed from sample 0
    res = mitigate.clean_pulsed(host_dev, raw, rise_db=5.0, floor_pct=25.0, **br.E2E_ONSET_ARGS)
    try:
        calls = [c for c in lib.calls if c[0] != "malloc"]
        assert [c[0] for c in calls] == ["onset", "chunk_power", "power_threshold", "blank"] and res.floor_from == "low percentile"
        assert calls[1] == ("chunk_power", raw.size // 128 * 128, 128, 0.0) and calls[2] == ("power_threshold", raw.size // 128, 25.0, 0.0)
        u = raw.astype(np.float64) - 127.5
        chunks = (u[0::2] ** 2 + u[1::2] ** 2).reshape(-1, 64).mean(axis=1).astype(np.float32)
        floor = float(np.percentile(chunks, 25.0))
        true = 2.0 * er.E2E_SIGMA ** 2 + 3 * 3.0 ** 2                        # noise and three satellites
        print(f"25th percentile of 64-sample means {floor:.2f} LSB^2 against {true:.0f}: {10 * math.log10(floor / true):+.2f} dB")
        assert -0.5 < 10 * math.log10(floor / true) < 0.0, "a few tenths of a dB low"
        assert res.threshold == float(np.float32(floor * 10.0 ** 0.5)) == calls[3][5]
        assert (res.removed_share, res.blanked_share) == shares(res) and 0.25 < res.blanked_share < 0.4
    finally:
        res.capture.free()
    lib.calls.clear()
    given = mitigate.clean_pulsed(host_dev, raw, window=32, guard=4, threshold=1234.5)
    assert [c for c in lib.calls if c[0] != "malloc"] == [("blank", 0, raw.size // 2, 32, 4, 1234.5)]
    assert given.floor_from == "given" and given.threshold == 1234.5
    given.capture.free()
    # a capture too short for K4 has no onset: low percentile again, also when it ends on a ragged chunk
    lib.calls.clear()
    short = mitigate.clean_pulsed(host_dev, raw[:2 * 5000 + 6])
    assert short.floor_from == "low percentile" and ("chunk_power", 9984, 128, 0.0) in lib.calls
    short.capture.free()
    assert not lib.mem


# ------------------------------------------------------------------------------------------------ end to end
def test_end_to_end_on_the_cpu_gives_the_gpu_tests_tolerance():
    """The restated chain on br.e2e_capture(): K4's floor from the quiet part, the blanker at clean_pulsed's defaults,
    C/N0 by the oracle's acquisition.  Re-measures E2E_CPU_RESIDUAL_DB, which E2E_CN0_TOL_DB is twice of."""
    from oracle import gpsjam_oracle as orc
    free_raw = br.e2e_capture(None)
    lead, n = er.E2E_LEAD, free_raw.size // 2
    free = [orc.acq_search(free_raw, lead, prn)[0] for prn, *_ in er.E2E_SATS]
    assert all(r["acquired"] for r in free)
    _, noise, _ = restated_onset(free_raw, **er.E2E_ONSET_ARGS)
    thr = float(np.float32(noise)) * 10.0 ** 0.6
    worst = 0.0
    for kind in br.E2E_KINDS:
        raw = br.e2e_capture(kind)
        assert raw[:2 * lead].tobytes() == free_raw[:2 * lead].tobytes()
        before = [orc.acq_search(raw, lead, prn)[0] for prn, *_ in er.E2E_SATS]
        res = br.blank(raw, thr, 16, 8)
        share = br.e2e_blanked_share(res.records, n)
        after = [orc.acq_search(res.out, lead, prn)[0] for prn, *_ in er.E2E_SATS]
        assert not res.blanked[:lead - 24].any(), "no quiet sample is blanked by mistake"
        assert res.out[:2 * (lead - 24)].tobytes() == raw[:2 * (lead - 24)].tobytes()
        assert abs(share - br.E2E_DUTY) < 0.02
        for (prn, *_), b, a, f in zip(er.E2E_SATS, before, after, free):
            resid = br.e2e_residual_db(a["cn0"], f["cn0"], share)
            worst = max(worst, abs(resid))
            print(f"{kind} PRN {prn}: C/N0 {f['cn0']:.2f} jammer-free, {b['cn0']:.2f} jammed, {a['cn0']:.2f} blanked; share {share:.4f} "
                  f"predicts {10 * math.log10(1 - share):.2f} dB, residual {resid:+.3f} dB")
            assert f["cn0"] - b["cn0"] >= br.E2E_MIN_LOSS_DB
            assert a["acquired"] and a["codei"] == f["codei"] and abs(a["freqi"] - f["freqi"]) <= 1
    print(f"worst residual {worst:.3f} dB (recorded {br.E2E_CPU_RESIDUAL_MEASURED}), tolerance {br.E2E_CN0_TOL_DB} dB")
    assert worst <= br.E2E_CPU_RESIDUAL_DB and abs(worst - br.E2E_CPU_RESIDUAL_MEASURED) < 0.005
    assert br.E2E_CN0_TOL_DB == 2.0 * br.E2E_CPU_RESIDUAL_DB
