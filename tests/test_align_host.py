"""CPU side of the pair alignment (gj_align_dev, gj_align_blocks, Device.align, gpsjam.align): the interface, the integer
restatement the GPU tests compare with (tests/align_restatement.py) checked against a per-sample loop of Python ints and
against the definition's own consequences, the interpolator's quality against an analytic tone, and estimate + to +
coherence.scan end to end on a host double of the library, which sets the figures of the GPU test.  No GPU call is made.

The tests under "the restatement" exercise tests/align_restatement.py alone: they check the yardstick.  The estimator is
not restated anywhere: gpsjam.align itself runs here, on restated integers."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import align_restatement as ar
import caf_restatement as caf
import csd_restatement as cs
import fine_restatement as fr
import gpsjam
import host_lib
from gpsjam import _ffi, align, coherence

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ interface
def test_symbols_bindings_and_python_interface():
    lib = _ffi.load()
    assert len(_ffi.SIGNATURES["gj_align_dev"][1]) == 9 and len(_ffi.SIGNATURES["gj_align_blocks"][1]) == 1
    for name in ("gj_align_dev", "gj_align_blocks"):
        assert callable(getattr(lib, name))
    assert _ffi.GJ_VERSION == 150
    assert (_ffi.GJ_ALIGN_PHASES, _ffi.GJ_ALIGN_TAPS, _ffi.GJ_ALIGN_ROT_LEN, _ffi.GJ_ALIGN_BLOCK) == (ar.PHASES, ar.TAPS, ar.ROT_LEN, ar.BLOCK) == (256, 16, 1024, 4096)
    assert (_ffi.GJ_ALIGN_MAX_DRIFT, _ffi.GJ_ALIGN_MAX_SAMPLES) == (ar.MAX_DRIFT, ar.MAX_SAMPLES) == (2 ** 24, 2 ** 28)
    assert (gpsjam.ALIGN_BLOCK, gpsjam.ALIGN_PHASES, gpsjam.ALIGN_TAPS, gpsjam.ALIGN_ROT_LEN) == (4096, 256, 16, 1024)
    assert C.sizeof(_ffi.AlignParams) == 32 and C.sizeof(_ffi.AlignBlock) == 16 == gpsjam.ALIGN_DTYPE.itemsize == ar.DTYPE.itemsize
    assert [f[0] for f in _ffi.AlignParams._fields_] == ["pos0", "pos_step", "rot_phase", "rot_step", "reserved"]
    assert [f[0] for f in _ffi.AlignBlock._fields_] == list(gpsjam.ALIGN_DTYPE.names) == list(ar.DTYPE.names) == ["power_out", "n_clipped", "n_edge"]
    for name in ("align", "align_dev"):
        assert callable(getattr(gpsjam.Device, name))
    for name in ("ALIGN_BLOCK", "ALIGN_DTYPE", "align_blocks", "AlignParams"):
        assert name in gpsjam.__all__
    for n in (0, 1, 4095, 4096, 4097, 2 ** 40 + 4095):
        assert gpsjam.align_blocks(n) == -(-n // 4096) == ar.blocks(n), n
    assert gpsjam.align_blocks(-1) == 0
    assert align.Estimate._fields[:3] == ("lag", "drift", "offset_hz")


def test_constants_and_layouts_match_the_header():
    text = open(os.path.join(REPO, "include", "gpsjam.h")).read()
    for name, value in (("PHASES", "256"), ("TAPS", "16"), ("ROT_LEN", "1024"), ("BLOCK", "4096"), ("MAX_DRIFT", r"\(1 << 24\)"),
                        ("MAX_SAMPLES", r"\(1 << 28\)")):
        assert re.search(rf"#define GJ_ALIGN_{name} {value}\s", text), name
    assert re.search(r"typedef struct gj_align_params \{[^}]*int64_t pos0;[^}]*uint64_t pos_step;[^}]*uint32_t rot_phase;[^}]*uint32_t rot_step;"
                     r"[^}]*uint64_t reserved;[^}]*\} gj_align_params;", text)
    assert re.search(r"typedef struct gj_align_block \{[^}]*uint64_t power_out;[^}]*int32_t n_clipped;[^}]*int32_t n_edge;[^}]*\} gj_align_block;", text)
    assert re.search(r"#define GJ_VERSION 150\b", text)


def test_the_python_tables_and_parameters():
    t, r = align.taps(), align.rot_table()
    assert t.dtype == np.int16 and t.shape == (256, 16) and r.dtype == np.int16 and r.shape == (1024,)
    assert np.all(t.astype(np.int64).sum(axis=1) == 16384), "every row has unit gain exactly"
    assert t[0].tolist() == [0] * 7 + [16384] + [0] * 8, "row 0 is the delta"
    assert np.array_equal(t[128], t[128][::-1]), "the half-sample row is symmetric"
    assert r[0] == 16384 and r[256] == 0 and r[512] == -16384 and r[768] == 0
    assert np.array_equal(r[1:], r[:0:-1]), "cos is even"
    p = align.params()
    assert (p.pos0, p.pos_step, p.rot_phase, p.rot_step, p.reserved) == (0, 2 ** 32, 0, 0, 0)
    p = align.params(lag=3.25, drift=2.0 ** -20, offset_hz=-500.0, fs=2.048e6)
    assert p.pos0 == 13 * 2 ** 30 and p.pos_step == 2 ** 32 + 2 ** 12
    assert p.rot_step == round(500.0 / 2.048e6 * (1 + 2.0 ** -20) * 2 ** 32) and p.rot_phase == round(500.0 / 2.048e6 * 3.25 * 2 ** 32)
    assert align.params(lag=-1.5).pos0 == -3 * 2 ** 31 and align.params(offset_hz=1000.0).rot_step == 2 ** 32 - 2 ** 21


# ------------------------------------------------------------------------------------------------ the restatement
def brute(raw, pos0, pos_step, rot_phase, rot_step, taps, rot, n_out):
    """The definition sample by sample with Python ints: (bytes, [(power_out, n_clipped, n_edge)])."""
    b, t, r = np.asarray(raw).tolist(), np.asarray(taps).tolist(), np.asarray(rot).tolist()
    n_src = len(b) // 2
    out, rec = [], [[0, 0, 0] for _ in range(-(-n_out // 4096))]
    for n in range(n_out):
        pos = pos0 + n * pos_step + 2 ** 23
        k, p = pos // 2 ** 32, (pos % 2 ** 32) >> 24
        yi = yq = 0
        edge = False
        for j in range(16):
            m = k - 7 + j
            if 0 <= m < n_src:
                yi += t[p][j] * (2 * b[2 * m] - 255)
                yq += t[p][j] * (2 * b[2 * m + 1] - 255)
            else:
                edge = True
        assert abs(yi) < 2 ** 31 and abs(yq) < 2 ** 31
        theta = (rot_phase + n * rot_step) % 2 ** 32
        i = ((theta + 2 ** 21) >> 22) & 1023
        c, s = r[i], r[(i - 256) & 1023]
        for z in (yi * c - yq * s, yi * s + yq * c):
            want = z // 2 ** 29 + 128
            got = min(max(want, 0), 255)
            out.append(got)
            rec[n // 4096][0] += (2 * got - 255) ** 2
            rec[n // 4096][1] += got != want
        rec[n // 4096][2] += edge
    return out, [tuple(v) for v in rec]


def check(raw, case, tables, n_out):
    got, rec = ar.align(raw, *case, *tables, n_out)
    want, wrec = brute(raw, *case, *tables, n_out)
    assert got.dtype == np.uint8 and got.tolist() == want, (case, n_out)
    assert [tuple(int(v) for v in row) for row in rec.tolist()] == wrec, (case, n_out)
    return got, rec


@pytest.mark.parametrize("kind", ["wide", "mid"])
def test_restatement_equals_the_python_int_loop_at_every_size_and_edge(kind):
    raw, tables, cases = ar.parity_capture(), ar.tables(kind), list(ar.CASES.values())
    for at, n in enumerate(ar.SIZES[:-1]):
        for case in (cases[at % len(cases)], cases[(at + 4) % len(cases)], cases[(at + 8) % len(cases)]):
            check(raw, case, tables, n)
    for case in cases:                                        # every edge where a sample and a block begin and end
        check(raw, case, tables, 17)
        check(raw, case, tables, 4097)
    check(raw, ar.CASES["slowest step"] if kind == "mid" else ar.CASES["fastest step"], tables, ar.SIZES[-1])


def test_the_cases_are_the_edges_they_claim_to_be():
    c = ar.CASES
    assert c["negative start"][0] < 0 and c["start past the source's end"][0] >> 32 > ar.PARITY_SAMPLES
    assert c["rounding carries into k"][0] & 0xFFFFFFFF == 0xFF800000
    assert c["fraction 2^23 - 1"][0] & 0xFFFFFFFF == 2 ** 23 - 1 and c["fraction 2^23"][0] & 0xFFFFFFFF == 2 ** 23
    assert {v[1] for v in c.values()} >= {2 ** 32 - 2 ** 24, 2 ** 32, 2 ** 32 + 2 ** 24}
    assert {v[2] for v in c.values()} >= {0, 1, 0xFFFFFFFF} and {v[3] for v in c.values()} >= {0, 1, 0xFFFFFFFF}
    assert abs(c["far before the source"][0]) < 2 ** 60 and abs(c["far behind the source"][0]) < 2 ** 60
    raw, tables = ar.parity_capture(), ar.tables("mid")
    # the carry: fraction 0xFF800000 rounds to phase 0 of the NEXT sample; 2^23 - 1 stays in phase 0, 2^23 is phase 1
    one = np.zeros((256, 16), np.int16)
    one[0, 7], one[1, 7] = 16384, -16384
    delta_rot = ar.tables("delta")[1]
    assert ar.align(raw, (2 << 32) | 0xFF800000, ar.ONE, 0, 0, one, delta_rot, 4)[0].tolist() == raw[6:14].tolist()
    assert ar.align(raw, (9 << 32) | 0x007FFFFF, ar.ONE, 0, 0, one, delta_rot, 4)[0].tolist() == raw[18:26].tolist()
    assert ar.align(raw, (9 << 32) | 0x00800000, ar.ONE, 0, 0, one, delta_rot, 4)[0].tolist() == (255 - raw[18:26]).tolist()
    # outside the source every output is the mid level, and every sample is an edge sample
    for name in ("start past the source's end", "far before the source", "far behind the source"):
        got, rec = ar.align(raw, *c[name], *tables, 4097)
        assert np.all(got == 128) and rec["n_edge"].tolist() == [4096, 1] and not rec["n_clipped"].any(), name


@pytest.mark.parametrize("kind", ["zeros", "full"])
def test_saturated_captures_reach_the_bounds_and_the_clamp(kind):
    raw = ar.parity_capture(kind)
    sign = -1 if kind == "zeros" else 1
    # every tap and the whole turn at -32768: |y| is the header's bound, and z = y * (c -+ s)
    worst = ar.tables("worst")
    n = 40
    got, rec = check(raw, (20 << 32, ar.ONE, 0, 0), worst, n)
    y = -sign * 16 * 255 * 32768
    assert abs(y) == 133693440 < 2 ** 31
    want_q = 0 if 2 * y * -32768 < 0 else 255                          # zI = y c - y s = 0, zQ = 2 y c
    assert np.all(got[0::2] == 128) and np.all(got[1::2] == want_q) and int(rec["n_clipped"][0]) == n and int(rec["n_edge"][0]) == 0
    for tk in ("wide", "mid"):
        got, rec = check(raw, ar.CASES["negative start"], ar.tables(tk), 300)
        assert int(rec["n_edge"][0]) == 13, "5.3 samples early: outputs 0 .. 12 miss a tap"
    got, rec = ar.align(raw, 0, ar.ONE, 0, 0, *ar.tables("wide"), 4096 + 9)
    assert int(rec["n_clipped"].sum()) > 4096 and {0, 255} & set(np.unique(got).tolist())
    assert rec["power_out"].tolist() == [int(((2 * got[:8192].astype(np.int64) - 255) ** 2).sum()), int(((2 * got[8192:].astype(np.int64) - 255) ** 2).sum())]


# ------------------------------------------------------------------------------------------------ properties
def test_identity_byte_for_byte():
    for tables in ((align.taps(), align.rot_table()), ar.tables("delta")):
        for kind in ("random", "zeros", "full"):
            raw = ar.parity_capture(kind)
            got, rec = ar.align(raw, 0, ar.ONE, 0, 0, *tables, ar.PARITY_SAMPLES)
            assert got.tobytes() == raw.tobytes() and not rec["n_clipped"].any()
            assert rec["n_edge"].tolist() == [7, 0, 0, 8], "the first 7 and the last 8 samples miss a tap (of weight 0)"


def test_a_whole_sample_start_is_a_shifted_copy_with_mid_level_beyond_the_source():
    raw, (t, r) = ar.parity_capture(), (align.taps(), align.rot_table())
    n = ar.PARITY_SAMPLES
    for shift in (1, 37, -1, -4100, n - 3, n, -n):
        got, _ = ar.align(raw, shift << 32, ar.ONE, 0, 0, t, r, n)
        want = np.full(2 * n, 128, np.uint8)
        lo, hi = max(0, -shift), min(n, n - shift)             # outputs whose source sample exists
        if hi > lo:
            want[2 * lo:2 * hi] = raw[2 * (lo + shift):2 * (hi + shift)]
        assert got.tobytes() == want.tobytes(), shift
    # a quarter turn is exact: (I, Q) -> (-Q, I), which in bytes is (255 - Q, I)
    got, _ = ar.align(raw, 0, ar.ONE, 1 << 30, 0, t, r, n)
    assert np.array_equal(got[0::2], 255 - raw[1::2]) and np.array_equal(got[1::2], raw[0::2])


def test_a_sub_range_call_writes_the_larger_calls_bytes():
    raw = ar.parity_capture()
    for kind, case in (("mid", ar.CASES["fastest step"]), ("mid", ar.CASES["rounding carries into k"]), ("wide", ar.CASES["slowest step"])):
        tables = ar.tables(kind)
        pos0, step, ph, st = case
        n = 2 * 4096 + 77
        whole, _ = ar.align(raw, pos0, step, ph, st, *tables, n)
        for n1, m in ((1, 50), (4095, 3), (4096, n - 4096), (5000, 1)):
            part, _ = ar.align(raw, pos0 + n1 * step, step, (ph + n1 * st) & 0xFFFFFFFF, st, *tables, m)
            assert part.tobytes() == whole[2 * n1:2 * (n1 + m)].tobytes(), (kind, n1, m)


# ------------------------------------------------------------------------------------------------ quality
QUALITY_AMP = 100.0
QUALITY_FREQS = np.linspace(-0.4, 0.4, 33)          # cycles per sample
QUALITY_LAG, QUALITY_DRIFT, QUALITY_OFFSET_HZ = 2.371, 1.3e-4, 7777.0
QUALITY_RMS = 0.5076                                 # LSB per component, measured (profiles/NOTES_align.md)


def tone_error(beta, lag=QUALITY_LAG):
    """rms error, LSB per component, of a 100-LSB complex tone brought through a fractional delay, a drift and a rotation
    by the restatement with the library's own tables, against the analytic tone; over QUALITY_FREQS, 4096 samples each."""
    t, r = align.taps(beta), align.rot_table()
    p = align.params(lag, QUALITY_DRIFT, QUALITY_OFFSET_HZ, ar.FS)
    n_src, n_out = 4096 + 64, 4096
    m = np.arange(n_src, dtype=np.float64)
    src_t = (np.arange(n_out) + 16) * (p.pos_step / 2.0 ** 32) + p.pos0 / 2.0 ** 32          # source time of every output
    turn = ((p.rot_phase + (np.arange(n_out) + 16) * p.rot_step) % 2 ** 32) / 2.0 ** 32
    sq = []
    for f in QUALITY_FREQS:
        raw = ar._bytes(QUALITY_AMP * np.exp(2j * np.pi * f * m))
        got, rec = ar.align(raw, p.pos0 + 16 * p.pos_step, p.pos_step, (p.rot_phase + 16 * p.rot_step) & 0xFFFFFFFF, p.rot_step, t, r, n_out)
        assert not rec["n_edge"].any() and not rec["n_clipped"].any()
        z = (got[0::2].astype(np.float64) - 127.5) + 1j * (got[1::2].astype(np.float64) - 127.5)
        want = QUALITY_AMP * np.exp(2j * np.pi * (f * src_t + turn))
        sq.append(np.mean(np.abs(z - want) ** 2) / 2.0)
    return float(np.sqrt(np.mean(sq)))


def test_a_tone_comes_through_within_half_an_lsb():
    """The yardstick is the analytic tone.  The floor is two roundings to bytes (1/12 LSB^2 each), the 1/256-sample grid
    of the rows (2 pi f / (512 sqrt 3) radians rms: 0.28 LSB at 0.4 fs on 100 LSB) and the turn's 1024 entries (0.18
    LSB): 0.47 LSB over this sweep.  The figure asserted is the one measured at BETA plus 10 %, which covers other phases
    of the sweep; the sweep over beta is printed (profiles/NOTES_align.md keeps it)."""
    sweep = {beta: tone_error(beta) for beta in (4.0, 4.5, 4.75, 5.0, 5.25, 5.5, 6.0, 7.0)}
    print("rms error of a 100-LSB tone over |f| <= 0.4 fs, LSB per component, by beta:", {k: round(v, 4) for k, v in sweep.items()})
    others = [tone_error(align.BETA, lag) for lag in (0.5, -3.127, 11.9)]
    print("at BETA, other lags:", [round(v, 4) for v in others])
    assert sweep[align.BETA] <= min(sweep.values()) * 1.02, "BETA is the sweep's best, within 2 %"
    assert max([sweep[align.BETA]] + others) <= QUALITY_RMS * 1.1


# ------------------------------------------------------------------------------------------------ the Python layers
class HostLib(host_lib.HostLib):
    """The library's entry points that Device.align, align.estimate, align.to and coherence.scan reach, computed by the
    restatements on host memory (tests/host_lib.py)."""

    log_malloc = False

    def gj_align_dev(self, ctx, d_iq, nbytes, params, d_taps, d_rot, n_out, d_out, d_blocks):
        self.calls.append(("align", params.pos0, params.pos_step, params.rot_phase, params.rot_step, n_out, bool(d_blocks)))
        if not 1 <= n_out <= ar.MAX_SAMPLES or abs(params.pos_step - ar.ONE) > ar.MAX_DRIFT:
            self.last_error = b"outside the limits"
            return -5
        out, rec = ar.align(self.view(d_iq, nbytes), params.pos0, params.pos_step, params.rot_phase, params.rot_step,
                            self.view(d_taps, 256 * 16, np.int16), self.view(d_rot, 1024, np.int16), n_out)
        self.view(d_out, 2 * n_out)[:] = out
        if d_blocks:
            self.view(d_blocks, rec.size, ar.DTYPE)[:] = rec
        return 0

    def gj_xcorr_caf_u8(self, ctx, ptrs, n_ant, n, pairs, n_pairs, bin_first, n_bins, out, ridge_lags, ridge_peaks, ms):
        self.calls.append(("caf", n_ant, n, n_pairs, bin_first, n_bins))
        for p in range(n_pairs):
            i, j = pairs[2 * p], pairs[2 * p + 1]
            s = caf.search(self.view(ptrs[j], 2 * n), self.view(ptrs[i], 2 * n), bin_first, n_bins)
            out[p].lag, out[p].bin, out[p].peak, out[p].margin_lag, out[p].margin_bin = s.lag, s.bin, s.peak, s.margin_lag, s.margin_bin
        return 0

    def gj_xcorr_fine_dev(self, ctx, d_a, nbytes_a, first_a, d_b, nbytes_b, first_b, n, lag_center, half_width, d_total, d_blocks):
        f = fr.fine(self.view(d_a, nbytes_a), self.view(d_b, nbytes_b), lag_center, half_width, first_a, first_b, n)
        self.view(d_total, f.total.size, np.int64)[:] = f.total.reshape(-1)
        if d_blocks:
            self.view(d_blocks, f.blocks.size, np.int32)[:] = f.blocks.reshape(-1)
        return 0

    def gj_csd_dev(self, ctx, d_a, nbytes_a, first_a, d_b, nbytes_b, first_b, nfft, hop, frames_per_row, n_rows, d_saa, d_sbb, d_sab, d_msc):
        saa, sbb, sab, msc = cs.csd(self.view(d_a, nbytes_a), self.view(d_b, nbytes_b), nfft, hop, frames_per_row, first_a, first_b, n_rows)
        self.view(d_saa, n_rows * nfft, np.float32)[:] = saa.reshape(-1)
        self.view(d_sbb, n_rows * nfft, np.float32)[:] = sbb.reshape(-1)
        self.view(d_sab, n_rows * nfft, np.complex64)[:] = sab.reshape(-1)
        if d_msc:
            self.view(d_msc, n_rows * nfft, np.float32)[:] = msc.reshape(-1)
        return 0

    def gj_timer_start(self, ctx):
        return 0

    def gj_timer_stop(self, ctx, ref):
        ref._obj.value = 0.25
        return 0


@pytest.fixture
def host_dev():
    dev = host_lib.host_device(HostLib())
    yield dev
    dev._ctx = None            # a Capture that outlives the test frees nothing


def test_device_align_on_the_host_double(host_dev):
    raw, lib = ar.parity_capture(), host_dev._lib
    tables = ar.tables("mid")
    case = ar.CASES["fastest step"]
    want, wrec = ar.align(raw, *case, *tables, 5000)
    uploads = gpsjam.Capture.uploads
    got, rec = host_dev.align(raw, case, *tables, n_out=5000)
    assert gpsjam.Capture.uploads == uploads + 1 and isinstance(got, gpsjam.Capture) and got.nsamples == 5000
    assert got.download().tobytes() == want.tobytes() and rec.dtype == gpsjam.ALIGN_DTYPE and rec.tobytes() == wrec.tobytes()
    assert lib.calls[-1] == ("align", *case, 5000, True) and host_dev.kernel_calls == {"align": 1}
    got.free()
    assert not lib.mem, "everything is freed"
    # a resident capture, an AlignParams, the default length; phases are taken modulo 2^32
    with gpsjam.Capture(host_dev, raw) as cap:
        uploads = gpsjam.Capture.uploads
        out, rec = host_dev.align(cap, gpsjam.AlignParams(0, ar.ONE, 0, 0, 0), align.taps(), align.rot_table())
        assert gpsjam.Capture.uploads == uploads and out.nsamples == cap.nsamples and out.download().tobytes() == raw.tobytes()
        out.free()
        out, _ = host_dev.align(cap, (0, ar.ONE, 2 ** 32 + 5, -1), *tables, n_out=3)
        assert lib.calls[-1] == ("align", 0, ar.ONE, 5, 0xFFFFFFFF, 3, True)
        out.free()
        held = set(lib.mem)
        with pytest.raises(ValueError):
            host_dev.align(cap, case, tables[0][:5], tables[1])
        with pytest.raises(gpsjam.GpsJamError) as e:
            host_dev.align(cap, (0, ar.ONE + 2 ** 24 + 1, 0, 0), *tables)
        assert e.value.status == -5 and set(lib.mem) == held, "a refusal leaks nothing"
    host_lib.check_freed(host_dev, raw, lambda c: host_dev.align(c, case, *tables))


@pytest.fixture(scope="module")
def e2e():
    """estimate and to on the host double, once for the tests below."""
    dev = host_lib.host_device(HostLib())
    raw_a, raw_b, raw_same = ar.e2e_pair()
    est = align.estimate(dev, raw_a, raw_b, fs=ar.FS, max_offset_hz=1000.0)
    aligned = align.to(dev, raw_a, raw_b, est, fs=ar.FS)
    out = aligned.download()
    aligned.free()
    assert not dev._lib.mem, "everything is freed"
    yield dev, est, out
    dev._ctx = None


def band_median(dev, a, b):
    scan = coherence.scan(dev, a, b, fs=ar.FS, nfft=ar.E2E_NFFT, frames_per_row=ar.E2E_FRAMES)
    assert len(scan.result) == 1
    return float(np.median(scan.result.msc[0, ar.band_bins()])), scan


def test_estimate_recovers_lag_drift_and_offset(e2e):
    dev, est, _ = e2e
    print(f"lag {est.lag:.4f} (truth {ar.E2E_LAG}), drift {est.drift * 1e6:.3f} ppm (truth {ar.E2E_DRIFT * 1e6}), offset {est.offset_hz:.3f} Hz "
          f"(truth {ar.E2E_OFFSET_HZ}); search {est.coarse_offset_hz:.2f} Hz, lags {est.coarse_lags}; slices {np.round(est.slice_lags, 3).tolist()}; "
          f"spread {est.spread:.4f}")
    assert est.ok and len(est.coarse_lags) == 8 and est.slice_times.tolist() == [4096.0 + 8192 * k for k in range(8)]
    assert abs(est.lag - ar.E2E_LAG) <= ar.E2E_TOL_LAG
    assert abs(est.drift - ar.E2E_DRIFT) <= ar.E2E_TOL_DRIFT
    assert abs(est.offset_hz - ar.E2E_OFFSET_HZ) <= ar.E2E_TOL_OFFSET_HZ
    # with the tuned frequency the drift is the offset's: a made-up rf that turns 300 Hz into 40 ppm
    rf = ar.E2E_OFFSET_HZ / ar.E2E_DRIFT
    raw_a, raw_b, _ = ar.e2e_pair()
    tied = align.estimate(dev, raw_a, raw_b, rf_hz=rf, fs=ar.FS, max_offset_hz=1000.0)
    print(f"with rf_hz: lag {tied.lag:.4f}, drift {tied.drift * 1e6:.3f} ppm, offset {tied.offset_hz:.3f} Hz")
    assert tied.drift == tied.offset_hz / rf and abs(tied.offset_hz - ar.E2E_OFFSET_HZ) <= ar.E2E_TOL_OFFSET_HZ
    assert abs(tied.lag - ar.E2E_LAG) <= ar.E2E_TOL_LAG


def test_the_aligned_pair_is_as_coherent_as_a_pair_on_one_clock(e2e):
    """Medians over the jammer's band, not minima: a sum of tones has thin bins."""
    dev, est, out = e2e
    raw_a, raw_b, raw_same = ar.e2e_pair()
    assert out.size == raw_a.size
    thr = coherence.threshold(ar.E2E_FRAMES)
    raw_msc, raw_scan = band_median(dev, raw_a, raw_b)
    got_msc, got_scan = band_median(dev, raw_a, out)
    one_msc, one_scan = band_median(dev, raw_a, raw_same)
    print(f"median MSC in the band: raw pair {raw_msc:.4f} (threshold {thr:.4f}), aligned {got_msc:.4f}, one clock {one_msc:.4f}")
    assert raw_msc < thr and not raw_scan.detection.flagged.any() and raw_scan.bands == []
    assert abs(got_msc - one_msc) <= ar.E2E_TOL_MSC
    flagged = np.flatnonzero(got_scan.detection.flagged)
    assert set(ar.band_bins().tolist()) <= set(flagged.tolist()), "the band is flagged"
    assert flagged.min() >= ar.band_bins()[0] - 3 and flagged.max() <= ar.band_bins()[-1] + 3, "and nothing else"
    assert len(got_scan.bands) == 1 and abs(got_scan.bands[0].delay) < 0.1


def test_command_line(tmp_path, monkeypatch, capsys):
    raw_a, raw_b, _ = ar.e2e_pair()
    pa, pb, po = (str(tmp_path / name) for name in ("a.bin", "b.bin", "out.bin"))
    raw_a[:2 * 16384].tofile(pa)
    raw_b[:2 * 16384].tofile(pb)

    class FileDevice(gpsjam.Device):
        def __init__(self, index=0):
            d = host_lib.host_device(HostLib())
            self.__dict__.update(d.__dict__)

        def capture(self, source, offset=0, max_bytes=0):
            return gpsjam.Capture(self, np.fromfile(source, np.uint8))

        def close(self):
            self._ctx = None

    monkeypatch.setattr(gpsjam, "Device", FileDevice)
    assert align.main([pa, pb, po, "--max-offset-hz", "500"]) == 0
    text = capsys.readouterr().out
    assert "lag +3." in text and "ppm" in text and "16384 samples" in text
    assert os.path.getsize(po) == 2 * 16384
