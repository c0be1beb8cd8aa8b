"""CPU side of fine TDOA (gj_xcorr_fine_dev, gj_fine_blocks, Device.xcorr_fine, gpsjam.tdoa): the interface, the int64
restatement the GPU tests compare with (tests/fine_restatement.py) checked against a per-sample double loop and against
the definition's own consequences, the Python layers on a host double of the library, and the estimator's accuracy on
synthetic pairs, which sets the tolerance of the GPU test.  No GPU call is made.

The tests under "the restatement" exercise tests/fine_restatement.py alone: they check the yardstick.  The estimator is
not restated anywhere: gpsjam.tdoa itself runs here, on restated integers."""
import ctypes as C
import math

import numpy as np
import pytest

import blank_restatement as br
import fine_restatement as fr
import gpsjam
import host_lib
from gpsjam import _ffi, tdoa


# ------------------------------------------------------------------------------------------------ interface
def test_symbols_bindings_and_python_interface():
    lib = _ffi.load()
    assert len(_ffi.SIGNATURES["gj_xcorr_fine_dev"][1]) == 12 and len(_ffi.SIGNATURES["gj_fine_blocks"][1]) == 1
    for name in ("gj_xcorr_fine_dev", "gj_fine_blocks"):
        assert callable(getattr(lib, name))
    assert _ffi.GJ_VERSION == 150 and _ffi.GJ_FINE_BLOCK == gpsjam.FINE_BLOCK == fr.BLOCK == 4096
    assert _ffi.GJ_FINE_MAX_HALF == gpsjam.FINE_MAX_HALF == fr.MAX_HALF == 32
    for name in ("xcorr_fine", "xcorr_fine_dev"):
        assert callable(getattr(gpsjam.Device, name))
    for name in ("fine_blocks", "FINE_BLOCK", "FineCorr"):
        assert name in gpsjam.__all__
    assert gpsjam.FineCorr._fields == ("lags", "c", "blocks", "n_samples")
    assert tdoa.FineLag._fields == ("lag", "coarse", "delta", "phase", "spread", "ok")
    for n in (0, 1, 4095, 4096, 4097, 2 ** 40 + 4095):
        assert gpsjam.fine_blocks(n) == -(-n // 4096), n
    assert gpsjam.fine_blocks(-1) == 0, "as blank_blocks: no range, no records"


# ------------------------------------------------------------------------------------------------ the restatement
def brute(raw_a, raw_b, c, R, first_a, first_b, n, offset):
    """The definition sample by sample with Python ints: {k: (re, im)}."""
    o2 = int(2 * offset)
    a = [2 * int(v) - o2 for v in raw_a[2 * first_a:2 * (first_a + n)]]
    b = [2 * int(v) - o2 for v in raw_b[2 * first_b:2 * (first_b + n)]]
    out = {}
    for k in range(c - R, c + R + 1):
        re = im = 0
        for t in range(n):
            if 0 <= t + k < n:
                re += b[2 * (t + k)] * a[2 * t] + b[2 * (t + k) + 1] * a[2 * t + 1]
                im += b[2 * (t + k) + 1] * a[2 * t] - b[2 * (t + k)] * a[2 * t + 1]
        out[k] = (re, im)
    return out


@pytest.mark.parametrize("offset", [127.5, 128, 0, 255])
def test_restatement_equals_the_double_loop(offset):
    rng = np.random.default_rng(int(2 * offset))
    raw_a, raw_b = (rng.integers(0, 256, 2 * 210).astype(np.uint8) for _ in range(2))
    raw_a[:8], raw_b[:8] = (0, 255, 255, 0, 0, 0, 255, 255), (255, 255, 0, 0, 255, 0, 0, 255)
    for n, first_a, first_b in ((1, 1, 3), (3, 0, 1), (61, 3, 1), (200, 1, 5)):
        for R in (0, 1, 5):
            for c in (0, 1, -1, 7, -7, n + 9):
                got = fr.fine(raw_a, raw_b, c, R, first_a, first_b, n, offset)
                want = brute(raw_a, raw_b, c, R, first_a, first_b, n, offset)
                assert got.lags.tolist() == list(want) and got.blocks.shape == (1, 2 * R + 1, 2)
                assert [tuple(v) for v in got.total.tolist()] == list(want.values()), (n, R, c, offset)
                if c == n + 9:
                    assert not got.total.any(), "no overlap: zeros"


def test_block_records_sum_to_the_totals_and_follow_a():
    a, b = fr.parity_captures()
    ref = fr.parity_reference(1, 16)
    assert ref.blocks.shape == (4, 33, 2) and np.array_equal(ref.blocks.sum(axis=0), ref.total)
    assert np.abs(ref.blocks).max() < 2 ** 31
    # record m is the sum over ITS samples of a alone, sample by sample, across the seam and in the ragged block
    n, o2 = fr.BLOCK + 50, 255
    got = fr.fine(a, b, -1, 1, 1, 3, n)
    ua = [2 * int(v) - o2 for v in a[2:2 * (1 + n)]]
    ub = [2 * int(v) - o2 for v in b[6:2 * (3 + n)]]
    for m, (t0, t1) in enumerate(((0, fr.BLOCK), (fr.BLOCK, n))):
        for j, k in enumerate((-2, -1, 0)):
            ts = [t for t in range(t0, t1) if 0 <= t + k < n]
            re = sum(ub[2 * (t + k)] * ua[2 * t] + ub[2 * (t + k) + 1] * ua[2 * t + 1] for t in ts)
            im = sum(ub[2 * (t + k) + 1] * ua[2 * t] - ub[2 * (t + k)] * ua[2 * t + 1] for t in ts)
            assert got.blocks[m, j].tolist() == [re, im], (m, k)


def test_autocorrelation_is_hermitian_and_its_zero_lag_is_the_blankers_total():
    raw = br.parity_capture()
    for offset in (127.5, 128):
        f = fr.fine(raw, raw, 0, 16, br.PARITY_FIRST, br.PARITY_FIRST, br.PARITY_SAMPLES, offset)
        assert f.total[16, 1] == 0 and not f.blocks[:, 16, 1].any()
        assert np.array_equal(f.total[::-1, 0], f.total[:, 0]) and np.array_equal(f.total[::-1, 1], -f.total[:, 1])
        want = br.blank(raw, np.inf, 16, 8, br.PARITY_FIRST, br.PARITY_SAMPLES, offset).records["total"]
        assert np.array_equal(f.blocks[:, 16, 0].astype(np.uint64), want)


def test_it_is_numpys_correlate_times_four():
    a, b = fr.parity_captures()
    for offset in (127.5, 128):
        for n in (5, 300):
            f = fr.fine(a, b, 2, 4, fr.PARITY_FIRST_A, fr.PARITY_FIRST_B, n, offset)
            x = [(raw[2 * first:2 * (first + n):2].astype(np.float64) - offset) + 1j * (raw[2 * first + 1:2 * (first + n):2].astype(np.float64) - offset)
                 for raw, first in ((a, fr.PARITY_FIRST_A), (b, fr.PARITY_FIRST_B))]
            full = np.correlate(x[1], x[0], "full")                     # every term a multiple of 1/4: exact in float64
            want = [full[k + n - 1] if -n < k < n else 0.0 for k in f.lags.tolist()]
            assert np.array_equal(f.corr().c, np.array(want))


def test_extremes_fill_the_block_record_without_wrapping():
    """The bound is reached with one sign only: under offset 0 every u is >= 0 and under offset 255 every u is <= 0, so
    the real part of saturated inputs is +2 130 739 200 (255 against 255 at offset 0, 0 against 0 at offset 255) and 0
    against 255 at offset 255 gives 0, byte 255 being the sample zero there.  The most negative record that bytes can
    make is the one of 0 against 255 at 127.5: -4096 * 2 * 255^2."""
    n = fr.BLOCK
    for (a, b, offset), want in fr.EXTREME_CASES.items():
        got = fr.fine(np.full(2 * n, a, np.uint8), np.full(2 * n, b, np.uint8), 0, 0, offset=offset)
        assert got.blocks[0, 0].tolist() == [want, 0], (a, b, offset)
    assert fr.BLOCK_BOUND == 2130739200 < 2 ** 31 and fr.BLOCK_BOUND in fr.EXTREME_CASES.values()


def test_parity_input_exercises_what_it_claims():
    a, b = fr.parity_captures()
    n = fr.PARITY_SAMPLES
    assert fr.PARITY_FIRST_A % 2 == 1 and fr.PARITY_FIRST_B % 2 == 1 and fr.PARITY_FIRST_A != fr.PARITY_FIRST_B
    assert n == 3 * 4096 + 1234 and a.size == 2 * (fr.PARITY_FIRST_A + n + fr.PARITY_TAIL) and b.size == 2 * (fr.PARITY_FIRST_B + n + fr.PARITY_TAIL)
    ref = fr.parity_reference(0, 16)
    assert int(np.argmax(np.abs(ref.corr().c))) == 16 + fr.PARITY_DELAY, "b is late by PARITY_DELAY"
    assert not fr.parity_reference(n + 40, 32).total.any(), "no overlap at all"
    last = fr.parity_reference(n - 1, 1)
    assert last.total[1].any() and not last.total[2].any(), "lag n - 1 is the last one with an overlap"
    assert fr.parity_reference(-4099, 16).total.all()
    for raw in (a, b):                                   # the four corners of the byte range occur inside the ranges
        pairs = set(zip(raw[0::2].tolist(), raw[1::2].tolist()))
        assert {(0, 0), (0, 255), (255, 0), (255, 255)} <= pairs


# ------------------------------------------------------------------------------------------------ the Python layers
class HostLib(host_lib.HostLib):
    """The library's entry points that Device.xcorr_fine and tdoa.refine reach, computed by the restatement (and, for K5,
    by numpy) on host memory (tests/host_lib.py)."""

    def gj_xcorr_fine_dev(self, ctx, d_a, nbytes_a, first_a, d_b, nbytes_b, first_b, n, lag_center, half_width, d_total, d_blocks):
        self.calls.append(("fine", first_a, first_b, n, lag_center, half_width, bool(d_blocks)))
        f = fr.fine(self.view(d_a, nbytes_a), self.view(d_b, nbytes_b), lag_center, half_width, first_a, first_b, n)
        self.view(d_total, f.total.size, np.int64)[:] = f.total.reshape(-1)
        if d_blocks:
            self.view(d_blocks, f.blocks.size, np.int32)[:] = f.blocks.reshape(-1)
        return 0

    def gj_xcorr_lags_u8(self, ctx, ptrs, n_ant, n, pairs, n_pairs, lags, peaks, margins, ms):
        self.calls.append(("lags", n_ant, n, n_pairs))
        x = [self.view(ptrs[k], 2 * n).astype(np.float64) - 127.5 for k in range(n_ant)]
        z = [v[0::2] + 1j * v[1::2] for v in x]
        for p in range(n_pairs):
            i, j = pairs[2 * p], pairs[2 * p + 1]
            L = 1 << int(math.ceil(math.log2(2 * n)))
            c = np.fft.ifft(np.fft.fft(z[j], L) * np.conj(np.fft.fft(z[i], L)))
            m = int(np.argmax(np.abs(c)))
            lags[p], peaks[p], margins[p] = (m if m < L // 2 else m - L), float(np.abs(c[m])), 1.0
        return 0


@pytest.fixture
def host_dev():
    dev = host_lib.host_device(HostLib())
    yield dev
    dev._ctx = None            # a Capture that outlives the test frees nothing


def test_device_xcorr_fine_on_the_host_double(host_dev):
    (a, b), lib = fr.parity_captures(), host_dev._lib
    want = fr.parity_reference(1, 16)
    uploads = gpsjam.Capture.uploads
    got = host_dev.xcorr_fine(a, b, lag_center=1, first_a=fr.PARITY_FIRST_A, first_b=fr.PARITY_FIRST_B, n_samples=fr.PARITY_SAMPLES)
    assert gpsjam.Capture.uploads == uploads + 2, "host bytes are uploaded once each"
    assert isinstance(got, gpsjam.FineCorr) and got.blocks is None and got.n_samples == fr.PARITY_SAMPLES
    assert got.lags.dtype == np.int64 and got.lags.tolist() == list(range(-15, 18)) and got.c.dtype == np.complex128
    assert np.array_equal(got.c, want.corr().c) and np.array_equal(4 * got.c.real, want.total[:, 0])
    assert host_lib.mallocs(lib) == [16 * 33] and lib.calls[-1] == ("fine", fr.PARITY_FIRST_A, fr.PARITY_FIRST_B, fr.PARITY_SAMPLES, 1, 16, False)
    assert not lib.mem, "everything is freed"
    assert host_dev.kernel_calls == {"xcorr_fine": 1}
    lib.calls.clear()
    # resident captures: no upload; the block records; the range defaults to what both captures hold
    with gpsjam.Capture(host_dev, a) as ca, gpsjam.Capture(host_dev, b) as cb:
        uploads = gpsjam.Capture.uploads
        got = host_dev.xcorr_fine(ca, cb, lag_center=1, half_width=5, first_a=fr.PARITY_FIRST_A, first_b=fr.PARITY_FIRST_B,
                                  n_samples=fr.PARITY_SAMPLES, want_blocks=True)
        assert gpsjam.Capture.uploads == uploads
        assert host_lib.mallocs(lib) == [16 * 11, 8 * 11 * 4]
        assert got.blocks.shape == (4, 11) and np.array_equal(got.blocks.sum(axis=0), got.c)
        assert np.array_equal(got.c, want.corr().c[11:22]) and np.array_equal(got.blocks, want.corr(True).blocks[:, 11:22])
        rest = host_dev.xcorr_fine(ca, cb, first_a=7, first_b=2)
        assert rest.n_samples == min(a.size // 2 - 7, b.size // 2 - 2) and lib.calls[-1] == ("fine", 7, 2, rest.n_samples, 0, 16, False)
        auto = host_dev.xcorr_fine(ca, ca, half_width=0)
        assert gpsjam.Capture.uploads == uploads and auto.c.shape == (1,) and auto.c[0].imag == 0
        assert set(lib.mem) == {ca.ptr, cb.ptr}, "everything but the inputs is freed"
    assert host_dev.kernel_calls == {"xcorr_fine": 4}
    same = host_dev.xcorr_fine(a, a, half_width=1)
    assert gpsjam.Capture.uploads == uploads + 1 and same.c[1].imag == 0, "one array given twice is uploaded once"
    assert not lib.mem


def test_device_xcorr_fine_refusals(host_dev):
    (a, b), lib = fr.parity_captures(), host_dev._lib
    host_lib.check_freed(host_dev, a, lambda cap: host_dev.xcorr_fine(cap, b))
    held = set(lib.mem)
    host_lib.check_freed(host_dev, a, lambda cap: host_dev.xcorr_fine(b, cap))
    assert set(lib.mem) == held, "the capture uploaded for a in front of the freed b is freed too"
    lib.calls.clear()
    lib.refuse("gj_xcorr_fine_dev")
    host_lib.check_refused(host_dev, a, lambda s: host_dev.xcorr_fine(s, s, half_width=40, want_blocks=True), gpsjam.GpsJamError,
                           host_lib.REFUSED_TEXT, counted="xcorr_fine")
    assert host_lib.mallocs(lib) == [16 * 81, 8 * 81 * gpsjam.fine_blocks(a.size // 2)] * 2


def test_refine_takes_k5s_lag_and_centres_the_window_there(host_dev):
    lib = host_dev._lib
    a, b = fr.e2e_pair(4096, "full", 3.37)
    want = tdoa.fine_lag(fr.fine(a, b, 3, 16).corr())
    uploads = gpsjam.Capture.uploads
    got = tdoa.refine(host_dev, b, a)
    assert gpsjam.Capture.uploads == uploads + 2 and not lib.mem
    assert [c for c in lib.calls if c[0] != "malloc"] == [("lags", 2, 4096, 1), ("fine", 0, 0, 4096, 3, 16, False)]
    assert got == want and got.coarse == 3 and got.ok and abs(got.lag - 3.37) <= fr.E2E_TOL[4096, "full"]
    back = tdoa.refine(host_dev, a, b, half_width=8)
    assert back.coarse == -3 and abs(back.lag + 3.37) <= fr.E2E_TOL[4096, "full"] and lib.calls[-1][4:6] == (-3, 8)
    assert tdoa.refine(host_dev, np.zeros(0, np.uint8), np.zeros(0, np.uint8)) is None, "an empty pair is invalid for K5"
    # series: one estimate per group of block records, each within the short integration's tolerance
    a, b = fr.e2e_pair(50000, "full", 3.37)
    with gpsjam.Capture(host_dev, a) as ca, gpsjam.Capture(host_dev, b) as cb:
        corr = host_dev.xcorr_fine(ca, cb, lag_center=3, want_blocks=True)
    pts = tdoa.series(corr, 4)
    assert len(pts) == 4 and all(p.ok and p.coarse == 3 for p in pts)
    print("series of 4 blocks:", [round(p.lag, 4) for p in pts])
    assert all(abs(p.lag - 3.37) <= 2 * fr.E2E_TOL[4096, "full"] for p in pts), "16 384 samples do no worse than twice 4096's bound"
    with pytest.raises(ValueError):
        tdoa.series(corr._replace(blocks=None), 4)


# ------------------------------------------------------------------------------------------------ the estimator
@pytest.mark.parametrize("band", fr.E2E_BANDS)
@pytest.mark.parametrize("n", fr.E2E_SIZES)
def test_estimator_accuracy_sets_the_tolerance(n, band):
    """Re-measures fr.E2E_CPU_ERROR_MEASURED, which fr.E2E_TOL is twice of."""
    worst, parabola = 0.0, 0.0
    for delay in fr.E2E_DELAYS:
        a, b = fr.e2e_pair(n, band, delay)
        corr = fr.fine(a, b, fr.e2e_centre(delay), fr.E2E_HALF).corr()
        got = tdoa.fine_lag(corr)
        perr = tdoa.parabola_lag(corr) - delay
        print(f"n {n} {band}-band delay {delay:+.2f}: lag {got.lag:+.5f} (error {got.lag - delay:+.5f}), phase {got.phase:.4f}, "
              f"spread {got.spread:.4f}, parabola error {perr:+.4f}")
        assert got.ok and got.coarse == fr.e2e_centre(delay), got
        assert abs(got.lag - delay) <= fr.E2E_TOL[n, band], (delay, got)
        assert abs(got.phase - fr.E2E_PHASE) < 0.02, got
        worst, parabola = max(worst, abs(got.lag - delay)), max(parabola, abs(perr))
    recorded = fr.E2E_CPU_ERROR_MEASURED[n, band]
    print(f"n {n} {band}-band: worst error {worst:.5f} sample (recorded {recorded}), parabola's worst {parabola:.4f}")
    assert abs(worst - recorded) <= 0.1 * recorded, (worst, recorded)
    assert fr.E2E_TOL[n, band] == 2.0 * recorded
    if band == "full":
        assert parabola > 0.2 > 10 * fr.E2E_TOL[n, band], "the parabola through |c| is biased by the sinc; the estimator earns its place"


def test_a_carrier_gives_a_finite_answer_and_a_flat_correlation_none():
    a, b = fr.e2e_pair(4096, "full", 3.37, carrier=True)
    got = tdoa.fine_lag(fr.fine(a, b, 3, 16).corr())
    print("carrier:", got)
    assert all(math.isfinite(v) for v in got[:5]) and got.coarse == 3
    zero = tdoa.fine_lag(gpsjam.FineCorr(np.arange(-16, 17), np.zeros(33, np.complex128), None, 100))
    assert not zero.ok and zero.lag == 0.0 and zero.delta == 0.0
    one = tdoa.fine_lag(fr.fine(a, b, 3, 0).corr())
    assert one.coarse == 3 and abs(one.delta) < 1e-12 and one.lag == 3.0, "a single lag carries no slope"


def test_frequency_offset_is_taken_out_per_block():
    n, delay, tol = 50000, 3.37, fr.E2E_TOL[50000, "full"]
    a, b = fr.e2e_pair(n, "full", delay, offset_hz=fr.E2E_OFFSET_HZ)
    corr = fr.fine(a, b, 3, fr.E2E_HALF).corr(want_blocks=True)
    with_it, without = tdoa.fine_lag(corr, offset_hz=fr.E2E_OFFSET_HZ), tdoa.fine_lag(corr)
    print(f"60 Hz between the receivers: offset_hz=60 {with_it}")
    print(f"                             offset_hz=0  {without}")
    assert with_it.ok and abs(with_it.lag - delay) <= tol and abs(with_it.phase - fr.E2E_PHASE) < 0.02
    assert abs(without.lag - delay) > tol and abs(without.phase - fr.E2E_PHASE) > 1.0 and without.spread > 5 * with_it.spread
    with pytest.raises(ValueError):
        tdoa.fine_lag(corr._replace(blocks=None), offset_hz=fr.E2E_OFFSET_HZ)
