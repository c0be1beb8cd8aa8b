"""Fine TDOA on the GPU: the exact lag-window correlation (gj_xcorr_fine_dev, Device.xcorr_fine) and the sub-sample
delay made from it (gpsjam.tdoa, skrypty/triangulateTDOA.correlation_lag_fine).

This file sits in a package of its own on purpose, as tests/blank/ does: the suite orders GPU files by basename
(tests/conftest.py SUITE_ORDER, which tests/test_suite_order.py holds every GPU file to), and under the name
test_round6_gpu.py it runs in stage 2.

Yardstick: the int64 restatement of the definition in include/gpsjam.h (tests/fine_restatement.py, which
tests/test_fine_host.py holds to a per-sample double loop).  Everything is integer arithmetic, so EVERY total and EVERY
block record is equal, bit for bit.  Every call writes into sentinel-filled buffers whose 256 bytes behind d_total and
behind d_blocks must stay untouched."""
import os
import sys

import numpy as np
import pytest

SKRYPTY = os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "gps-jamming_amd", "skrypty")
if SKRYPTY not in sys.path:
    sys.path.append(SKRYPTY)

import blank_restatement as br
import fine_restatement as fr
import gpsjam
import k5_check
from gpsjam import tdoa
from gpu_lib import GJ_ERR_INVALID, GJ_ERR_UNSUPPORTED, Guarded, freed, refused
from gpu_lib import run_fine as run

pytestmark = pytest.mark.gpu



@pytest.fixture(scope="module")
def caps(dev):
    a, b = (dev.capture(raw) for raw in fr.parity_captures())
    yield a, b
    a.free()
    b.free()


def compare(got, want, what):
    total, blocks = got
    np.testing.assert_array_equal(total, want.total, err_msg=f"{what} total")
    if blocks is not None:
        np.testing.assert_array_equal(blocks.astype(np.int64), want.blocks, err_msg=f"{what} blocks")


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("half", fr.PARITY_HALVES)
def test_parity_with_the_restatement(dev, caps, half):
    a, b = caps
    try:
        for offset, scale in fr.CONVENTIONS:
            dev.set_unpack(offset, scale)
            for centre in fr.PARITY_CENTRES:
                want = fr.parity_reference(centre, half, offset)
                with_blocks = run(dev, a, b, fr.PARITY_FIRST_A, fr.PARITY_FIRST_B, fr.PARITY_SAMPLES, centre, half)
                compare(with_blocks, want, (half, centre, offset))
                without = run(dev, a, b, fr.PARITY_FIRST_A, fr.PARITY_FIRST_B, fr.PARITY_SAMPLES, centre, half, want_blocks=False)
                assert without[0].tobytes() == with_blocks[0].tobytes(), "d_blocks = NULL changes no bit of the total"
                print(f"R {half} centre {centre} offset {offset}: peak |C4| {np.abs(want.total[:, 0] + 1j * want.total[:, 1]).max():.4g}, all equal")
    finally:
        dev.set_unpack()
    assert dev.get_unpack() == (127.5, 1.0 / 127.5)


@pytest.mark.parametrize("n", [1, 5])
def test_ranges_shorter_than_the_window(dev, caps, n):
    a, b = caps
    for centre in (0, 2, -3):
        want = fr.parity_reference(centre, 32, 127.5, n)
        compare(run(dev, a, b, fr.PARITY_FIRST_A, fr.PARITY_FIRST_B, n, centre, 32), want, (n, centre))


# ------------------------------------------------------------------------------------------------ 2. extremes
def test_saturated_blocks_do_not_wrap(dev):
    """fr.EXTREME_CASES, see tests/test_fine_host.py: +2 130 739 200 is reached (255 against 255 at offset 0, 0 against 0
    at offset 255); 0 against 255 at offset 255 is exactly 0, byte 255 being the sample zero there; no negative record
    reaches the bound, the most negative one that bytes can make is included."""
    n = fr.BLOCK
    try:
        for (va, vb, offset), want in fr.EXTREME_CASES.items():
            dev.set_unpack(offset, 1.0 / 127.5)
            with dev.capture(np.full(2 * n, va, np.uint8)) as a, dev.capture(np.full(2 * n, vb, np.uint8)) as b:
                total, blocks = run(dev, a, b, 0, 0, n, 0, 1)
            assert blocks[0, 1].tolist() == [want, 0] and total[1].tolist() == [want, 0], (va, vb, offset, blocks[0, 1])
            assert total[0].tolist() == total[2].tolist() == [want // n * (n - 1), 0]
        # the total past 2^32: 2^22 + 5 saturated samples against the closed form
        dev.set_unpack(0.0, 1.0 / 127.5)
        n = 2 ** 22 + 5
        with dev.capture(np.full(2 * n, 255, np.uint8)) as a:
            total, blocks = run(dev, a, a, 0, 0, n, 0, 2)
        want = [(n - abs(k)) * 2 * 510 ** 2 for k in range(-2, 3)]
        assert total[:, 0].tolist() == want and not total[:, 1].any() and want[2] > 2 ** 32
        assert blocks[:-1, 2, 0].tolist() == [fr.BLOCK_BOUND] * (n // fr.BLOCK) and blocks[-1, 2, 0] == 5 * 2 * 510 ** 2
        assert int(blocks[:, :, 0].astype(np.int64).sum()) == sum(want)
    finally:
        dev.set_unpack()


# ------------------------------------------------------------------------------------------------ 3. autocorrelation
def test_autocorrelation(dev):
    raw = br.parity_capture()
    first, n = br.PARITY_FIRST, br.PARITY_SAMPLES
    with dev.capture(raw) as c:
        total, blocks = run(dev, c, c, first, first, n, 0, 16)
        compare((total, blocks), fr.fine(raw, raw, 0, 16, first, first, n), "d_a == d_b")
        assert total[16, 1] == 0 and np.array_equal(total[::-1, 0], total[:, 0]) and np.array_equal(total[::-1, 1], -total[:, 1])
        # C4[0] per block is the blanker's `total` record at a threshold that never blanks
        out, rec = dev.alloc(2 * n), dev.alloc(gpsjam.BLANK_DTYPE.itemsize * gpsjam.blank_blocks(n))
        try:
            dev.blank_dev(c, c.nbytes, first, n, 16, 8, np.inf, out, rec)
            blank_total = rec.download(gpsjam.BLANK_DTYPE)["total"]
        finally:
            out.free()
            rec.free()
        assert np.array_equal(blocks[:, 16, 0].astype(np.uint64), blank_total) and not blocks[:, 16, 1].any()
        # the same capture, overlapping ranges 7 samples apart: the peak moves to lag -7
        shifted = run(dev, c, c, first, first + 7, n - 7, -7, 4)
        compare(shifted, fr.fine(raw, raw, -7, 4, first, first + 7, n - 7), "overlapping ranges")
        assert int(np.argmax(shifted[0][:, 0])) == 4 and shifted[0][4, 1] == 0


# ------------------------------------------------------------------------------------------------ 4. range independence
def test_the_result_depends_on_the_bytes_of_the_ranges_alone(dev, caps):
    a, b = caps
    raw_a, raw_b = fr.parity_captures()
    fa, fb, n = fr.PARITY_FIRST_A, fr.PARITY_FIRST_B, fr.PARITY_SAMPLES
    whole = run(dev, a, b, fa, fb, n, 3, 16)
    again = run(dev, a, b, fa, fb, n, 3, 16)
    assert whole[0].tobytes() == again[0].tobytes() and whole[1].tobytes() == again[1].tobytes(), "two calls, identical bits"
    # the two ranges cut out as captures of their own (even starts, nothing around them)
    with dev.capture(raw_a[2 * fa:2 * (fa + n)]) as ca, dev.capture(raw_b[2 * fb:2 * (fb + n)]) as cb:
        cut = run(dev, ca, cb, 0, 0, n, 3, 16)
    assert cut[0].tobytes() == whole[0].tobytes() and cut[1].tobytes() == whole[1].tobytes()
    # other loud bytes outside the ranges
    noisy = []
    for raw, first in ((raw_a, fa), (raw_b, fb)):
        r = raw.copy()
        r[:2 * first] = np.random.default_rng(first).integers(0, 256, 2 * first)
        r[2 * (first + n):] = 0
        noisy.append(r)
    with dev.capture(noisy[0]) as ca, dev.capture(noisy[1]) as cb:
        other = run(dev, ca, cb, fa, fb, n, 3, 16)
    assert other[0].tobytes() == whole[0].tobytes() and other[1].tobytes() == whole[1].tobytes()


# ------------------------------------------------------------------------------------------------ 5. against K5
def against_k5(dev, raw_i, raw_j, what):
    lags, peaks = dev.xcorr_lags([raw_i, raw_j], [(0, 1)])
    corr = dev.xcorr_fine(raw_i, raw_j, lag_center=int(lags[0]), half_width=16)
    mag = np.abs(corr.c)
    print(f"{what}: K5 lag {int(lags[0])} peak {float(peaks[0]):.6g}; window's |c| at the centre {mag[16]:.6g}")
    assert int(np.argmax(mag)) == 16 and corr.lags[16] == int(lags[0]), what
    assert abs(mag[16] - float(peaks[0])) <= k5_check.PEAK_RTOL * mag[16], what
    assert np.array_equal(corr.c, fr.fine(raw_i, raw_j, int(lags[0]), 16).corr().c), what


def test_the_window_agrees_with_k5(dev, g4_raws, golden_meta):
    on = golden_meta["g4"]["onset"]
    sl = [r[2 * o:2 * (o + 50000)] for r, o in zip(g4_raws, on)]
    for i, j in ((0, 1), (0, 2), (1, 2)):
        against_k5(dev, sl[i], sl[j], f"G4 pair {i}{j}")
    a, b = fr.e2e_pair(50000, "full", 3.37)
    against_k5(dev, a, b, "synthetic, delay 3.37")


# ------------------------------------------------------------------------------------------------ 6. end to end
def test_end_to_end_refine_on_a_resident_pair(dev):
    """tdoa.refine on the resident 50 000-sample full-band pair whose b is 3.37 samples late: the same integers as the
    restatement's, so the same floats from the same host code; within fr.E2E_TOL (twice the 0.00126 sample that
    tests/test_fine_host.py measures on the CPU) of the truth; and the same lag through the drop-in."""
    n, delay = 50000, 3.37
    raw_a, raw_b = fr.e2e_pair(n, "full", delay)
    want = tdoa.fine_lag(fr.fine(raw_a, raw_b, 3, 16).corr())
    with dev.capture(raw_a) as a, dev.capture(raw_b) as b:
        uploads, calls = gpsjam.Capture.uploads, dev.kernel_calls.get("xcorr_fine", 0)
        got = tdoa.refine(dev, b, a)
        assert gpsjam.Capture.uploads == uploads and dev.kernel_calls["xcorr_fine"] == calls + 1
        blocks = dev.xcorr_fine(a, b, lag_center=3, want_blocks=True)
    print(f"refine: {got}; error {got.lag - delay:+.5f} sample, tolerance {fr.E2E_TOL[n, 'full']}")
    assert got == want, (got, want)
    assert got.ok and got.coarse == 3 and abs(got.lag - delay) <= fr.E2E_TOL[n, "full"]
    assert np.array_equal(blocks.blocks, fr.fine(raw_a, raw_b, 3, 16).corr(True).blocks) and np.array_equal(blocks.blocks.sum(axis=0), blocks.c)
    import triangulateTDOA as tt
    lag, peak = tt.correlation_lag_fine(tt.IQCapture(raw_b), tt.IQCapture(raw_a))
    assert lag == got.lag and peak == tt.correlation_lag(tt.IQCapture(raw_b), tt.IQCapture(raw_a))[1]
    geo = tt.bearing_from_lag(lag, ant1_pos=np.array([600.0, 0.0]))
    assert "error" not in geo and geo["path_difference"] == pytest.approx(delay * 299792458 / 2048000, rel=1e-3)


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_enqueue_nothing(dev, caps):
    a, b = caps
    n, nl = 3 * 4096, 33
    tot, rec = Guarded(dev, 16 * 65), Guarded(dev, 8 * 65 * 4)
    try:
        I, U = GJ_ERR_INVALID, GJ_ERR_UNSUPPORTED
        cases = [  # d_a, nbytes_a, first_a, d_b, nbytes_b, first_b, n, centre, half, d_total, d_blocks, status
            (a, a.nbytes, 0, b, b.nbytes, 0, 0, 0, 16, tot, rec, I),                          # n_samples == 0
            (a, a.nbytes, 1, b, b.nbytes, 0, a.nsamples, 0, 16, tot, rec, I),                 # a range past capture a
            (a, a.nbytes, 0, b, b.nbytes, b.nsamples - n + 1, n, 0, 16, tot, rec, I),         # ... past capture b
            (a, a.nbytes, a.nsamples + 1, b, b.nbytes, 0, 1, 0, 16, tot, rec, I),
            (a, a.nbytes, 2 ** 63, b, b.nbytes, 0, 2 ** 63 + 16, 0, 16, tot, rec, I),          # first + n wraps
            (0, a.nbytes, 0, b, b.nbytes, 0, n, 0, 16, tot, rec, I),                          # null d_a
            (a, a.nbytes, 0, 0, b.nbytes, 0, n, 0, 16, tot, rec, I),                          # null d_b
            (a.ptr + 1, a.nbytes - 2, 0, b, b.nbytes, 0, n, 0, 16, tot, rec, I),              # odd d_a
            (a, a.nbytes, 0, b.ptr + 1, b.nbytes - 2, 0, n, 0, 16, tot, rec, I),              # odd d_b
            (a, a.nbytes, 0, b, b.nbytes, 0, n, 0, 16, 0, rec, I),                            # null d_total
            (a, a.nbytes, 0, b, b.nbytes, 0, n, 0, 16, tot.ptr + 4, rec, I),                  # d_total not 8-byte aligned
            (a, a.nbytes, 0, b, b.nbytes, 0, n, 0, 16, tot, rec.ptr + 2, I),                  # d_blocks not 4-byte aligned
            (a, a.nbytes, 0, b, b.nbytes, 0, n, 2 ** 31 - 16, 16, tot, rec, I),               # |lag_center| + R overflows
            (a, a.nbytes, 0, b, b.nbytes, 0, n, -2 ** 31 + 16, 17, tot, rec, I),
            (a, a.nbytes, 0, b, b.nbytes, 0, n, -2 ** 31, 0, tot, rec, I),
            (a, a.nbytes, 0, b, b.nbytes, 0, n, 0, -1, tot, rec, U),
            (a, a.nbytes, 0, b, b.nbytes, 0, n, 0, 33, tot, rec, U),
        ]
        for c in cases:                                      # nothing written behind each one of them
            refused(dev, dev.xcorr_fine_dev, [(c[:-1], c[-1])], tot, rec)
        # accepted: the limits of the lag (no overlap: zeros), the whole captures, one sample
        dev.xcorr_fine_dev(a, a.nbytes, 0, b, b.nbytes, 0, n, 2 ** 31 - 1 - 16, 16, tot, rec)
        dev.xcorr_fine_dev(a, a.nbytes, 0, b, b.nbytes, 0, n, -2 ** 31 + 1, 0, tot, None)
        dev.xcorr_fine_dev(a, a.nbytes, a.nsamples - 1, b, b.nbytes, b.nsamples - 1, 1, 0, 32, tot, rec)
        dev.synchronize()
        tot.check_pads("totals")
        rec.check_pads("records")
    finally:
        freed(tot, rec)
    # the next valid call gives the parity bits
    compare(run(dev, a, b, fr.PARITY_FIRST_A, fr.PARITY_FIRST_B, fr.PARITY_SAMPLES, 1, nl // 2), fr.parity_reference(1, 16), "after the refusals")
    # the wrapper: a library refusal raises, frees everything and leaves the captures alone
    with pytest.raises(gpsjam.GpsJamError) as e:
        dev.xcorr_fine(a, b, half_width=40)
    assert e.value.status == GJ_ERR_UNSUPPORTED and a.ptr and b.ptr
