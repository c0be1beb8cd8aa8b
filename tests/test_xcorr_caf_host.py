"""CPU side of the cross-ambiguity search (gj_xcorr_caf_dev): the numpy / scipy restatement the GPU tests compare with
(tests/caf_restatement.py) is checked against itself and against the reference's own call, the reason the feature
exists is shown in numbers, and the host-only pieces of the new interface are pinned.  No GPU call is made."""
import ctypes as C
import inspect
import os
import sys

import numpy as np
import pytest
from scipy import signal

import caf_restatement as caf
import gpsjam
from gpsjam import _ffi

HERE = os.path.dirname(os.path.abspath(__file__))
SKRYPTY = os.path.join(os.path.dirname(HERE), "gps-jamming_amd", "skrypty")
if SKRYPTY not in sys.path:
    sys.path.insert(0, SKRYPTY)

N = caf.N_REF
FIRST, NBINS = caf.BINS_REF


@pytest.fixture(scope="module")
def surfaces():
    """Per case: the two slices, the float64 sweep and the direct (complex64, scipy.signal.correlate) evaluation."""
    out = []
    for k, (d, f) in enumerate(caf.CASES):
        a0, a1 = caf.make_antennas(N, [(0, 0.0), (d, f)], seed=100 + k)
        out.append((a0, a1, caf.search(a1, a0, FIRST, NBINS), caf.search_direct(a1, a0, FIRST, NBINS)))
    return out


def test_the_two_evaluations_of_the_definition_agree(surfaces):
    worst = 1.0
    for (d, f), (a0, a1, fast, direct) in zip(caf.CASES, surfaces):
        assert (fast.lag, fast.bin) == (direct.lag, direct.bin) == (d, int(round(f))), ((d, f), fast[:5], direct[:5])
        np.testing.assert_allclose(fast.peak, direct.peak, rtol=1e-5)
        for b, (x, y) in enumerate(zip(fast.bins, direct.bins)):
            np.testing.assert_allclose(x.peak, y.peak, rtol=1e-5)
            if x.margin >= caf.LAG_NEAR_TIE:
                assert x.lag == y.lag, ((d, f), FIRST + b, x, y)
            worst = min(worst, x.margin)
        # bin 0 IS the reference's call on the unrotated slices: this pins the sign convention of the lag
        c = signal.correlate(caf.unpack(a1), caf.unpack(a0), mode="full")
        m = int(np.argmax(np.abs(c)))
        zero = direct.bins[-FIRST]
        assert zero.lag == m - (N - 1) and zero.peak == float(np.abs(c[m]))
    assert worst > caf.LAG_NEAR_TIE, worst     # no (case, bin) cell of these inputs is a near tie: the GPU test compares them all


def test_plain_correlation_fails_under_an_offset_and_the_search_does_not(surfaces):
    """Why the feature exists: a 300-Hz offset turns the phase seven times over the reference's 24-ms slice."""
    want_margin_bin = [0.22, 0.048, 0.22, 0.22]     # |sinc| of the neighbouring bin at n / L = 50000 / 131072
    for (d, f), (a0, a1, fast, _), mb in zip(caf.CASES, surfaces, want_margin_bin):
        plain = caf.plain_lag(a1, a0)
        if f != 0.0:
            assert plain != d and abs(plain - d) > 100, ((d, f), plain)
            assert fast.peak > 30 * fast.bins[-FIRST].peak
        else:
            assert plain == d
        assert (fast.lag, fast.bin) == (d, int(round(f)))
        assert abs(fast.margin_bin - mb) < 0.01, ((d, f), fast.margin_bin)
    # the positive direction: antenna 1 sees the source HIGHER by f bins -> bin +f
    assert surfaces[0][2].bin == 21 and surfaces[2][2].bin == -57


def test_fft_len_and_bin_width():
    lib = _ffi.load()
    for n in (1, 32768, 32769, 50000, 1 << 19, 1 << 23):
        L = 65536
        while L < 2 * n - 1:
            L *= 2
        assert lib.gj_xcorr_fft_len(n) == L == caf.fft_len(n) == gpsjam.xcorr_fft_len(n), n
    assert [lib.gj_xcorr_fft_len(n) for n in (1, 32768, 32769, 50000, 1 << 19, 1 << 23)] == \
           [65536, 65536, 131072, 131072, 1 << 20, 1 << 24]
    assert gpsjam.xcorr_bin_hz(50000, 2.048e6) == 2.048e6 / 131072 == 15.625
    assert gpsjam.caf_bin_range(50000, 1000.0, 2.048e6) == (-64, 129)
    assert gpsjam.caf_bin_range(50000, 0.0) == (0, 1)


def test_result_record_layout():
    text = open(os.path.join(os.path.dirname(HERE), "include", "gpsjam.h")).read()
    body = text[text.index("typedef struct gj_caf_result"):text.index("} gj_caf_result;")]
    fields = [ln.split(";")[0].split()[-1] for ln in body.splitlines()[1:] if ";" in ln]
    assert fields == [f[0] for f in _ffi.CafResult._fields_] == ["lag", "bin", "peak", "margin_lag", "margin_bin", "reserved"]
    assert C.sizeof(_ffi.CafResult) == 24 and C.sizeof(_ffi.CafResult) % 8 == 0
    assert _ffi.CafResult.bin.offset == 4 and _ffi.CafResult.margin_bin.offset == 16
    assert "#define GJ_CAF_MAX_BINS %d" % _ffi.GJ_CAF_MAX_BINS in text
    assert gpsjam.CafPeak._fields == ("lag", "bin", "offset_hz", "peak", "margin_lag", "margin_bin")


def test_python_and_dropin_surface():
    params = lambda f: list(inspect.signature(f).parameters)
    assert params(gpsjam.Device.xcorr_caf) == ["self", "slices", "pairs", "max_offset_hz", "bins", "fs", "want_ridge"]
    sig = inspect.signature(gpsjam.Device.xcorr_caf)
    assert sig.parameters["fs"].default == 2.048e6 and sig.parameters["want_ridge"].default is False
    assert params(gpsjam.Device.xcorr_caf_dev)[:8] == ["self", "d_iqs", "nbytes_list", "d_starts", "n_samples", "pairs", "bin_first",
                                                      "n_bins"]
    assert params(gpsjam.Device.xcorr_caf_slots_dev)[:8] == ["self", "d_slots", "slot_stride", "n_ant", "n_samples", "pairs",
                                                            "bin_first", "n_bins"]
    assert params(gpsjam.Device.xcorr_caf_workspace) == ["self", "n_ant", "n_samples", "n_pairs", "n_bins", "bins_per_launch"]
    assert params(gpsjam.xcorr_bin_hz) == ["n_samples", "fs"]
    import triangulateTDOA as tdoa
    assert params(tdoa.correlation_lag_offset) == ["signal1_slice", "signal0_slice", "max_offset_hz"]
    assert params(tdoa.correlation_lag) == ["signal1_slice", "signal0_slice"]
    assert tdoa.FREQ_SEARCH_HZ == 0.0 and isinstance(tdoa.FREQ_SEARCH_HZ, float)
