"""CPU side of the K2 size tests (tests/welch_sizes/test_round6_gpu.py): the float64 restatement of the Welch waterfall
(tests/welch_restatement.py) pinned to scipy.signal.welch and to gj_welch_rows, the float32 oracle and the committed
golden rows placed against it, the budgets E32 measured from the float32 restatement of K2's own form, and the proof
that every case of the GPU file is strong enough: each mutant of the float64 restatement below is further off than the
tolerance the GPU is held to.  No GPU call is made and no GPU result enters a constant."""
import os

import numpy as np
import pytest
import scipy.signal

import welch_restatement as wr
from gpsjam import _ffi
from gpsjam.synth import StreamSpec, generate
from oracle import gpsjam_oracle as orc

HERE = os.path.dirname(os.path.abspath(__file__))


# ------------------------------------------------------------------------------------------------ the definition
@pytest.mark.parametrize("nperseg", wr.SIZES)
def test_float64_restatement_is_scipy_welch(nperseg):
    """scipy.signal.welch(x, fs, nperseg=N, return_onesided=False) on complex128, chunk by chunk, to 1e-12."""
    for shape, klass in (("plus1", "modest"), ("odd", "large_dc"), ("one", "modest")):
        if shape not in wr.shapes_of(nperseg):
            continue
        chunk, samples, rows, _, _ = wr.geometry(nperseg, shape)
        raw, offset, scale = wr.case_bytes(nperseg, shape, klass)
        got = wr.welch(raw, nperseg, chunk)
        assert got.shape == (rows, nperseg) and got.dtype == np.float64
        x = wr.unpack(raw, offset, scale)
        assert x.dtype == np.complex128 and x.size == samples
        for c in range(rows):
            _, want = scipy.signal.welch(x[c * chunk:(c + 1) * chunk], wr.FS, nperseg=nperseg, return_onesided=False)
            np.testing.assert_allclose(got[c], want, rtol=1e-12, atol=0)
            # the rows are the mean of the per-segment periodograms the restatement also gives
            p = wr.periodograms(raw[2 * c * chunk:2 * (c + 1) * chunk], nperseg)
            assert p.shape == (wr.segments_in(min(chunk, samples - c * chunk), nperseg), nperseg)
            np.testing.assert_array_equal(p.mean(axis=0), got[c])
    # the other convention, and white complex128 noise that never was bytes
    raw, _, _ = wr.case_bytes(nperseg, "odd", "modest")
    chunk = wr.geometry(nperseg, "odd")[0]
    _, want = scipy.signal.welch(wr.unpack(raw, 128.0, 1 / 128.0)[:chunk], wr.FS, nperseg=nperseg, return_onesided=False)
    np.testing.assert_allclose(wr.welch(raw, nperseg, chunk, 128.0, 1 / 128.0)[0], want, rtol=1e-12, atol=0)
    rng = np.random.default_rng(nperseg)
    z = rng.normal(size=5 * nperseg + 3) + 1j * rng.normal(size=5 * nperseg + 3) + (0.3 - 0.2j)
    _, want = scipy.signal.welch(z, wr.FS, nperseg=nperseg, return_onesided=False)
    np.testing.assert_allclose(wr.periodograms_of(wr.segments(z, nperseg)).mean(axis=0), want, rtol=1e-12, atol=0)


def test_rows_that_fit_is_gj_welch_rows():
    lib = _ffi.load()
    for nperseg in wr.SIZES:
        for chunk in (nperseg, nperseg + 1, 3 * nperseg // 2, 2 * nperseg + 7, 65536):
            lengths = {0, 1, 2 * nperseg - 2, 2 * nperseg - 1, 2 * nperseg, 2 * nperseg + 1, 2 * chunk - 1, 2 * chunk, 2 * chunk + 1,
                       2 * (chunk + nperseg) - 2, 2 * (chunk + nperseg) - 1, 2 * (chunk + nperseg), 6 * chunk, 6 * chunk + 2 * nperseg - 1,
                       6 * chunk + 2 * nperseg, 40961}
            for nbytes in sorted(lengths):
                assert lib.gj_welch_rows(nbytes, chunk, nperseg) == wr.rows_that_fit(nbytes, chunk, nperseg), (nbytes, chunk, nperseg)
        # every geometry of the GPU file: the rows it names, from sample 0 and from sample 1
        for shape in wr.shapes_of(nperseg):
            chunk, samples, rows, nseg, last = wr.geometry(nperseg, shape)
            assert lib.gj_welch_rows(2 * samples, chunk, nperseg) == rows == wr.rows_that_fit(2 * samples, chunk, nperseg)
            assert wr.segments_in(chunk, nperseg) == nseg and wr.segments_in(min(chunk, samples - (rows - 1) * chunk), nperseg) == last
    assert lib.gj_welch_rows(1 << 20, 0, 16) == 0 == wr.rows_that_fit(1 << 20, 0, 16)
    assert lib.gj_welch_rows(1 << 20, 4096, 0) == 0 == wr.rows_that_fit(1 << 20, 4096, 0)


def test_geometries_reach_what_they_name():
    for nperseg in wr.SIZES:
        b, shapes = wr.groups(nperseg), wr.shapes_of(nperseg)
        assert [wr.shape_nseg(nperseg, s) for s in shapes] == sorted({wr.shape_nseg(nperseg, s) for s in wr.SHAPES} - {0})
        assert {"one", "odd", "split2", "split5"} <= set(shapes) and (b < 4 or shapes == list(wr.SHAPES))
        for shape in shapes:
            chunk, samples, rows, nseg, last = wr.geometry(nperseg, shape)
            assert samples + 1 <= wr.MAX_SAMPLES
            if nseg == 1:
                assert rows == 8 and chunk == nperseg and 0 < samples - 8 * chunk < nperseg
            else:
                assert rows == 4 and 1 <= last < nseg and samples - 3 * chunk - (nperseg + (nperseg // 2) * (last - 1)) == 3
        chunk = wr.geometry(nperseg, "odd")[0]
        assert chunk % 2 == 1 and chunk - (nperseg + (nperseg // 2) * 2 * b) == nperseg // 2 - 1
    # 2048 points: runs of 1, 2 and 3 segments
    assert [wr.shape_nseg(2048, s) for s in wr.shapes_of(2048)][:3] == [1, 2, 3]


def test_captures_are_the_generator_with_the_jammer_on_inside_the_second_chunk():
    for nperseg, shape, klass in ((16, "odd", "modest"), (1024, "plus1", "large_dc"), (4096, "split5", "modest")):
        chunk, samples, _, _, _ = wr.geometry(nperseg, shape)
        on = chunk + chunk // 2
        assert chunk < on < 2 * chunk
        dc_i, dc_q = wr.DC_Q8[klass]
        want = generate(StreamSpec(seed=nperseg, jam_start=on, jam_end=1 << 40, jam_sigma=30.0, dc_i_q8=dc_i, dc_q_q8=dc_q), samples + 1)
        assert np.array_equal(wr.capture(nperseg, shape, klass), want)
        x = wr.unpack(want, 127.5, 1.0)
        assert np.var(x[on:]) > 10 * np.var(x[:on])
        assert abs(x.real.mean() - dc_i / 256) < 1.0 and abs(x.imag.mean() - dc_q / 256) < 1.0
    for name in wr.EXTREME_NAMES:
        assert wr.capture(4096, "odd", "extreme", name).size == 2 * (wr.geometry(4096, "odd")[1] + 1)


# ------------------------------------------------------------------------------------------------ the float32 oracle
def test_oracle_and_golden_lie_within_their_measured_float32_error():
    for nperseg in wr.SIZES:
        spec = StreamSpec(seed=nperseg, jam_start=30000, jam_end=90000, jam_sigma=30.0, dc_i_q8=600, dc_q_q8=-900)
        raw = generate(spec, 2 * 65536 + max(nperseg, 5000))                  # test_gpu_parity.test_k2_all_sizes_vs_oracle
        lin, _, _ = orc.widmo_waterfall(raw, nperseg=nperseg, chunk_samples=65536)
        truth = wr.welch(raw, nperseg, 65536)
        e = wr.case_error(np.fft.ifftshift(lin, axes=1), truth)
        k2 = wr.case_error(wr.welch(raw, nperseg, 65536, single=True), truth)
        print(f"nperseg {nperseg}: oracle {e:.3e} off float64 (recorded {wr.ORACLE_E32[nperseg]:.2e}), float32 restatement of K2's form {k2:.3e}")
        assert e <= wr.ORACLE_E32[nperseg] <= 2 * e
        assert e < 1e-5 and k2 < 1e-5, "either float32 form is 10 times closer to float64 than the parity tests' 1e-4"
    import golden_inputs
    g = np.load(os.path.join(HERE, "golden", "g2_welch.npz"))
    raw = golden_inputs.g2_stream()
    for nperseg, recorded in wr.GOLDEN_E32.items():
        e = wr.case_error(np.fft.ifftshift(g[f"lin_{nperseg}"], axes=1), wr.welch(raw, nperseg, 2048000))
        print(f"nperseg {nperseg}: golden rows {e:.3e} off float64 (recorded {recorded:.2e})")
        assert e <= recorded <= 2 * e


# ------------------------------------------------------------------------------------------------ budgets
@pytest.mark.parametrize("nperseg", wr.SIZES)
def test_budgets_are_the_float32_restatements_error(nperseg):
    assert set(wr.E32[nperseg]) == set(wr.CLASSES)
    for klass in wr.CLASSES:
        measured = wr.measure_e32(nperseg, klass)
        print(f"nperseg {nperseg}, {klass}: measured {measured:.3e}, E32 {wr.E32[nperseg][klass]:.2e}, tolerance {wr.tolerance(nperseg, klass):.2e}")
        assert measured <= wr.E32[nperseg][klass] <= 2 * measured, klass
        assert wr.tolerance(nperseg, klass) == 4 * wr.E32[nperseg][klass]
    assert wr.tolerance(nperseg, "modest") < 1e-4, "otherwise the new tests add nothing over the old"
    # the float32 form's rows are float32 and are the mean of its own per-segment periodograms
    raw, chunk = wr.case_bytes(nperseg, "plus1", "modest")[0], wr.geometry(nperseg, "plus1")[0]
    p, row = wr.periodograms(raw[:2 * chunk], nperseg, single=True), wr.reference(nperseg, "plus1", "modest", None, "plain", True)[0]
    assert p.dtype == row.dtype == np.float32 and p.shape == (wr.groups(nperseg) + 1, nperseg)
    np.testing.assert_allclose(p.mean(axis=0, dtype=np.float64), row, rtol=1e-6)
    # the empty spectra: the floor carries the comparison, and they are not what sets the class's budget
    for name in ("constant 255", "constant 0", "constant 128/127"):
        truth = wr.reference(nperseg, "odd", "extreme", name)
        assert truth.max() < 1e-3 * wr.floor(nperseg)
        assert wr.case_error(wr.reference(nperseg, "odd", "extreme", name, "plain", True), truth) < 0.1 * wr.E32[nperseg]["extreme"]


# ------------------------------------------------------------------------------------------------ sensitivity
def _chunks(raw, chunk, rows):
    return [raw[2 * c * chunk:2 * (c + 1) * chunk] for c in range(rows)]


def _symmetric_hann(n):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / (n - 1))


def mutants(nperseg, shape):
    """name -> rows of a float64 Welch that is wrong in one way, on the modest capture of one shape.  The per-segment
    defects sit in ONE segment of chunk 0 (noise alone: the weakest place), the middle one."""
    chunk, samples, rows, nseg, last = wr.geometry(nperseg, shape)
    raw, offset, scale = wr.case_bytes(nperseg, shape, "modest")
    truth = wr.reference(nperseg, shape, "modest")
    segs0 = wr.segments(wr.unpack(raw[:2 * chunk], offset, scale), nperseg)
    p0 = wr.periodograms_of(segs0)
    assert np.array_equal(p0.mean(axis=0), truth[0])
    i, half = nseg // 2, nperseg // 2
    out = {}
    for name, w in (("window rotated by one sample", np.roll(wr.hann(nperseg), 1)), ("symmetric Hann", _symmetric_hann(nperseg))):
        out[name] = np.array([wr.periodograms_of(wr.segments(wr.unpack(piece, offset, scale), nperseg), window=w).mean(axis=0)
                              for piece in _chunks(raw, chunk, rows)])
    m = truth.copy()
    m[-1] *= last / (last + 1.0)
    out["nseg off by one in the last chunk's scale"] = m
    means = segs0.mean(axis=1)
    means[i] += scale                                             # one LSB on I
    m = truth.copy()
    m[0] = wr.periodograms_of(segs0, means=means).mean(axis=0)
    out["the mean of one segment off by one LSB"] = m
    # the correction is S/4 on both bins, so exchanging the corrections alone changes nothing: the mutant is the slip
    # in the bin lookup that makes them land on each other's bin, X[1] and X[N-1] exchanged, in one segment
    p = p0.copy()
    p[i, [1, nperseg - 1]] = p[i, [nperseg - 1, 1]]
    m = truth.copy()
    m[0] = p.mean(axis=0)
    out["bins 1 and N-1 swapped in the mean removal"] = m
    if nseg >= 2:
        j = min(i, nseg - 2)
        p = p0.copy()
        p[j] = p0[j + 1]
        m = truth.copy()
        m[0] = p.mean(axis=0)
        out["one segment replaced by its neighbour"] = m
        s = np.array(segs0)
        s[j, half:] = segs0[j + 1, half:]
        m = truth.copy()
        m[0] = wr.periodograms_of(s).mean(axis=0)
        out["the second half of one segment taken from the next"] = m
    return out


@pytest.mark.parametrize("nperseg", wr.SIZES)
def test_every_mutant_is_over_the_gpu_tolerance(nperseg):
    """Each mutant on every shape that has the segments for it -- the largest nseg of the size, where one segment is
    diluted most, included."""
    tol = wr.tolerance(nperseg, "modest")
    seen = set()
    for shape in wr.shapes_of(nperseg):
        truth = wr.reference(nperseg, shape, "modest")
        for name, rows in mutants(nperseg, shape).items():
            e = wr.case_error(rows, truth)
            print(f"nperseg {nperseg}, {shape} ({wr.shape_nseg(nperseg, shape)} segments): {name}: {e:.2e} ({e / tol:.0f} x the tolerance)")
            assert e > tol, (shape, name)
            seen.add(name)
    assert len(seen) == 7
    assert "one segment replaced by its neighbour" in mutants(nperseg, "split5")
