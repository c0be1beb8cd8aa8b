"""The short-time kernels (gj_ridge_dev, gj_chirp_dev, gj_sk_dev) and the two excisors (gj_excise_dev,
gj_excise_chirp_dev) on saturated and degenerate captures: constant 0, constant 255, constant 128/127, the Nyquist
pattern at full scale, uniform bytes, a hard-clipped tone, quiet then rail to rail, one impulse
(tests/extremes_inputs.py), under both unpack conventions.

This file sits in a package of its own for the reason tests/ridge/test_round6_gpu.py gives: the suite orders GPU files
by basename (tests/conftest.py SUITE_ORDER), and under this name it runs in stage 2.

Yardsticks: the float64 restatements of the parity tests with the parity tests' tolerances -- rtol 1e-5 on total, peak
and peaks, 1e-5 * peak on second, sr.S1_TOL / sr.S2_TOL, skurt's check_sk -- through the parity files' run() helpers
(sentinel-filled buffers, nothing written behind the output).  New is only the handling of EXACT ties, which these
inputs have by construction: a frame is clear if the restatement's margin is at least NEAR_TIE; on clear frames bin and
rate are equal, on the others the GPU's choice must be a candidate, its float64 power within NEAR_TIE of the maximum
(the rule of compare_chirp in tests/stft_scale).  Which frames are clear comes from the restatement
(tests/extremes_inputs.py, asserted by tests/test_extremes_host.py), never from the GPU's own result.  A frame without
power has total, peak and second 0 and bin 0."""
import numpy as np
import pytest

import chirp_restatement as cr
import excise_restatement as er
import extremes_inputs as xi
import gpsjam
import ridge_restatement as rr
import skurt_restatement as sr
from gpu_lib import Convention, Resident, run_chirp, run_excise, run_excise_chirp, run_ridge, run_sk

pytestmark = pytest.mark.gpu

RTOL = cr.RTOL
assert RTOL == rr.RTOL == 1e-5


@pytest.fixture(scope="module")
def caps(dev):
    """The captures resident, uploaded on first use."""
    held = {}

    def get(name):
        if name not in held:
            held[name] = dev.capture(xi.capture(name))
        return held[name]
    yield get
    for c in held.values():
        c.free()


def within(got, want, scale, what):
    """|got - want| <= RTOL * scale, element by element: where the scale is 0 the value must be 0."""
    err = np.abs(got.astype(np.float64) - want)
    bad = err > RTOL * scale
    assert not bad.any(), (what, int(bad.sum()), float(np.max(err[bad] / np.maximum(scale[bad], 1e-300))))


def compare_records(got, rec, clear, what):
    """Records of the ridge's layout: total on every frame, peak, second and the bin on the clear ones; everything 0 on
    a frame without power."""
    assert got.size == rec.size, what
    within(got["total"], rec["total"], rec["total"], (what, "total"))
    within(got["peak"][clear], rec["peak"][clear], rec["peak"][clear], (what, "peak"))
    within(got["second"][clear], rec["second"][clear], rec["peak"][clear], (what, "second"))
    np.testing.assert_array_equal(got["peak_bin"][clear], rec["peak_bin"][clear], err_msg=str(what))
    dead = rec["total"] == 0
    for key in ("total", "peak", "second", "peak_bin"):
        assert not got[key][dead].any(), (what, key, "a frame without power")


# ------------------------------------------------------------------------------------------------ 1. ridge
@pytest.mark.parametrize("nfft", xi.RIDGE_NFFT)
@pytest.mark.parametrize("name", xi.NAMES)
def test_ridge(dev, caps, name, nfft):
    cap = caps(name)
    for offset, scale in xi.CONVENTIONS:
        with Convention(dev, offset, scale):
            for hop in xi.hops(nfft):
                rec, margin = xi.ridge_reference(name, nfft, hop, offset, scale)
                tied = xi.ridge_not_clear(name, nfft, hop, offset, scale)
                clear = margin >= rr.NEAR_TIE
                what = (name, nfft, hop, offset)
                got = run_ridge(dev, cap, cap.nbytes, nfft, hop, xi.FIRST, rec.size, xi.GUARD)
                compare_records(got, rec, clear, what)
                for f in tied:                               # the GPU's bin is one of the tied ones
                    p = xi.frame_spectrum(name, nfft, xi.FIRST + int(f) * hop, offset, scale)
                    k = int(got["peak_bin"][f])
                    assert 0 <= k < nfft and p[k] >= (1.0 - rr.NEAR_TIE) * p.max(), (what, int(f), k)
                    within(got["peak"][f:f + 1], p[k:k + 1], p[k:k + 1], (what, int(f), "peak of the chosen bin"))
                if tied.size:
                    print(f"{what}: {tied.size} of {rec.size} frames tied, the GPU chose bins {sorted(set(got['peak_bin'][tied].tolist()))[:8]}")


# ------------------------------------------------------------------------------------------------ 2. chirp
@pytest.mark.parametrize("nfft", xi.CHIRP_NFFT)
@pytest.mark.parametrize("name", xi.NAMES)
def test_chirp(dev, caps, name, nfft):
    cap = caps(name)
    for offset, scale in xi.CONVENTIONS:
        with Convention(dev, offset, scale):
            for hop in xi.hops(nfft):
                for rates in xi.chirp_rate_sets(nfft):
                    want = xi.chirp_reference(name, nfft, hop, rates, offset, scale)
                    rec = want.records
                    tied = xi.chirp_not_clear(name, nfft, hop, rates, offset, scale)
                    clear = np.ones(rec.size, bool)
                    clear[tied] = False
                    what = (name, nfft, hop, rates, offset)
                    got, peaks = run_chirp(dev, cap, cap.nbytes, nfft, hop, xi.FIRST, rec.size, rates, xi.GUARD)
                    compare_records(got, rec, clear, what)
                    np.testing.assert_array_equal(got["rate_index"][clear], rec["rate_index"][clear], err_msg=str(what))
                    within(peaks, want.peaks, want.peaks, (what, "peaks"))
                    rows = np.arange(rec.size)
                    assert np.array_equal(peaks[rows, got["rate_index"]], got["peak"]), (what, "peaks[f, rate_index] is the record's peak")
                    dead = rec["total"] == 0
                    assert not got["rate_index"][dead].any(), (what, "rate of a frame without power")
                    qs = cr.rate_values(rates)
                    # a sample of the tied frames (all of them where they are few): the chosen rate's float64 peak
                    # within NEAR_TIE of the best, the chosen bin within NEAR_TIE of that rate's maximum
                    for f in tied[::max(1, tied.size // 64)]:
                        r, k = int(got["rate_index"][f]), int(got["peak_bin"][f])
                        assert 0 <= r < len(qs) and 0 <= k < nfft, (what, int(f))
                        assert want.peaks[f, r] >= (1.0 - cr.NEAR_TIE) * want.peaks[f].max(), (what, int(f), "rate")
                        p = xi.frame_spectrum(name, nfft, xi.FIRST + int(f) * hop, offset, scale, qs[r])
                        assert p[k] >= (1.0 - cr.NEAR_TIE) * p.max(), (what, int(f), "bin")


# ------------------------------------------------------------------------------------------------ 3. kurtosis
@pytest.mark.parametrize("nfft", xi.RIDGE_NFFT)
@pytest.mark.parametrize("name", xi.NAMES)
def test_kurtosis(dev, caps, name, nfft):
    cap = caps(name)
    for offset, scale in xi.CONVENTIONS:
        with Convention(dev, offset, scale):
            for hop, m in xi.sk_cases(nfft):
                p = xi.frame_powers(name, nfft, hop, offset, scale)
                n_rows = gpsjam.sk_rows(cap.nbytes, xi.FIRST, nfft, hop, m)
                assert n_rows == p.shape[0] // m >= 1
                r1, r2, _ = sr.sums_of(p, m, n_rows)
                s1, s2, skv = run_sk(dev, cap, cap.nbytes, nfft, hop, xi.FIRST, m, n_rows)
                what = (name, nfft, hop, m, offset)
                # sr.S1_TOL and sr.S2_TOL of the row's largest reference value; a row without power is 0
                assert np.all(np.abs(s1 - r1) <= sr.S1_TOL * r1.max(axis=1, keepdims=True)), (what, "S1")
                assert np.all(np.abs(s2 - r2) <= sr.S2_TOL * r2.max(axis=1, keepdims=True)), (what, "S2")
                assert np.all(np.isfinite(s1)) and np.all(np.isfinite(s2)), what
                sr.check_sk(s1, s2, skv, m, what)       # NaN exactly where the GPU's own S1 is 0


# ------------------------------------------------------------------------------------------------ 4. excisors
@pytest.fixture(scope="module")
def res(dev):
    r = Resident(dev)
    yield r
    r.free()


@pytest.mark.parametrize("nfft", xi.CHIRP_NFFT)
@pytest.mark.parametrize("name", xi.NAMES)
def test_excisors_identity_is_byte_exact(dev, caps, res, name, nfft):
    """Nothing notched (+inf): the input on every byte, through gj_excise_dev and through gj_excise_chirp_dev at every
    rate of xi.chirp_identity_rates.  No tie band: tests/test_extremes_host.py shows every value an integer to 1.2e-4."""
    cap, raw = caps(name), xi.capture(name)
    n = cap.nsamples - xi.FIRST
    nf = gpsjam.excise_frames(n, nfft)
    body = raw[2 * xi.FIRST:].tobytes()
    inf = res(np.full(nfft, np.inf))
    for offset, scale in xi.CONVENTIONS:
        with Convention(dev, offset, scale):
            runs = [("plain", run_excise(dev, cap, cap.nbytes, xi.FIRST, n, nfft, inf))]
            runs += [(q, run_excise_chirp(dev, cap, cap.nbytes, xi.FIRST, n, nfft, res(np.full(nf, q), np.int32), inf))
                     for q in xi.chirp_identity_rates(nfft)]
            want = xi.notch_reference(name, nfft, offset, scale).records["total"]     # the totals do not depend on the threshold
            for kind, (got, rec) in runs:
                what = (name, nfft, offset, kind)
                differ = int(np.sum(np.frombuffer(body, np.uint8) != got))
                assert differ == 0, (what, differ, "bytes differ")
                assert rec.size == nf and not rec["n_excised"].any() and not rec["removed"].any() and not rec["reserved"].any(), what
                within(rec["total"], want, want, (what, "total"))


def compare_notched(got, rec, want, thr, what):
    """GPU bytes and records against an er.Excised, with the tie band of these inputs: bytes equal outside the band and
    within 1 inside it, total and removed to RTOL of total (0 where the frame has no power), n_excised equal on every
    frame none of whose bins lies within NEAR_TIE of its threshold."""
    assert rec.size == want.records.size and got.size == want.out.size, what
    clear_f = xi.frames_clear_of_the_threshold(want, thr)
    np.testing.assert_array_equal(rec["n_excised"][clear_f], want.records["n_excised"][clear_f], err_msg=str(what))
    assert not rec["reserved"].any()
    tot = want.records["total"]
    for key in ("total", "removed"):
        within(rec[key], want.records[key], tot, (what, key))
    assert np.array_equal(got[:want.lo], want.out[:want.lo]) and np.array_equal(got[want.hi:], want.out[want.hi:]), (what, "edges")
    body, ref = got[want.lo:want.hi].astype(np.int16), want.out[want.lo:want.hi].astype(np.int16)
    clear = er.tie_distance(want.value) > xi.TIE_BAND
    diff = np.abs(body - ref)
    share = float(np.mean(~clear))
    print(f"{what}: {int(np.sum(diff != 0))} of {diff.size} bytes differ, {int(np.sum(~clear))} lie in the tie band ({share:.2e}), "
          f"{int(np.sum(~clear_f))} frames near the threshold")
    assert share <= xi.TIE_SHARE_CAP, (what, share)
    assert not diff[clear].any(), (what, int(np.sum(diff[clear] != 0)), "bytes differ outside the tie band")
    assert diff.max(initial=0) <= 1, (what, int(diff.max()))


@pytest.mark.parametrize("name,nfft,offset,scale", xi.notch_cases())
def test_excisor_notches(dev, caps, res, name, nfft, offset, scale):
    cap = caps(name)
    thr = er.parity_threshold(nfft, scale)
    want = xi.notch_reference(name, nfft, offset, scale)
    with Convention(dev, offset, scale):
        got, rec = run_excise(dev, cap, cap.nbytes, xi.FIRST, cap.nsamples - xi.FIRST, nfft, res(thr))
    compare_notched(got, rec, want, thr, (name, nfft, offset))


@pytest.mark.parametrize("name,nfft,offset,scale", xi.chirp_notch_cases())
def test_chirp_excisor_notches(dev, caps, res, name, nfft, offset, scale):
    """The same threshold through gj_excise_chirp_dev, the rates 0, 3 and -N^2/2 on consecutive frames."""
    cap = caps(name)
    thr = er.parity_threshold(nfft, scale)
    want = xi.chirp_notch_reference(name, nfft, offset, scale)
    with Convention(dev, offset, scale):
        got, rec = run_excise_chirp(dev, cap, cap.nbytes, xi.FIRST, cap.nsamples - xi.FIRST, nfft, res(xi.chirp_notch_rates(nfft), np.int32), res(thr))
    compare_notched(got, rec, want, thr, ("chirp excisor", name, nfft, offset))


@pytest.mark.parametrize("nfft", xi.CLAMP_NFFT)
def test_excisor_clamps_at_both_ends(dev, res, nfft):
    """The one input here whose notched output leaves [0, 255] before rounding (tests/test_extremes_host.py)."""
    raw, thr = er.clamp_capture(), er.clamp_threshold(nfft)
    want = xi.clamp_reference(nfft)
    assert want.value.max() > 255.5 and want.value.min() < -0.5
    with dev.capture(raw) as cap:
        got, rec = run_excise(dev, cap, cap.nbytes, xi.FIRST, cap.nsamples - xi.FIRST, nfft, res(thr))
    compare_notched(got, rec, want, thr, ("clamp", nfft))
    assert (got == 0).any() and (got == 255).any()
