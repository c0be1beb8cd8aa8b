"""The five short-time kernels (gj_ridge_dev, gj_chirp_dev, gj_sk_dev, gj_excise_dev, gj_excise_chirp_dev) at the scale a
long capture gives them: many steps per workgroup, excisor runs longer than four frames, offsets past byte 2^32.

This file sits in a package of its own for the reason tests/ridge/test_round6_gpu.py gives: the suite orders GPU files by
basename (tests/conftest.py SUITE_ORDER, which tests/test_suite_order.py holds every GPU file to), and under the name
test_round6_gpu.py it runs in stage 2, behind the parity tests of K2 whose transform the kernels share.

The parity tests of tests/ridge, chirp, skurt, excise and excise_chirp run on 2^15 to 2^17 samples.  On 256 CUs every
workgroup then takes ONE step of `for (; step < nsteps; step += gridDim.x)`, so neither the prefetch of the next step's
frame, nor the reuse of the reduction rows in LDS, nor the hand-over of the kurtosis's next block is ever exercised, and
every excisor run holds four frames.  Here:
  * ridge, chirp and kurtosis take 1541 (kurtosis: 1542) steps, three or four per workgroup and unevenly many;
  * the excisors get 2048 B + 1 frames: runs of five with a short last run;
  * all five run on a window at sample 2^31 + 1 of a buffer of 4 GiB + 1 MiB.
Each test reads the device's CU count and asserts its regime before it compares anything.

Yardsticks, all of them the existing ones: the float64 restatements (tests/*_restatement.py, evaluated in blocks by
tests/stft_scale_inputs.py) with the parity tests' tolerances -- rtol 1e-5 on total, peak and peaks, 1e-5 * peak on
second, sr.S1_TOL / sr.S2_TOL, two ulps on SK, er/xr.TIE_BAND and xr.TIE_SHARE_CAP on bytes -- and bit-exactness against
short calls of the same kernels, which the parity tests tie to the restatements.  New are only SCALE_TIE_SHARE_CAP (the
share of chirp frames with a nearly tied rate or bin, which 400 000 frames cannot be seeded free of) and the seed of the
excisors' capture; tests/test_stft_scale_host.py asserts what they rest on.  Every call writes into sentinel-filled
buffers whose bytes behind the asked-for output must stay untouched: the run() helpers of the five parity files."""
import numpy as np
import pytest

import chirp_restatement as cr
import excise_chirp_restatement as xr
import excise_restatement as er
import gpsjam
import ridge_restatement as rr
import skurt_restatement as sr
import stft_scale_inputs as si
from gpu_lib import GJ_ERR_INVALID, Guarded, Resident, freed, refused, run_chirp, run_excise_chirp, run_ridge, run_sk

pytestmark = pytest.mark.gpu

RTOL = cr.RTOL
assert RTOL == rr.RTOL == xr.RTOL == 1e-5


@pytest.fixture(scope="module")
def cus(dev):
    return dev.info()["compute_units"]


@pytest.fixture(scope="module")
def tone(dev):
    c = dev.capture(si.scale_tone_capture())
    yield c
    c.free()


@pytest.fixture(scope="module")
def sweeps(dev):
    """scale_sweep_capture(nfft) resident, one per size, uploaded on first use."""
    held = {}

    def get(nfft):
        if nfft not in held:
            held[nfft] = dev.capture(si.scale_sweep_capture(nfft))
        return held[nfft]
    yield get
    for c in held.values():
        c.free()


@pytest.fixture(scope="module")
def res(dev):
    r = Resident(dev)
    yield r
    r.free()


def many_steps(cus, min_waves, nsteps, what):
    """The regime of the looping kernels: the call's grid; some workgroup takes three steps at least."""
    assert si.STEPS > 2 * 3 * cus, f"{what}: {si.STEPS} steps are sized for {si.SIZED_FOR_CUS} CUs, this device has {cus}"
    grid, most, fewest = si.one_round(cus, min_waves, nsteps)
    assert most >= 3 and grid * most >= nsteps > grid * (most - 1), (what, grid, most)
    print(f"{what}: {nsteps} steps on a grid of {grid}: {most} steps per workgroup, {fewest} for the last ones")
    return grid


def pieces(grid, b, n):
    """(first frame, frames) of three pieces of at most 64 steps: the head, one that begins in the second round of the
    long call's grid (on an odd frame), one that ends on the last frame."""
    m = min(64 * b, n)
    assert grid * b + 1 + m <= n
    return [(0, m), (grid * b + 1, m), (n - m, m)]


def one_step_each(cus, min_waves, nsteps):
    grid, most, _ = si.one_round(cus, min_waves, nsteps)
    return most == 1 and grid == nsteps


def rel(got, want, scale=None):
    return float(np.max(np.abs(got - want) / (want if scale is None else scale)))


# ------------------------------------------------------------------------------------------------ 1. ridge
@pytest.mark.parametrize("nfft", rr.PARITY_NFFT)
def test_ridge_at_1541_steps(dev, cus, tone, nfft):
    b, hop, n = si.per_step(nfft), si.scale_hop(nfft), si.scale_frames(nfft)
    grid = many_steps(cus, si.ridge_min_waves(nfft), si.STEPS, f"ridge {nfft}")
    want, margin = si.ridge_reference(nfft)
    assert margin.min() >= rr.NEAR_TIE
    got = run_ridge(dev, tone, tone.nbytes, nfft, hop, si.FIRST, n, si.GUARD)
    print(f"ridge {nfft}: {n} frames, peak_bin differs on {int(np.sum(got['peak_bin'] != want['peak_bin']))}, total {rel(got['total'], want['total']):.2e}, "
          f"peak {rel(got['peak'], want['peak']):.2e}, second {rel(got['second'], want['second'], want['peak']):.2e} (tolerance {RTOL:.0e})")
    rr.compare(got, want, (nfft, hop, "1541 steps"))
    assert run_ridge(dev, tone, tone.nbytes, nfft, hop, si.FIRST, n, si.GUARD).tobytes() == got.tobytes(), "the long call repeated"
    for k, m in pieces(grid, b, n):
        assert one_step_each(cus, si.ridge_min_waves(nfft), -(-m // b))
        piece = run_ridge(dev, tone, tone.nbytes, nfft, hop, si.FIRST + k * hop, m, si.GUARD)
        assert piece.tobytes() == got[k:k + m].tobytes(), (nfft, k, m)


# ------------------------------------------------------------------------------------------------ 2. chirp
def compare_chirp(got, peaks, want, raw, nfft, rates, what):
    """The comparison of tests/chirp/test_round6_gpu.py::compare on the clear frames; on the others the GPU's choice must
    be one of the nearly tied candidates of the restatement.  d_peaks is compared on every frame and every rate."""
    rec = want.records
    assert got.size == rec.size and peaks.shape == want.peaks.shape, what
    clear = si.clear_frames(want)
    share = 1.0 - float(clear.mean())
    errs = {"peaks": rel(peaks, want.peaks)}
    for key in ("total", "peak"):
        errs[key] = rel(got[key][clear], rec[key][clear])
    errs["second"] = rel(got["second"][clear], rec["second"][clear], rec["peak"][clear])
    wrong = int(np.sum(((got["rate_index"] != rec["rate_index"]) | (got["peak_bin"] != rec["peak_bin"]))[clear]))
    print(f"{what}: {got.size} frames, {int(np.sum(~clear))} not clear ({share:.2e}, cap {si.SCALE_TIE_SHARE_CAP:.1e}), rate or bin differs on "
          f"{wrong} clear frames, errors {({k: f'{v:.2e}' for k, v in errs.items()})} (tolerance {RTOL:.0e})")
    assert share <= si.SCALE_TIE_SHARE_CAP, (what, share)
    assert errs["peaks"] <= RTOL, (what, "peaks", errs["peaks"])
    np.testing.assert_array_equal(got["rate_index"][clear], rec["rate_index"][clear], err_msg=str(what))
    np.testing.assert_array_equal(got["peak_bin"][clear], rec["peak_bin"][clear], err_msg=str(what))
    for key in ("total", "peak", "second"):
        assert errs[key] <= RTOL, (what, key, errs[key])
    rows = np.arange(got.size)
    assert np.array_equal(peaks[rows, got["rate_index"]], got["peak"]), (what, "peaks[f, rate_index] is the record's peak")
    # the frames that are not clear: the chosen rate's float64 peak within NEAR_TIE of the best, the chosen bin within
    # NEAR_TIE of that rate's maximum
    x = rr.unpack(raw)
    qs = cr.rate_values(rates)
    for f in np.flatnonzero(~clear):
        r, k = int(got["rate_index"][f]), int(got["peak_bin"][f])
        assert 0 <= r < len(qs) and 0 <= k < nfft, (what, f)
        assert want.peaks[f, r] >= (1.0 - cr.NEAR_TIE) * want.peaks[f].max(), (what, f, "rate")
        p = si.chirp_spectrum(x, nfft, si.FIRST + int(f) * si.scale_hop(nfft), qs[r])
        assert p[k] >= (1.0 - cr.NEAR_TIE) * p.max(), (what, f, "bin")


@pytest.mark.parametrize("nfft", si.CHIRP_NFFT)
def test_chirp_at_1541_steps(dev, cus, sweeps, nfft):
    b, hop, n, rates = si.per_step(nfft), si.scale_hop(nfft), si.scale_frames(nfft), si.RATES
    grid = many_steps(cus, si.chirp_min_waves(nfft), si.STEPS, f"chirp {nfft}")
    cap = sweeps(nfft)
    assert gpsjam.ridge_frames(cap.nbytes, si.FIRST, nfft, hop) == n
    got, peaks = run_chirp(dev, cap, cap.nbytes, nfft, hop, si.FIRST, n, rates, si.GUARD)
    compare_chirp(got, peaks, si.chirp_reference(nfft), si.scale_sweep_capture(nfft), nfft, rates, f"chirp {nfft}")
    again, pagain = run_chirp(dev, cap, cap.nbytes, nfft, hop, si.FIRST, n, rates, si.GUARD)
    assert again.tobytes() == got.tobytes() and pagain.tobytes() == peaks.tobytes(), "the long call repeated"
    for k, m in pieces(grid, b, n):
        assert one_step_each(cus, si.chirp_min_waves(nfft), -(-m // b))
        piece, ppiece = run_chirp(dev, cap, cap.nbytes, nfft, hop, si.FIRST + k * hop, m, rates, si.GUARD)
        assert piece.tobytes() == got[k:k + m].tobytes() and ppiece.tobytes() == peaks[k:k + m].tobytes(), (nfft, k, m)


@pytest.mark.parametrize("nfft", si.CHIRP_RIDGE_NFFT)
def test_rate_zero_is_gj_ridge_dev_byte_for_byte_at_1541_steps(dev, cus, sweeps, nfft):
    """Also the ridge's only many-step run on an input whose peak bin moves from frame to frame."""
    hop, n, rates = si.scale_hop(nfft), si.scale_frames(nfft), (0, 1, 1)
    many_steps(cus, si.chirp_min_waves(nfft), si.STEPS, f"chirp {nfft} at rate 0")
    many_steps(cus, si.ridge_min_waves(nfft), si.STEPS, f"ridge {nfft} on the sweep")
    cap = sweeps(nfft)
    got, peaks = run_chirp(dev, cap, cap.nbytes, nfft, hop, si.FIRST, n, rates, si.GUARD)
    ridge = run_ridge(dev, cap, cap.nbytes, nfft, hop, si.FIRST, n, si.GUARD)
    head = np.ascontiguousarray(got.view(np.uint8).reshape(n, gpsjam.CHIRP_DTYPE.itemsize)[:, :16])
    assert head.tobytes() == ridge.tobytes(), nfft
    assert not got["rate_index"].any() and peaks[:, 0].tobytes() == got["peak"].tobytes()
    moves = int(np.sum(np.diff(ridge["peak_bin"]) != 0))
    print(f"ridge {nfft} on the sweep: the peak bin changes {moves} times over {np.unique(ridge['peak_bin']).size} bins")
    assert moves >= 3, "the peak bin moves"
    compare_chirp(got, peaks, si.chirp_reference(nfft, rates), si.scale_sweep_capture(nfft), nfft, rates, f"chirp {nfft} at rate 0")


# ------------------------------------------------------------------------------------------------ 3. kurtosis
@pytest.mark.parametrize("nfft", si.SK_NFFT)
def test_kurtosis_block_hand_over_across_steps(dev, cus, tone, nfft):
    """Rows of three blocks (13, 13 and 11 frames), so that a transform group's next block, its first frame and its
    length change from step to step: next_f0 / next_count of sk_kernel."""
    b, m, rows, nb = si.per_step(nfft), si.SK_M, si.sk_rows(nfft), len(si.SK_BLOCKS)
    nsteps = -(-nb * rows // b)
    grid = many_steps(cus, si.sk_min_waves(nfft), nsteps, f"kurtosis {nfft}")
    assert rows <= gpsjam.sk_rows(tone.nbytes, si.FIRST, nfft, si.SK_HOP, m) and m <= 64
    s1, s2, skv = run_sk(dev, tone, tone.nbytes, nfft, si.SK_HOP, si.FIRST, m, rows)
    r1, r2 = si.sk_reference(nfft)
    e1, e2 = rel(s1, r1, r1.max(axis=1, keepdims=True)), rel(s2, r2, r2.max(axis=1, keepdims=True))
    print(f"kurtosis {nfft}: {rows} rows of {m} frames, S1 {e1:.2e} (tolerance {sr.S1_TOL:.0e}), S2 {e2:.2e} (tolerance {sr.S2_TOL:.0e})")
    assert e1 <= sr.S1_TOL, (nfft, "S1", e1)
    assert e2 <= sr.S2_TOL, (nfft, "S2", e2)
    sr.check_sk(s1, s2, skv, m, (nfft, "many steps"))
    print(f"kurtosis {nfft}: SK within {sr.worst['sk_ulp']:.2f} ulp (the largest of this run so far; tolerance 2)")
    again = run_sk(dev, tone, tone.nbytes, nfft, si.SK_HOP, si.FIRST, m, rows)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(again, (s1, s2, skv))), "the long call repeated"
    second_round = -(-grid * b // nb) + 1
    assert second_round + 8 <= rows - 8
    for k in (second_round, rows - 8):
        assert one_step_each(cus, si.sk_min_waves(nfft), -(-nb * 8 // b))
        piece = run_sk(dev, tone, tone.nbytes, nfft, si.SK_HOP, si.FIRST + k * m * si.SK_HOP, m, 8)
        assert all(x.tobytes() == y[k:k + 8].tobytes() for x, y in zip(piece, (s1, s2, skv))), (nfft, k)


# ------------------------------------------------------------------------------------------------ 4. excisors
def compare_window(body, rec, want, band, what):
    """tests/excise_chirp/test_round6_gpu.py::compare on a window restated from its own bytes: the records of its frames
    and the bytes between its first and its last half frame (those two are edges of the window, not of the call).
    Returns (bytes that differ, bytes in the tie band, bytes)."""
    assert rec.size == want.records.size and body.size == want.hi - want.lo == want.value.size, what
    np.testing.assert_array_equal(rec["n_excised"], want.records["n_excised"], err_msg=str(what))
    assert not rec["reserved"].any()
    tot = want.records["total"]
    errs = {key: float(np.max(np.abs(rec[key] - want.records[key]) / tot)) for key in ("total", "removed")}
    diff = np.abs(body.astype(np.int16) - want.out[want.lo:want.hi].astype(np.int16))
    clear = er.tie_distance(want.value) > band
    share = float(np.mean(~clear))
    print(f"{what}: total {errs['total']:.2e}, removed {errs['removed']:.2e} (tolerance {RTOL:.0e}), {int(np.sum(diff != 0))} of {diff.size} bytes "
          f"differ, {int(np.sum(~clear))} lie in the tie band ({share:.2e}, cap {xr.TIE_SHARE_CAP:.2e})")
    for key, err in errs.items():
        assert err <= RTOL, (what, key, err)
    assert share <= xr.TIE_SHARE_CAP, (what, share)
    assert not diff[clear].any(), (what, int(np.sum(diff[clear] != 0)), "bytes differ outside the tie band")
    assert diff.max(initial=0) <= 1, (what, int(diff.max()))
    return int(np.sum(diff != 0)), int(np.sum(~clear)), diff.size


@pytest.fixture(scope="module")
def excise_cap(dev):
    c = dev.capture(si.scale_excise_capture())
    yield c
    c.free()


@pytest.mark.parametrize("chirp,nfft", si.excise_cases())
def test_excisor_runs_longer_than_four_frames(dev, cus, excise_cap, res, chirp, nfft):
    name = "gj_excise_chirp_dev" if chirp else "gj_excise_dev"
    f, n, h, first, b = si.excise_frames(nfft), si.excise_samples(nfft), nfft // 2, si.EXCISE_FIRST, si.per_step(nfft)
    per = si.excise_per_run(cus, nfft, f)
    assert per >= 5 and per % 4 != 0, (f"{name} {nfft}: {f} frames are sized for runs of five on {si.SIZED_FOR_CUS} CUs; on this device's "
                                       f"{cus} a run holds {per} frames, which the parity tests cover already")
    runs = -(-f // per)
    print(f"{name} {nfft}: {f} frames in {runs} runs of {per}, the last one of {f - (runs - 1) * per}, on {-(-runs // b)} workgroups")
    raw, cap = si.scale_excise_capture(), excise_cap
    assert gpsjam.excise_frames(n, nfft) == f and first + n <= cap.nsamples
    d_thr = res(si.excise_thresholds(nfft))
    d_rate = res(si.excise_chirp_rates(nfft), np.int32) if chirp else None

    def run(first_frame, n_samples, want_frames=True):
        rate = d_rate.ptr + 4 * first_frame if chirp else None
        return run_excise_chirp(dev, cap, cap.nbytes, first + first_frame * h, n_samples, nfft, rate, d_thr, want_frames, plain=not chirp)

    long_b, long_r = run(0, n)
    assert long_r["n_excised"].sum() > 0
    again_b, again_r = run(0, n)
    assert again_b.tobytes() == long_b.tobytes() and again_r.tobytes() == long_r.tobytes(), "the long call repeated"
    no_rec, _ = run(0, n, want_frames=False)
    assert no_rec.tobytes() == long_b.tobytes(), "d_frames = NULL changes no byte"
    assert long_b[:nfft].tobytes() == raw[2 * first:2 * first + nfft].tobytes(), "the first half frame is the input's"
    assert f * nfft < 2 * n and long_b[f * nfft:].tobytes() == raw[2 * first + f * nfft:2 * (first + n)].tobytes(), "the tail is the input's"

    # two overlapping halves with runs of another length: records of every frame, interior bytes of every hop
    covered = np.zeros(f, bool)
    for k, m in si.excise_halves(nfft):
        half_per = si.excise_per_run(cus, nfft, m)
        assert half_per != per and half_per >= si.EXCISE_MIN_RUN, (nfft, per, half_per)
        piece_b, piece_r = run(k, (m - 1) * h + nfft if k == 0 else n - k * h)
        assert piece_r.size == m and piece_r.tobytes() == long_r[k:k + m].tobytes(), (name, nfft, k, "records")
        assert piece_b[nfft:m * nfft].tobytes() == long_b[(k + 1) * nfft:(k + m) * nfft].tobytes(), (name, nfft, k, "interior bytes")
        covered[k + 1:k + m] = True
    assert covered[1:].all(), "every hop [f h, (f + 1) h) of the long call lies inside a half"

    # the float64 restatement on six windows, each from its own input bytes alone
    differ = band = total = 0
    for w in si.excise_windows(nfft):
        want = si.window_reference(nfft, w, chirp)
        body = long_b[(w + 1) * nfft:(w + si.WINDOW_FRAMES) * nfft]
        d, t, s = compare_window(body, long_r[w:w + si.WINDOW_FRAMES], want, si.tie_band(chirp), f"{name} {nfft} frames {w}..{w + si.WINDOW_FRAMES - 1}")
        differ, band, total = differ + d, band + t, total + s
    print(f"{name} {nfft}: over the six windows {differ} of {total} bytes differ, {band} lie in the tie band ({band / total:.2e})")


# ------------------------------------------------------------------------------------------------ 5. past byte 2^32
BIG = 2 ** 32 + 2 ** 20
WINDOW_AT = 2 ** 32 + 2                         # byte offset of the window: sample 2^31 + 1, an odd one
S0 = WINDOW_AT // 2
PAST_NFFT = (64, 4096)


@pytest.fixture(scope="module")
def big(dev):
    """4 GiB + 1 MiB, never filled: only the window that a test uploads is ever read.  An allocation failure fails."""
    b = dev.alloc(BIG)
    assert b.ptr and b.nbytes == BIG
    yield b
    b.free()


def place(big, raw):
    assert WINDOW_AT > 2 ** 32 and S0 > 2 ** 31 and S0 % 2 == 1 and WINDOW_AT + raw.size <= BIG
    big.upload(raw, offset=WINDOW_AT)
    assert big.download(np.uint8, 64, offset=WINDOW_AT).tobytes() == raw[:64].tobytes()


@pytest.mark.parametrize("nfft", PAST_NFFT)
def test_ridge_and_kurtosis_past_byte_2_32(dev, big, nfft):
    raw, s, hop = rr.parity_capture(), 1, nfft // 2 + 37
    place(big, raw)
    with dev.capture(raw) as small:
        want, _ = rr.parity_reference(nfft, hop, s, si.GUARD)
        a = run_ridge(dev, small, small.nbytes, nfft, hop, s, want.size, si.GUARD)
        rr.compare(a, want, (nfft, "the window as a capture of its own"))
        far = run_ridge(dev, big, BIG, nfft, hop, S0 + s, want.size, si.GUARD)
        assert far.tobytes() == a.tobytes(), ("gj_ridge_dev", nfft)
        # kurtosis: M = 5 and a hop that is not nfft / 2
        m, p = 5, sr.parity_powers(nfft, hop, s)
        rows = p.shape[0] // m
        assert rows == gpsjam.sk_rows(small.nbytes, s, nfft, hop, m) >= 1
        near = run_sk(dev, small, small.nbytes, nfft, hop, s, m, rows)
        sr.compare(near, p, m, rows, (nfft, "the window as a capture of its own"))
        far = run_sk(dev, big, BIG, nfft, hop, S0 + s, m, rows)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(far, near)), ("gj_sk_dev", nfft)


@pytest.mark.parametrize("nfft", PAST_NFFT)
def test_chirp_past_byte_2_32(dev, big, nfft):
    raw, s, hop, rates = cr.parity_capture(nfft), 1, cr.parity_hop(nfft), si.RATES
    place(big, raw)
    with dev.capture(raw) as small:
        want = cr.parity_reference(nfft, rates, s)
        n = want.records.size
        a, pa = run_chirp(dev, small, small.nbytes, nfft, hop, s, n, rates)
        cr.compare(a, pa, want, (nfft, "the window as a capture of its own"))
        far, pfar = run_chirp(dev, big, BIG, nfft, hop, S0 + s, n, rates)
        assert far.tobytes() == a.tobytes() and pfar.tobytes() == pa.tobytes(), ("gj_chirp_dev", nfft)


@pytest.mark.parametrize("chirp", [False, True])
@pytest.mark.parametrize("nfft", PAST_NFFT)
def test_excisors_past_byte_2_32(dev, big, res, nfft, chirp):
    name = "gj_excise_chirp_dev" if chirp else "gj_excise_dev"
    raw = xr.parity_capture(nfft) if chirp else er.parity_capture()
    want = xr.parity_reference(nfft) if chirp else er.parity_reference(nfft)
    s = xr.PARITY_FIRST if chirp else er.PARITY_FIRST
    n = raw.size // 2 - s
    d_thr = res(er.parity_threshold(nfft))
    d_rate = res(xr.parity_rates(nfft), np.int32) if chirp else None
    place(big, raw)
    with dev.capture(raw) as small:
        near_b, near_r = run_excise_chirp(dev, small, small.nbytes, s, n, nfft, d_rate, d_thr, plain=not chirp)
        (xr if chirp else er).compare(near_b, near_r, want, (name, nfft, "the window as a capture of its own"))
    far_b, far_r = run_excise_chirp(dev, big, BIG, S0 + s, n, nfft, d_rate, d_thr, plain=not chirp)
    assert far_b.tobytes() == near_b.tobytes() and far_r.tobytes() == near_r.tobytes(), (name, nfft)
    # one sample past the buffer's end: refused, nothing written
    out, rec = Guarded(dev, 2 * n), Guarded(dev, near_r.size * gpsjam.EXCISE_DTYPE.itemsize)
    try:
        total = BIG // 2

        def launch(first):
            if chirp:
                dev.excise_chirp_dev(big, BIG, first, n, nfft, d_rate, d_thr, out, rec)
            else:
                dev.excise_dev(big, BIG, first, n, nfft, d_thr, out, rec)
        refused(dev, launch, [((first,), GJ_ERR_INVALID) for first in (total - n + 1, total)], out, rec)
    finally:
        freed(out, rec)
