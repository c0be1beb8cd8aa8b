"""CPU side of the scale tests of the short-time kernels (tests/stft_scale/test_round6_gpu.py): the arithmetic of their
geometries -- the frames fit the captures, 1541 steps are uneven for both grid sizes of a 256-CU device, 2048 B + 1 frames
give the excisors runs of five -- and the conditions on their inputs that the GPU comparisons rely on: no ridge frame with
a nearly tied peak, few chirp frames with a nearly tied rate or bin (and none on which a float32 evaluation picks
otherwise), no bin of a restated excisor window near its threshold.  No GPU call is made; what runs here is the yardstick
(tests/stft_scale_inputs.py on the existing restatements), not the library."""
import numpy as np
import pytest

import chirp_restatement as cr
import excise_chirp_restatement as xr
import excise_restatement as er
import gpsjam
import ridge_restatement as rr
import skurt_restatement as sr
import stft_scale_inputs as si


# ------------------------------------------------------------------------------------------------ geometry
def test_frames_rows_and_runs_fit_the_captures():
    tone = si.scale_tone_capture()
    assert tone.size == 2 << 19
    for nfft in rr.PARITY_NFFT:
        b, n, hop = si.per_step(nfft), si.scale_frames(nfft), si.scale_hop(nfft)
        assert -(-n // b) == si.STEPS and (n % b != 0) == (b > 1), "STEPS steps, the last one part-filled wherever B > 1"
        assert gpsjam.ridge_frames(tone.size, si.FIRST, nfft, hop) >= n == rr.frames_that_fit(2 * (si.FIRST + (n - 1) * hop + nfft), si.FIRST, nfft, hop)
    for nfft in si.CHIRP_NFFT:
        n, hop, nbytes = si.scale_frames(nfft), si.scale_hop(nfft), 2 * si.sweep_samples(nfft)
        assert si.sweep_samples(nfft) <= 1 << 19
        # exactly all that fit: the last frame ends on the capture's last byte
        assert gpsjam.ridge_frames(nbytes, si.FIRST, nfft, hop) == n and gpsjam.ridge_frames(nbytes - 2, si.FIRST, nfft, hop) == n - 1
    for nfft in si.SK_NFFT:
        rows, b = si.sk_rows(nfft), si.per_step(nfft)
        assert rows == {4096: 514, 1024: 2055, 256: 8219}[nfft]
        assert gpsjam.sk_rows(tone.size, si.FIRST, nfft, si.SK_HOP, si.SK_M) >= rows == sr.rows_that_fit(
            2 * (si.FIRST + (rows * si.SK_M - 1) * si.SK_HOP + nfft), si.FIRST, nfft, si.SK_HOP, si.SK_M)
        assert len(si.SK_BLOCKS) * rows >= si.STEPS * b > len(si.SK_BLOCKS) * (rows - 1)
    # the kernel's partition of a row (stft_rows.h row_blocks): ceil(M / 16) blocks of ceil(M / blocks) frames, a short last one
    nb = -(-si.SK_M // sr.MAX_RUN)
    run = -(-si.SK_M // nb)
    assert (nb, run) == (3, 13) and si.SK_BLOCKS == (run, run, si.SK_M - 2 * run) and 0 < si.SK_BLOCKS[-1] < run
    raw = si.scale_excise_capture()
    assert raw.size == 2 * si.EXCISE_SAMPLES <= 8.4e6
    for chirp, nfft in si.excise_cases():
        f, n, h = si.excise_frames(nfft), si.excise_samples(nfft), nfft // 2
        assert f == 4 * si.SIZED_FOR_CUS * si.EXCISE_MIN_WAVES * si.per_step(nfft) + 1
        assert gpsjam.excise_frames(n, nfft) == f == er.frames_loop(n, nfft) and gpsjam.excise_frames(n - (h // 2 + 2), nfft) == f - 1
        assert n - f * h > h, "a tail behind the last whole hop and the last frame's second half are copied"
        assert si.EXCISE_FIRST + n <= si.EXCISE_SAMPLES
        if chirp:
            assert si.excise_chirp_rates(nfft).size == f and len(set(si.excise_chirp_rates(nfft)[:8].tolist())) == 8


def test_1541_steps_are_uneven_for_both_grid_sizes():
    cus = si.SIZED_FOR_CUS
    assert si.STEPS > 2 * 3 * cus
    assert si.one_round(cus, 2, si.STEPS) == (386, 4, 3) and si.one_round(cus, 3, si.STEPS) == (514, 3, 2)
    for nfft in rr.PARITY_NFFT:
        grid, most, fewest = si.one_round(cus, si.ridge_min_waves(nfft), si.STEPS)
        assert most >= 3 and fewest == most - 1 and grid <= cus * si.ridge_min_waves(nfft)
    for nfft in si.CHIRP_NFFT:
        grid, most, fewest = si.one_round(cus, si.chirp_min_waves(nfft), si.STEPS)
        assert most >= 3 and fewest == most - 1
    for nfft in si.SK_NFFT:
        # the rows are whole, so the kurtosis takes one step more: 1542, uneven at 512 slots (1024 and 4096 points) and
        # three steps for every workgroup at 768 (256 points)
        nsteps = -(-len(si.SK_BLOCKS) * si.sk_rows(nfft) // si.per_step(nfft))
        assert nsteps == si.STEPS + 1
        grid, most, fewest = si.one_round(cus, si.sk_min_waves(nfft), nsteps)
        assert (grid, most, fewest) == ((514, 3, 3) if nfft == 256 else (386, 4, 3))
    # fewer CUs keep the regime (more steps per workgroup); a one-round grid never exceeds its steps
    for c in (1, 64, 128, 255, 256):
        for mw in (2, 3):
            grid, most, fewest = si.one_round(c, mw, si.STEPS)
            assert most >= 3 and grid <= si.STEPS and grid * most >= si.STEPS > grid * (most - 1)


def test_2048_b_plus_1_frames_give_runs_of_five():
    for chirp, nfft in si.excise_cases():
        f, b = si.excise_frames(nfft), si.per_step(nfft)
        per = si.excise_per_run(si.SIZED_FOR_CUS, nfft, f)
        assert per == 5 and f % per != 0, "runs of five with a short last run"
        for c in (64, 128, 255):                            # fewer CUs: longer runs, still no multiple of four
            assert si.excise_per_run(c, nfft, f) >= 5 and si.excise_per_run(c, nfft, f) % 4 != 0
        assert si.excise_per_run(2 * si.SIZED_FOR_CUS, nfft, f) == 4, "more CUs fall back to runs of four: the GPU test fails there"
        (a0, an), (b0, bn) = si.excise_halves(nfft)
        assert a0 == 0 and b0 + bn == f and a0 + an - b0 == 4, "the halves overlap by four frames"
        for n in (an, bn):
            assert n <= 4 * si.SIZED_FOR_CUS * si.EXCISE_MIN_WAVES * b and si.excise_per_run(si.SIZED_FOR_CUS, nfft, n) == 4
        # Seams of the long call lie at multiples of 5, those of a half at multiples of 4 from its start.  Three seams in
        # four of the long call fall inside a run of the half that holds them (a carry primed there against a carry handed
        # over); every 20th frame is a seam of both, which the parity tests' runs of four already tie to the restatement.
        seams = list(range(5, f, 5))
        inside = [s for s in seams if (s < an and s % 4 != 0) or (s > b0 and (s - b0) % 4 != 0)]
        assert len(inside) >= 0.74 * len(seams) and len(seams) >= 400
        ws = si.excise_windows(nfft)
        assert len(ws) == 6 == len(set(ws)) and ws[0] == 0 and ws[-1] + si.WINDOW_FRAMES == f
        assert all(0 <= w <= f - si.WINDOW_FRAMES for w in ws)
        assert ws[1] < 5 * b < ws[1] + si.WINDOW_FRAMES - 1, "the seam between the first two workgroups lies inside the window"
        assert ws[3] < f // 2 < ws[3] + si.WINDOW_FRAMES


# ------------------------------------------------------------------------------------------------ conditions on the inputs
def test_no_ridge_frame_of_the_tone_capture_has_a_nearly_tied_peak():
    """tests/stft_scale holds gj_ridge_dev to the restatement's peak_bin on EVERY frame of 1541 steps."""
    smallest = {}
    for nfft in rr.PARITY_NFFT:
        rec, margin = si.ridge_reference(nfft)
        assert rec.size == si.scale_frames(nfft)
        smallest[nfft] = float(margin.min())
    print("smallest peak margin per size:", {k: round(v, 3) for k, v in smallest.items()})
    assert min(smallest.values()) >= rr.NEAR_TIE, smallest
    assert min(smallest.values()) >= 0.9 * si.RIDGE_MARGIN_MEASURED, "the figure written beside the inputs"


@pytest.mark.parametrize("nfft", si.CHIRP_NFFT)
def test_few_chirp_frames_are_nearly_tied_and_float32_agrees_on_all_others(nfft):
    """The GPU test compares rate_index and peak_bin exactly on the clear frames and holds the others to a choice among
    the nearly tied candidates.  Fair only if the others are few (SCALE_TIE_SHARE_CAP) and float32 arithmetic, which the
    kernel has, picks the float64 answer on every clear frame."""
    assert si.SCALE_TIE_SHARE_CAP == 2 * max(si.SCALE_TIE_SHARE_MEASURED.values())
    a, b = si.chirp_reference(nfft), si.chirp_reference(nfft, single=True)
    clear = si.clear_frames(a)
    assert clear.size == si.scale_frames(nfft) and a.peaks.shape == (clear.size, si.RATES[2])
    share = 1.0 - float(clear.mean())
    disagree = int(np.sum(((a.records["rate_index"] != b.records["rate_index"]) | (a.records["peak_bin"] != b.records["peak_bin"]))[clear]))
    errs = {k: float(np.max((np.abs(a.records[k] - b.records[k]) / a.records[k])[clear])) for k in ("total", "peak")}
    errs["peaks"] = float(np.max(np.abs(a.peaks - b.peaks) / a.peaks))
    print(f"nfft {nfft}: {clear.size} frames, share not clear {share:.2e} (cap {si.SCALE_TIE_SHARE_CAP:.1e}), float32 disagrees on "
          f"{disagree} clear frames, float32 errors {errs}")
    assert share <= si.SCALE_TIE_SHARE_CAP
    assert disagree == 0
    assert max(errs.values()) <= cr.RTOL / 10.0, errs
    # chirp_spectrum, which the GPU test consults on the frames that are not clear, is the restatement's own spectrum
    x, hop, qs = rr.unpack(si.scale_sweep_capture(nfft)), si.scale_hop(nfft), cr.rate_values(si.RATES)
    for f in (0, clear.size // 2, clear.size - 1, *np.flatnonzero(~clear)[:3]):
        r = int(a.records["rate_index"][f])
        p = si.chirp_spectrum(x, nfft, si.FIRST + int(f) * hop, qs[r])
        assert p.max() == a.records["peak"][f] == a.peaks[f, r] and int(np.argmax(p)) == a.records["peak_bin"][f]
    if nfft in si.CHIRP_RIDGE_NFFT:                         # the single rate 0, which the GPU test holds against gj_ridge_dev
        zero = si.chirp_reference(nfft, (0, 1, 1))
        share0 = 1.0 - float(si.clear_frames(zero).mean())
        print(f"nfft {nfft}: at the single rate 0 the share not clear is {share0:.2e}")
        assert share0 <= si.SCALE_TIE_SHARE_CAP and np.all(zero.rate_margin == 1.0)


def test_no_bin_of_an_excisor_window_is_near_its_threshold():
    """The GPU test restates six windows of 24 frames per size in float64 and holds the kernels to the mask on EVERY bin
    and to the bytes outside the rounding-tie band."""
    margin, share = {}, {}
    for chirp, nfft in si.excise_cases():
        thr = si.excise_thresholds(nfft)
        cut = 0
        for w in si.excise_windows(nfft):
            ref = si.window_reference(nfft, w, chirp)
            assert ref.records.size == si.WINDOW_FRAMES and ref.value.size == (si.WINDOW_FRAMES - 1) * nfft
            margin[(chirp, nfft, w)] = er.threshold_margin(ref.power, thr)
            share[(chirp, nfft, w)] = float(np.mean(er.tie_distance(ref.value) <= si.tie_band(chirp)))
            cut += int(ref.records["n_excised"].sum())
        assert cut > 0, "every case must excise something"
    print(f"seed {si.EXCISE_SEED}: smallest threshold margin {min(margin.values()):.4e}, largest tie-band share of a window "
          f"{max(share.values()):.2e} (cap {xr.TIE_SHARE_CAP:.2e})")
    assert min(margin.values()) >= er.NEAR_TIE, margin
    assert min(margin.values()) >= 0.99 * si.EXCISE_MARGIN_MEASURED, "the figure written beside the seed"
    assert max(share.values()) <= xr.TIE_SHARE_CAP, share
