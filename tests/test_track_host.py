"""The tracking loops on the CPU: the restatement (tests/track_restatement.py) against the header and against itself,
and the loop's behaviour on a capture with a Doppler ramp.  No GPU: tests/track/test_round6_gpu.py holds the kernel to
every bit of this restatement."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import corr_restatement as cr
import gpsjam
import track_restatement as tr
from gpsjam import _ffi, postcorr, track

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(REPO, "include", "gpsjam.h")).read()


def header_define(name):
    return re.search(r"#define\s+%s\s+(.+?)(?:/\*|\n(?!\s*[0-9]))" % name, HEADER, re.S).group(1)


# ------------------------------------------------------------------------------------------------ 1. the header
def test_header_constants_structs_and_version():
    table = [int(v) for v in re.findall(r"-?\d+", header_define("GJ_TRACK_ATAN_TABLE").replace("\\", " "))]
    assert tuple(table) == tr.ATAN == _ffi.GJ_TRACK_ATAN_TABLE and len(table) == 16
    assert sum(table) == tr.ANGLE_BOUND == 1191629338
    for name, want in (("GJ_TRACK_MAX_CHANNELS", tr.MAX_CHANNELS), ("GJ_TRACK_MAX_EPOCHS", tr.MAX_EPOCHS), ("GJ_TRACK_MAX_GAIN", tr.MAX_GAIN),
                       ("GJ_TRACK_PLL_SHIFT", tr.PLL_SHIFT), ("GJ_TRACK_DLL_SHIFT", tr.DLL_SHIFT)):
        assert eval(header_define(name).strip().strip("()")) == want == getattr(_ffi, name), name
    assert C.sizeof(_ffi.TrackState) == gpsjam.TRACK_STATE_DTYPE.itemsize == 64
    assert C.sizeof(_ffi.TrackParams) == 32
    assert C.sizeof(_ffi.TrackEpoch) == gpsjam.TRACK_EPOCH_DTYPE.itemsize == 56
    for struct, dtype in ((_ffi.TrackState, gpsjam.TRACK_STATE_DTYPE), (_ffi.TrackEpoch, gpsjam.TRACK_EPOCH_DTYPE)):
        for name, _ in struct._fields_:
            assert getattr(struct, name).offset == dtype.fields[name][1], name
    assert _ffi.GJ_VERSION == 150 and re.search(r"#define\s+GJ_VERSION\s+150\b", HEADER)


def test_gains_are_the_restatement_and_inside_the_bound():
    for bands in (track.WIDE, track.NARROW, tr.WIDE, tr.NARROW):
        for B, fs in ((2048, 2.048e6), (4096, 4.096e6), (16, 2.048e6)):
            p = track.gains(*bands, B, fs, spacing=3, aid_div=77)
            got = (p.spacing, p.aid_div, p.pll_p, p.pll_i, p.fll, p.dll_p, p.dll_i)
            assert got == tr.gains(*bands, B, fs, 3, 77) and p.reserved == 0
            assert all(abs(g) <= tr.MAX_GAIN for g in got[2:])
    assert track.WIDE == tr.WIDE == (30, 200, 5) and track.NARROW == tr.NARROW == (20, 50, 2)


# ------------------------------------------------------------------------------------------------ 2. brute == track
EDGE_PARAMS = (1, 1540, 335703, 13438, 10541, 7161655, 47781)


def edge_states(n, starts=(0, 1, 5)):
    return [tr.state(ch, starts[k % len(starts)]) for k, ch in enumerate(cr.parity_channels(n))]


@pytest.mark.parametrize("B", [16, 48])
def test_brute_is_track(B):
    raw, codes = cr.parity_capture(), cr.parity_codes()
    for n_epochs in (1, 2, 3):
        for params in (EDGE_PARAMS, (2, 0, 0, 0, 0, 0, 0), (64, 1, -tr.MAX_GAIN, tr.MAX_GAIN, -tr.MAX_GAIN, tr.MAX_GAIN, -tr.MAX_GAIN)):
            n = 3 * B + 5
            a = tr.brute(raw, 7, n, B, n_epochs, codes, edge_states(6), params)
            b = tr.track(raw, 7, n, B, n_epochs, codes, edge_states(6), params)
            assert a == b, (B, n_epochs, params)
            assert all(len(r) == n_epochs for r in a[0]) and all(s[7] == t[7] + n_epochs * B for s, t in zip(a[1], edge_states(6)))


# ------------------------------------------------------------------------------------------------ 3. the CORDIC
def test_cordic_against_atan2():
    rng = np.random.default_rng(5)
    bound = cr.RECORD_BOUND
    v = rng.integers(-bound, bound + 1, (100000, 2))
    v[:50000] = np.round(v[:50000] * 10.0 ** rng.uniform(-4.5, 0.0, (50000, 1)))        # every magnitude down to |v| of about 1000
    axes = [(s * m, 0) for s in (1, -1) for m in (1, 1000, bound)] + [(0, s * m) for s in (1, -1) for m in (1, 1000, bound)]
    assert tr.cordic(0, 0) == (0, 0)
    worst_angle, worst_length, lo, hi = 0.0, 0.0, math.inf, 0.0
    for I, Q in [tuple(int(x) for x in row) for row in v] + axes + [(bound, bound), (-bound, -bound), (bound, -bound), (-bound, bound)]:
        angle, length = tr.cordic(I, Q)
        assert abs(angle) <= tr.ANGLE_BOUND and 0 <= length < 2 ** 34
        r = math.hypot(I, Q)
        if r < 1000.0:
            continue
        x, y = (-I, -Q) if I < 0 else (I, Q)
        worst_angle = max(worst_angle, abs(angle / 2.0 ** 32 - math.atan2(y, x) / (2.0 * math.pi)))
        lo, hi = min(lo, length / (256.0 * r)), max(hi, length / (256.0 * r))
        worst_length = max(worst_length, abs(length / (256.0 * tr.CORDIC_GAIN * r) - 1.0))
    print(f"cordic: largest angle error {worst_angle:.3e} cycle (recorded {tr.CORDIC_ERROR_ANGLE:.3e}), largest length error "
          f"{worst_length:.3e} (recorded {tr.CORDIC_ERROR_LENGTH:.3e}), gain {lo:.5f} .. {hi:.5f}")
    assert worst_angle == pytest.approx(tr.CORDIC_ERROR_ANGLE, rel=0.1)
    assert worst_length == pytest.approx(tr.CORDIC_ERROR_LENGTH, rel=0.1)


# ------------------------------------------------------------------------------------------------ 4. zero gains: the bank
@pytest.mark.parametrize("d", [1, 64])
def test_zero_gains_reproduce_the_bank(d):
    raw, codes, channels = cr.parity_capture(), cr.parity_codes(), cr.parity_channels(6)
    B, n_epochs = 272, 5
    rec, after = tr.track(raw, 7, n_epochs * B, B, n_epochs, codes, [tr.state(ch) for ch in channels], (d, 0, 0, 0, 0, 0, 0))
    want = cr.bank(raw, 7, n_epochs * B, B, codes, channels, (d, 0, -d))
    assert np.array_equal(tr.as_array(rec)[:, :, :6].reshape(6, n_epochs, 3, 2), want)
    for s, ch in zip(after, channels):
        assert s[:6] == tuple(postcorr.advance(postcorr.Channel(*ch), n_epochs * B)) and s[6] == 0 and s[7] == n_epochs * B and s[10] == 1


# ------------------------------------------------------------------------------------------------ 5. chaining
def test_n_plus_m_epochs_are_n_then_m():
    raw, codes = cr.parity_capture(), cr.parity_codes()
    B, N, M, n = 48, 5, 7, 12 * 48 + 5
    whole, after = tr.track(raw, 3, n, B, N + M, codes, edge_states(6), EDGE_PARAMS)
    first, mid = tr.track(raw, 3, n, B, N, codes, edge_states(6), EDGE_PARAMS)
    second, end = tr.track(raw, 3, n, B, M, codes, mid, EDGE_PARAMS)
    assert [a + b for a, b in zip(first, second)] == whole and end == after


# ------------------------------------------------------------------------------------------------ 6. the clamps
def test_extreme_gains_stay_inside_the_bounds():
    raw, codes = cr.parity_capture(), cr.parity_codes()
    G = tr.MAX_GAIN
    low = high = wrapped = False
    for params in ((1, 1, G, G, G, G, G), (1, 1, -G, -G, -G, -G, -G), (64, 1540, G, -G, G, -G, G), (1, 0, -G, G, -G, G, -G)):
        rec, after = tr.track(raw, 0, cr.PARITY_SAMPLES, 16, 97, codes, edge_states(6), params)
        a = tr.as_array(rec)
        assert a[..., 9].min() >= 0 and a[..., 9].max() <= cr.MAX_CODE_STEP - 1 and a[..., 8].max() < cr.PERIOD
        assert a[..., 7].min() >= 0 and a[..., 7].max() < 2 ** 32 and np.abs(a[..., 10]).max() <= tr.ANGLE_BOUND and np.abs(a[..., 11]).max() <= 65536
        low, high = low or bool((a[..., 9] == 0).any()), high or bool((a[..., 9] == cr.MAX_CODE_STEP - 1).any())
        step = a[..., 7]
        wrapped = wrapped or bool((np.abs(np.diff(step, axis=1)) > 2 ** 31).any())
        assert not any(tr.state_bad(s, 4, 1, 16, cr.PARITY_SAMPLES) for s in after)
    assert low and high and wrapped, (low, high, wrapped)


def test_bad_channels_are_left_alone():
    raw, codes = cr.parity_capture(), cr.parity_codes()
    good = edge_states(3)
    for bad in tr.bad_states(good[1], 4, 3, 48, 200):
        rec, after = tr.track(raw, 0, 200, 48, 3, codes, [good[0], bad, good[2]], EDGE_PARAMS)
        assert rec[1] is None and after[1] == bad and rec[0] is not None and rec[2] is not None


# ------------------------------------------------------------------------------------------------ 7. the loop
def test_loop_follows_a_doppler_ramp():
    """1200 epochs of PRN 9 at 45 dB-Hz from the acquisition grid (73 Hz off, 0.19 sample off) under 50 Hz/s: 200 epochs
    WIDE, 1000 NARROW; the figures over the last 1000 against the recorded ones, and against the open-loop bank."""
    rec, after = tr.loop_track()
    rms, lock, cn0 = tr.loop_figures(rec)
    open_cn0 = postcorr.cn0(tr.loop_open()[-tr.LOOP_WINDOW:], tr.LOOP_B / cr.FS)
    open_prompts = tr.loop_open()[-tr.LOOP_WINDOW:]
    open_lock = float(np.abs(open_prompts.real).sum() / np.abs(open_prompts).sum())
    print(f"loop: Doppler rms error {rms:.3f} Hz (recorded {tr.LOOP_CPU_DOPPLER_RMS}), lock {lock:.4f} ({tr.LOOP_CPU_LOCK}), tracked C/N0 "
          f"{cn0:.2f} dB-Hz ({tr.LOOP_CPU_CN0_TRACKED}), open-loop C/N0 {open_cn0:.2f} dB-Hz ({tr.LOOP_CPU_CN0_OPEN}), open-loop lock {open_lock:.4f}")
    assert rms == pytest.approx(tr.LOOP_CPU_DOPPLER_RMS, rel=0.1)
    assert lock == pytest.approx(tr.LOOP_CPU_LOCK, rel=0.1)
    assert cn0 == pytest.approx(tr.LOOP_CPU_CN0_TRACKED, rel=0.1)
    assert open_cn0 == pytest.approx(tr.LOOP_CPU_CN0_OPEN, rel=0.1)
    assert tr.LOOP_CPU_CN0_TRACKED > tr.LOOP_CPU_CN0_OPEN
    assert cn0 - open_cn0 >= 0.5 * (tr.LOOP_CPU_CN0_TRACKED - tr.LOOP_CPU_CN0_OPEN)
    assert lock > 0.9 > 0.7 > open_lock, "phase lock is what the open loop cannot have"
    assert after[7] == tr.LOOP_START + tr.LOOP_EPOCHS * tr.LOOP_B and not tr.state_bad(after, 1, 1, 16, tr.LOOP_SAMPLES + 16)
