"""CPU side of the subtraction of tracked signals (gj_subtract_track_dev, Device.subtract_tracked,
gpsjam.track.amplitudes): the interface, the integer restatement the GPU tests compare with
(tests/subtract_track_restatement.py) checked against a per-sample Python-int loop and against the definition's own
consequences, and the end-to-end figures on restated integers, which set the tolerances of the GPU test.  No GPU call
is made.

The float chain is not restated anywhere: gpsjam.track.amplitudes itself runs here, on restated integers."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import corr_restatement as cr
import gpsjam
import subtract_restatement as sr
import subtract_track_restatement as st
import track_restatement as tr
from gpsjam import _ffi, mitigate, postcorr, spoof, track

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gpsjam.h")


# ------------------------------------------------------------------------------------------------ interface
def test_symbols_bindings_and_python_interface():
    lib = _ffi.load()
    assert callable(lib.gj_subtract_track_dev) and len(_ffi.SIGNATURES["gj_subtract_track_dev"][1]) == 17
    assert _ffi.GJ_VERSION == 150 == lib.gj_version()
    assert C.sizeof(_ffi.SubtractTrackChannel) == 8 == gpsjam.SUB_TRACK_CHANNEL_DTYPE.itemsize
    assert [f[0] for f in _ffi.SubtractTrackChannel._fields_] == list(gpsjam.SUB_TRACK_CHANNEL_DTYPE.names) == ["start", "code_row"]
    assert "SUB_TRACK_CHANNEL_DTYPE" in gpsjam.__all__
    for name in ("subtract_tracked", "subtract_track_dev"):
        assert callable(getattr(gpsjam.Device, name))
    assert callable(track.amplitudes) and callable(spoof.remove_tracked)
    import inspect
    assert inspect.signature(mitigate.clean_spoofed).parameters["tracked"].default is False
    text = open(HEADER).read()
    assert re.search(r"typedef struct gj_subtract_track_channel\s*\{[^}]*uint32_t start;[^}]*int32_t\s+code_row;", text)
    # the four fields the call reads are 24 bytes at offset 24 of a 56-byte record
    E = gpsjam.TRACK_EPOCH_DTYPE
    assert E.itemsize == 56 and [E.fields[f][1] for f in ("carr_phase", "carr_step", "code_phase", "code_step")] == [24, 28, 32, 40]


# ------------------------------------------------------------------------------------------------ the restatement
def small_input(seed, n_samples=700):
    rng = np.random.default_rng(seed)
    raw = rng.integers(0, 256, 2 * n_samples).astype(np.uint8)
    raw[:8] = (0, 0, 255, 255, 0, 255, 255, 0)
    return raw


class FarSlice:
    """A capture of which only the bytes from sample ``origin`` on exist: indexing and slicing by absolute byte."""

    def __init__(self, data, origin):
        self.data, self.at = data, 2 * origin

    def __getitem__(self, key):
        if isinstance(key, slice):
            assert key.start >= self.at and key.step is None
            return self.data[key.start - self.at:key.stop - self.at]
        assert key >= self.at
        return self.data[key - self.at]


@pytest.mark.parametrize("B", [16, 48])
def test_restatement_equals_the_python_int_loop(B):
    raw, codes = small_input(B), cr.parity_codes()
    channels = [(0, 0), (1, 1), (15, 1), (16, 2), (B - 1, 3), (B, 0), (3 * B + 7, 2), (2, 3)]
    for first, n, E in ((0, B, 1), (3, B + 15, 1), (1, 2 * B - 1, 1), (0, 4 * B + 7, 1), (5, 6 * B + 5, 2), (2, 10 * B + 9, 6)):
        table = [c for c in channels if c[0] + E * B <= n]
        for bound, flags, seed in ((2 ** 14, 0, 0), (2 ** 14, 1, 0), (2 ** 19, 1, 0xDEADBEEF), (2 ** 22, 0, 5)):
            rec = st.random_records(len(table), E, seed=n)
            amps = sr.random_amps(len(table), E, bound, seed=n)
            got, blk = st.subtract_tracked(raw, first, n, B, E, codes, table, rec, amps, flags, seed)
            want, wblk = st.brute(raw, first, n, B, E, codes, table, rec, amps, flags, seed)
            assert got.tolist() == want and [tuple(int(v) for v in r)[:3] for r in blk] == wblk, (first, n, E, bound, flags)
            assert not blk["reserved"].any()


def test_a_first_sample_above_2_31_and_the_window():
    """The dither's key is 64 bits wide: the same bytes from sample 2^31 + 1 give other bytes than from sample 1; and a
    window of the range is the whole range's bytes and records there."""
    codes, B, E = cr.parity_codes(), 48, 3
    data = small_input(77, 200)
    table = [(5, 1), (31, 2)]
    rec, amps = st.random_records(2, E), sr.random_amps(2, E, 2 ** 15)
    far = 2 ** 31 + 1
    got, blk = st.subtract_tracked(FarSlice(data, far), far, 200, B, E, codes, table, rec, amps, sr.DITHER, 9)
    want, wblk = st.brute(FarSlice(data, far), far, 200, B, E, codes, table, rec, amps, sr.DITHER, 9)
    assert got.tolist() == want and [tuple(int(v) for v in r)[:3] for r in blk] == wblk
    near, _ = st.subtract_tracked(FarSlice(data, 1), 1, 200, B, E, codes, table, rec, amps, sr.DITHER, 9)
    assert near.tobytes() != got.tobytes(), "the upper word of the key is seen"
    raw = cr.parity_capture()
    n, E = 3 * 4096 + 5, 4
    rec, amps = st.random_records(2, E, seed=1), sr.random_amps(2, E, 2 ** 15, seed=1)
    table = [(4095, 0), (17, 3)]
    whole, wblk = st.subtract_tracked(raw, 7, n, 2048, E, codes, table, rec, amps, sr.DITHER, 3)
    for lo, hi in ((0, 4096), (4096, 3 * 4096), (2 * 4096, n)):
        part, pblk = st.subtract_tracked(raw, 7, n, 2048, E, codes, table, rec, amps, sr.DITHER, 3, window=(lo, hi))
        assert part.tobytes() == whole[2 * lo:2 * hi].tobytes() and pblk.tobytes() == wblk[lo // 4096:-(-hi // 4096)].tobytes(), (lo, hi)


@pytest.mark.parametrize("B", [16, 48, 2048])
def test_advanced_records_are_the_subtraction_with_that_channel(B):
    """Records that are one constant channel advanced by m B per epoch, start 0, n = E B: gj_subtract_dev's bytes and
    records with that channel and the same amplitudes."""
    raw, codes, channels = cr.parity_capture(), cr.parity_codes(), cr.parity_channels(6, seed=B)
    E = min(cr.PARITY_SAMPLES // B, 300)
    n = E * B
    rec = np.stack([st.advanced_records(c, E, B) for c in channels])
    amps = sr.random_amps(6, E, 2 ** 15, seed=B)
    for first, flags, seed in ((0, 0, 0), (7, 1, 0xC0FFEE11)):
        got, blk = st.subtract_tracked(raw, first, n, B, E, codes, [(0, c[4]) for c in channels], rec, amps, flags, seed)
        want, wblk = sr.subtract(raw, first, n, B, codes, channels, amps, flags, seed)
        assert got.tobytes() == want.tobytes() and blk.tobytes() == wblk.tobytes(), (first, flags)


def test_zero_amplitudes_and_silent_channels_are_the_identity():
    raw, codes = cr.parity_capture(), cr.parity_codes()
    n, B, E = 2 * 4096 + 77, 256, 4
    rec = st.random_records(3, E)
    for flags, seed in ((0, 0), (1, 12345)):
        got, blk = st.subtract_tracked(raw, 3, n, B, E, codes, [(0, 0), (17, 1), (n - E * B, 2)], rec, np.zeros((3, E, 2), np.int32), flags, seed)
        assert got.tobytes() == raw[6:6 + 2 * n].tobytes() and not blk["removed"].any() and not blk["n_clipped"].any()
        bad = rec.copy()
        bad["code_phase"][:, ::2], bad["code_step"][:, 1::2] = cr.PERIOD, cr.MAX_CODE_STEP
        got, blk = st.subtract_tracked(raw, 3, n, B, E, codes, [(0, 0), (17, 1), (n - E * B, 2)], bad, sr.random_amps(3, E, 2 ** 19), flags, seed)
        assert got.tobytes() == raw[6:6 + 2 * n].tobytes() and not blk["removed"].any(), "every record is bad: every channel is silent"


def test_a_bad_record_is_its_epochs_amplitude_zero():
    raw, codes = cr.parity_capture(), cr.parity_codes()
    n, B, E = 4096 + 300, 48, 80
    table = [(0, 0), (13, 1), (n - E * B, 3)]
    rec, amps = st.random_records(3, E), sr.random_amps(3, E, 2 ** 16)
    bad, zeroed = rec.copy(), amps.copy()
    for ch, m, field, value in ((0, 0, "code_phase", cr.PERIOD), (0, 7, "code_step", cr.MAX_CODE_STEP), (1, 79, "code_phase", 2 ** 64 - 1),
                                (2, 40, "code_step", 2 ** 63), (2, 41, "code_phase", cr.PERIOD + 5)):
        bad[ch, m][field] = value
        zeroed[ch, m] = 0
    got, blk = st.subtract_tracked(raw, 1, n, B, E, codes, table, bad, amps, sr.DITHER, 4)
    want, wblk = st.subtract_tracked(raw, 1, n, B, E, codes, table, rec, zeroed, sr.DITHER, 4)
    assert got.tobytes() == want.tobytes() and blk.tobytes() == wblk.tobytes()
    assert got.tobytes() != st.subtract_tracked(raw, 1, n, B, E, codes, table, rec, amps, sr.DITHER, 4)[0].tobytes()
    small = slice(0, 2 * (13 + 3 * B))
    assert st.brute(raw, 1, 13 + 3 * B, B, 3, codes, table[:2], bad[:2, :3], amps[:2, :3], sr.DITHER, 4)[0] == \
        st.subtract_tracked(raw, 1, 13 + 3 * B, B, 3, codes, table[:2], bad[:2, :3], amps[:2, :3], sr.DITHER, 4)[0][small].tolist()
    assert st.table_bad(codes, [(0, 4)], 1, 16, 16) and st.table_bad(codes, [(0, -1)], 1, 16, 16) and st.table_bad(codes, [(1, 0)], 1, 16, 16)
    assert not st.table_bad(codes, [(0, 3)], 1, 16, 16)


# ------------------------------------------------------------------------------------------------ the amplitudes
def test_amplitudes_null_each_epochs_own_prompt_on_noiseless_bytes():
    """A noiseless signal whose NCOs change from epoch to epoch, correlated epoch by epoch at exactly those NCOs: the
    amplitudes made of the prompts take the signal out, and every epoch's prompt falls to the rounding's share."""
    B, E, start = 2048, 12, 100
    rng = np.random.default_rng(31)
    codes = postcorr.codes([5])
    rec = np.zeros((1, E), gpsjam.TRACK_EPOCH_DTYPE)
    ch = postcorr.channel(0, 200.0, 1500.0, cr.FS, 0.3)
    z = np.zeros(start + E * B + 50, np.complex128)
    for m in range(E):
        rec[0, m]["code_phase"], rec[0, m]["code_step"], rec[0, m]["carr_phase"], rec[0, m]["carr_step"] = ch[:4]
        u = np.arange(B, dtype=np.int64)
        chip = cr.chip_index(ch.code_phase, ch.code_step, u)
        theta = ((ch.carr_phase + u * ch.carr_step) & 0xFFFFFFFF) / 2.0 ** 32
        z[start + m * B:start + (m + 1) * B] = 40.0 * codes[0][chip] * np.exp(-2j * np.pi * theta + 0.4j) * (-1) ** (m // 5)
        ch = postcorr.advance(ch, B)._replace(carr_step=(ch.carr_step + int(rng.integers(-3000, 3000))) % 2 ** 32,
                                              code_step=ch.code_step + int(rng.integers(-50, 50)))
    raw = cr.quantise(z)
    chans = [(int(r["code_phase"]), int(r["code_step"]), int(r["carr_phase"]), int(r["carr_step"]), 0, 0) for r in rec[0]]
    prompts = lambda b: np.array([cr.bank(b, start + m * B, B, B, codes, [chans[m]], (0,))[0, 0, 0] for m in range(E)], np.int64)
    before = prompts(raw)
    rec["prompt"][0] = before
    amps = track.amplitudes(rec, B)
    assert amps.shape == (1, E, 2) and amps.dtype == np.int32
    want = np.floor(before / (B * postcorr.MIXER_GAIN) * 2.0 ** 16 + 0.5)
    assert np.array_equal(amps[0], want) and np.array_equal(track.amplitudes(rec[0], B), amps)
    got, blk = st.subtract_tracked(raw, 0, raw.size // 2, B, E, codes, [(start, 0)], rec, amps, sr.DITHER, 0)
    after = prompts(got)
    share = np.abs(after[:, 0] + 1j * after[:, 1]) / np.abs(before[:, 0] + 1j * before[:, 1])
    print("prompt left of each epoch's own:", np.round(share, 4).tolist())
    # the byte's rounding (1 / sqrt(12) LSB per component, twice: the capture's and the cleaned one's) over 2048 samples against
    # 40 LSB of signal: 0.41 / 40 / sqrt(2048) = 2.3e-4 rms; the 16-step carrier leaves nothing at the replica's own NCO
    assert share.max() < 0.002 and not blk["n_clipped"].any()
    assert got[:2 * start].tobytes() == raw[:2 * start].tobytes() and got[2 * (start + E * B):].tobytes() == raw[2 * (start + E * B):].tobytes()


# ------------------------------------------------------------------------------------------------ end to end
def test_the_tracked_replica_leaves_less_than_the_open_loop_one():
    """The loop capture (1.2 s under a 50 Hz/s ramp) cleaned twice: at the tracked NCOs, and open loop at the grid
    channel with one amplitude per epoch.  The judge reads both at the truth's per-epoch NCOs against an absent PRN."""
    raw, codes = tr.loop_capture(), tr.loop_codes()
    rows, _ = tr.loop_track()
    rec = st.records_from_rows(rows)[None]
    assert rec.shape == (1, tr.LOOP_EPOCHS)
    tracked, blk = st.subtract_tracked(raw, 0, tr.LOOP_SAMPLES, tr.LOOP_B, tr.LOOP_EPOCHS, codes, [(tr.LOOP_START, 0)], rec,
                                       track.amplitudes(rec, tr.LOOP_B), sr.DITHER, 0)
    n = tr.LOOP_EPOCHS * tr.LOOP_B
    piece, oblk = sr.subtract(raw, tr.LOOP_START, n, tr.LOOP_B, codes, [tr.loop_channel()], st.open_loop_amplitudes(tr.loop_open()), sr.DITHER, 0)
    opened = np.array(raw)
    opened[2 * tr.LOOP_START:2 * (tr.LOOP_START + n)] = piece
    figures = {"untouched": st.residue_db(raw), "tracked": st.residue_db(tracked), "open loop": st.residue_db(opened)}
    print("residue over the absent PRN's floor, dB:", {k: round(v, 3) for k, v in figures.items()},
          f"(recorded: tracked {st.E2E_CPU_RESIDUE_TRACKED_DB}, open loop {st.E2E_CPU_RESIDUE_OPEN_DB})")
    assert abs(figures["tracked"] / st.E2E_CPU_RESIDUE_TRACKED_DB - 1.0) <= 0.1
    assert abs(figures["open loop"] / st.E2E_CPU_RESIDUE_OPEN_DB - 1.0) <= 0.1
    assert figures["tracked"] < figures["open loop"] < figures["untouched"]
    assert not blk["n_clipped"].any() and not oblk["n_clipped"].any(), "no byte is clipped"
