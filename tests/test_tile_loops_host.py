"""The helpers and the size rules of the tile-loop tests (tests/tile_loops_inputs.py), held to the existing restatements
on the CPU: a sub-range with moved arguments gives the bytes and records of the whole range's restatement, the windows
of the runs at the limit are where a workgroup's second and third tile lie, and the dither's key is 64 bits wide."""
import numpy as np
import pytest

import align_restatement as ar
import corr_restatement as cr
import subtract_restatement as sr
import tile_loops_inputs as tl

N3 = 3 * 4096                                   # three tiles
# (t1, samples): sub-ranges that start on a tile, on a multiple of 16 that is no tile, and on no multiple of 16
PARTS = ((0, 4096), (4096, 2 * 4096), (8192, 4096), (4096 + 48, 4000), (1, 50), (4095, 3), (5000 + 7, 4096 + 77))


# ------------------------------------------------------------------------------------------------ moved arguments
@pytest.mark.parametrize("name", ["fastest step", "slowest step", "negative start"])
def test_moved_align_gives_the_whole_ranges_bytes_and_records(name):
    raw, case, tables = ar.parity_capture(), ar.CASES[name], ar.tables("mid")
    whole, wrec = ar.align(raw, *case, *tables, N3)
    for n1, m in PARTS:
        part, prec = ar.align(raw, *tl.moved_align(case, n1), *tables, m)
        assert part.tobytes() == whole[2 * n1:2 * (n1 + m)].tobytes(), (n1, m)
        if n1 % ar.BLOCK == 0 and m % ar.BLOCK == 0:
            assert prec.tobytes() == wrec[n1 // ar.BLOCK:(n1 + m) // ar.BLOCK].tobytes(), (n1, m)
        # ... and on the span of the source that the sub-range reads, edge samples included
        lo, hi = tl.align_span(tl.moved_align(case, n1), m, raw.size // 2)
        cut, crec = ar.align(raw[2 * lo:2 * hi], *tl.on_span(tl.moved_align(case, n1), lo), *tables, m)
        assert cut.tobytes() == part.tobytes() and crec.tobytes() == prec.tobytes(), (n1, m, lo, hi)
    for piece in (4096, 2 * 4096):
        got, rec = tl.align_in_pieces(raw, case, *tables, N3 + 5, piece=piece)
        want, wrec5 = ar.align(raw, *case, *tables, N3 + 5)
        assert got.tobytes() == want.tobytes() and rec.tobytes() == wrec5.tobytes(), piece


def test_the_span_of_a_range_that_leaves_the_source_keeps_its_edge_samples():
    raw, tables = ar.parity_capture(), ar.tables("mid")
    for name in ("ends past the source's end", "start past the source's end", "far before the source", "far behind the source"):
        case = ar.CASES[name]
        want, wrec = ar.align(raw, *case, *tables, 4096 + 9)
        got, rec = tl.align_in_pieces(raw, case, *tables, 4096 + 9, piece=4096)
        assert got.tobytes() == want.tobytes() and rec.tobytes() == wrec.tobytes(), name
    assert int(wrec["n_edge"].sum()) == 4096 + 9


def test_moved_channel_gives_the_whole_ranges_bytes_and_records_of_the_subtraction():
    raw, codes, channels = cr.parity_capture(), cr.parity_codes(), cr.parity_channels(6)
    first, B, seed = 7, 16, 0xC0FFEE11
    amps = sr.random_amps(6, cr.blocks(N3, B), 2 ** 14)
    whole, wrec = sr.subtract(raw, first, N3, B, codes, channels, amps, sr.DITHER, seed)
    for t1, m in PARTS:
        if t1 % B:
            continue                                           # amplitudes go by blocks of the range: a sub-range starts on one
        moved = [tl.moved_channel(ch, t1) for ch in channels]
        part, prec = sr.subtract(raw, first + t1, m, B, codes, moved, amps[:, t1 // B:t1 // B + cr.blocks(m, B)], sr.DITHER, seed)
        assert part.tobytes() == whole[2 * t1:2 * (t1 + m)].tobytes(), (t1, m)
        if t1 % sr.SUB_BLOCK == 0 and m % sr.SUB_BLOCK == 0:
            assert prec.tobytes() == wrec[t1 // sr.SUB_BLOCK:(t1 + m) // sr.SUB_BLOCK].tobytes(), (t1, m)
    # at a t1 that is no multiple of 16: one amplitude for the whole range, so that blocks do not matter
    one = sr.random_amps(6, 1, 2 ** 14)
    whole, _ = sr.subtract(raw, first, N3, 4096, codes, channels, np.repeat(one, 3, axis=1), sr.DITHER, seed)
    for t1, m in PARTS:
        moved = [tl.moved_channel(ch, t1) for ch in channels]
        part, _ = sr.subtract(raw, first + t1, m, 4096, codes, moved, np.repeat(one, cr.blocks(m, 4096), axis=1), sr.DITHER, seed)
        assert part.tobytes() == whole[2 * t1:2 * (t1 + m)].tobytes(), (t1, m)


def test_moved_channel_gives_the_whole_ranges_records_of_the_bank():
    raw, codes, channels = cr.parity_capture(), cr.parity_codes(), cr.parity_channels(6)
    taps = (0, -64, 33)
    for B in (16, 48):
        whole = cr.bank(raw, 1, N3, B, codes, channels, taps)
        for t1, m in PARTS:
            moved = [tl.moved_channel(ch, t1) for ch in channels]
            part = cr.bank(raw, 1 + t1, m, B, codes, moved, taps)
            if t1 % B == 0:
                full = m // B                                  # the sub-range's last block may be a ragged one
                assert np.array_equal(part[:, :full], whole[:, t1 // B:t1 // B + full]), (B, t1, m)
            else:                                              # blocks no longer line up: the sums over the sub-range do
                one = cr.bank(raw, 1 + t1, m, 4096, codes, moved, taps) if m <= 4096 else None
                if one is not None:
                    assert np.array_equal(one[:, 0], part.sum(axis=1)), (B, t1, m)
    # t1 no multiple of 16 against the whole range: sample by sample through one-sample blocks is too slow, so through
    # the difference of two ranges that start at 0
    whole = cr.bank(raw, 1, 5007 + 300, 4096, codes, channels, taps).sum(axis=1)
    head = cr.bank(raw, 1, 5007, 4096, codes, channels, taps).sum(axis=1)
    tail = cr.bank(raw, 1 + 5007, 300, 4096, codes, [tl.moved_channel(ch, 5007) for ch in channels], taps).sum(axis=1)
    assert np.array_equal(whole - head, tail)


def test_moved_channel_at_the_limit_is_the_python_int_definition():
    """code_step = 2^34 - 1 from the period's last phase at t1 = 2^28 - 4096: t code_step passes 2^61.  The chip and the
    carrier index of samples t1 .. t1 + 63, each from the definition with Python ints, against the moved channel's at
    0 .. 63, against numpy int64 at the absolute t (the restatements' arithmetic), and through sr.brute."""
    t1 = tl.LIMIT - 4096
    ch = tl.limit_channels()[0]
    assert ch[1] == 2 ** 34 - 1 and ch[0] == cr.PERIOD - 1 and 2 ** 61 < (tl.LIMIT - 1) * ch[1] < 2 ** 62
    moved = tl.moved_channel(ch, t1)
    cr.check_channels(cr.parity_codes(), [moved])
    for d in (0, -1, 64, -64):
        for t in range(64):
            chip = ((ch[0] + (t1 + t + d) * ch[1]) // 2 ** 32) % 1023
            index = ((ch[2] + (t1 + t) * ch[3]) % 2 ** 32) // 2 ** 28
            assert cr.chip_index(moved[0], moved[1], t + d) == chip and cr.carrier_index(moved[2], moved[3], t) == index, (t, d)
            assert int(cr.chip_index(ch[0], ch[1], np.array([t1 + t + d], np.int64))[0]) == chip
            assert int(cr.carrier_index(ch[2], ch[3], np.array([t1 + t], np.int64))[0]) == index
    raw, codes = cr.parity_capture(), cr.parity_codes()
    amps = sr.random_amps(1, 1, 2 ** 14)
    first = 2 ** 31 + 1
    got, rec = sr.subtract(tl.sparse_capture(first + 64, {first: raw[:128]}), first, 64, 4096, codes, [moved], amps, sr.DITHER, 9)
    near, _ = sr.brute(np.concatenate((np.zeros(2, np.uint8), raw[:128])), 1, 64, 4096, codes, [moved], amps, sr.DITHER, 9)
    assert len(near) == 128 and got.tolist() != near, "the same bytes at first = 1: another dither"
    out = []
    for t in range(64):                                       # sr.brute's sample loop at an absolute index past 2^31
        chip = ((ch[0] + (t1 + t) * ch[1]) // 2 ** 32) % 1023
        i = ((ch[2] + (t1 + t) * ch[3]) % 2 ** 32) // 2 ** 28
        c = -1 if int(codes[ch[4]][chip]) < 0 else 1
        aI, aQ = (int(v) for v in amps[0][0])
        R = (c * (aI * cr.COS[i] + aQ * cr.SIN[i]), c * (aQ * cr.COS[i] - aI * cr.SIN[i]))
        for comp in (0, 1):
            out.append(max(0, min(255, int(raw[2 * t + comp]) - (R[comp] + sr.dither_one(first + t, comp, 9)) // 65536)))
    assert got.tolist() == out


# ------------------------------------------------------------------------------------------------ sizes and windows
@pytest.mark.parametrize("cus", [1, 64, 256, 304])
def test_looping_tiles_gives_every_workgroup_a_second_tile(cus):
    T = tl.looping_tiles(cus)
    assert T > 2 * 4 * cus and T - 2 * 4 * cus == 3, "four slots per CU: every workgroup a second tile, three a third"
    assert T - 8 * cus == 3, "eight slots per CU: three workgroups still take a second tile"
    assert tl.looping_tiles(256) == 2051
    for B, blocks in ((48, 85), (256, 16), (4096, 1)):
        assert tl.corr_tile(B) == blocks * B <= 4096


@pytest.mark.parametrize("slots", [768, 1024])
@pytest.mark.parametrize("T", [3, 2051, 65536])
def test_the_windows_of_the_limit_runs(T, slots):
    w = tl.limit_windows(T, slots)
    assert w and w == sorted(set(w)) and w[0] == 0 and w[-1] == T - 1 and all(0 <= t < T for t in w) and len(w) <= 13
    assert {0, 1, T - 2, T - 1, T // 2, T // 3} <= set(w)
    if T > 2 * slots:                                          # workgroup 0's first, second and third tile, and its neighbours'
        assert {0, slots, 2 * slots} <= set(w) and {slots - 1, slots + 1, 2 * slots - 1, 2 * slots + 1} <= set(w)
    assert tl.LIMIT // tl.SUB_TILE == 65536 == tl.LIMIT // tl.ALIGN_TILE


def test_the_limit_align_case_runs_off_the_sources_end():
    pos0, step, phase, rot_step = tl.LIMIT_ALIGN_CASE
    assert step == ar.ONE + ar.MAX_DRIFT and pos0 < 0 and phase and rot_step % 2 == 1 and tl.LIMIT == ar.MAX_SAMPLES
    assert 2 ** 60 < (tl.LIMIT - 1) * step < 2 ** 61
    last = tl.moved_align(tl.LIMIT_ALIGN_CASE, tl.LIMIT - 2 * 4096)
    assert tl.align_span(last, 2 * 4096, tl.LIMIT_SOURCE_SAMPLES) == (tl.LIMIT_SOURCE_SAMPLES - 1, tl.LIMIT_SOURCE_SAMPLES)
    out, rec = ar.align(np.full(2, 255, np.uint8), *tl.on_span(last, tl.LIMIT_SOURCE_SAMPLES - 1), *ar.tables("mid"), 2 * 4096)
    assert np.all(out == 128) and rec["n_edge"].tolist() == [4096, 4096]
    lo, hi = tl.align_span(tl.LIMIT_ALIGN_CASE, 4096, tl.LIMIT_SOURCE_SAMPLES)
    assert lo == 0 and hi == ((pos0 + 4095 * step + (1 << 23)) >> 32) + 9


# ------------------------------------------------------------------------------------------------ the dither's key
def test_the_dither_sees_the_upper_word_of_its_key():
    seed = 0xC0FFEE11
    far, near = sr.dither(2 ** 31 + 1, 8, seed), sr.dither(1, 8, seed)
    assert far.shape == (8, 2) and not np.array_equal(far, near)
    assert far.tolist() == [[sr.dither_one(2 ** 31 + 1 + t, comp, seed) for comp in (0, 1)] for t in range(8)]
    k = 2 * (2 ** 31 + 1)
    assert k >> 32 == 1 and sr.dither_one(2 ** 31 + 1, 0, seed) == sr.hash32((k & tl.M32) ^ 0x9e3779b9 ^ seed) >> 16


def test_a_sparse_capture_is_zero_but_for_its_windows():
    raw = tl.sparse_capture(2 ** 31 + 9, {2 ** 31 + 1: np.arange(16, dtype=np.uint8)})
    assert raw.size == 2 ** 32 + 18 and raw[2 ** 32 + 2:].tolist() == list(range(16)) and not raw[2 ** 32 - 64:2 ** 32 + 2].any()
