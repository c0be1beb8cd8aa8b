"""The five kernels that walk their range tile by tile from a fixed grid -- gj_align_dev, gj_subtract_dev,
gj_xcorr_fine_dev, gj_corr_bank_dev, gj_synth_u8_dev -- at sizes where that loop turns: every workgroup takes a second
tile (section 1), the range lies past byte 2^32 of its capture (section 2), and n is the limit 2^28 (section 3).

This file sits in a package of its own on purpose, as tests/align/ and tests/corr/ do: the suite orders GPU files by
basename (tests/conftest.py SUITE_ORDER, which tests/test_suite_order.py holds every GPU file to), and under the name
test_round6_gpu.py it runs in stage 2.

Yardsticks: the integer restatements of the definitions in include/gpsjam.h (tests/align_restatement.py,
subtract_restatement.py, fine_restatement.py, corr_restatement.py) and gpsjam/synth.py, imported, each held to a
per-sample Python-int loop by its own host test.  Everything is integer arithmetic: EVERY compared byte and record is
equal, bit for bit.  Sections 1 and 2 compare every byte and every record of the call.  Section 3 compares the tiles
of tile_loops_inputs.limit_windows -- at most 13 of 65 536, a fixed list around a workgroup's first, second and third
tile, the middle and the end -- with the restatement of that tile alone under moved arguments
(tests/test_tile_loops_host.py holds the moving to the whole range's restatement); the rest of those outputs is not
looked at.  Every call writes into 0xA5-filled buffers whose 256 bytes on either side of the call's output must stay
untouched.  The captures are random bytes of one seeded stream or the synthesiser's: no two tiles are alike.

Each test of section 1 asserts that its run has more than twice as many tiles as the grid has workgroups, from the
device's CU count and the kernel's present workgroups per CU: a change of a grid fails that assertion instead of
quietly taking the loop out of the test."""
import numpy as np
import pytest

import align_restatement as ar
import corr_restatement as cr
import fine_restatement as fr
import gpsjam
import subtract_restatement as sr
import tile_loops_inputs as tl
from gpsjam.synth import StreamSpec, generate
from gpu_lib import GJ_ERR_INVALID, Guarded, freed, refused, run_align, run_corr, run_fine, run_subtract

pytestmark = pytest.mark.gpu


# workgroups per CU of each grid as it is launched today
ALIGN_PER_CU = 4                                # k_align.hip gj_align_dev: slots = 4ull * num_cus
SUBTRACT_PER_CU = 4                             # k_subtract.hip gj_subtract_dev: replica_grid(ctx, 4, g.n_tiles)
FINE_PER_CU = 4                                 # k_fine.hip gj_xcorr_fine_dev: slots = 4ull * num_cus
CORR_PER_CU = 3                                 # k_corr.hip gj_corr_bank_dev: replica_grid(ctx, 3, g.n_tiles)
SYNTH_PER_CU = 32                               # k_synth.hip launch_synth: blocks <= num_cus * 32

TAPS = (0, -64, 33)
FIRST = 7                                       # an odd first sample
FINE_FIRST_A, FINE_FIRST_B = 5, 4107            # odd, and different


@pytest.fixture(scope="module")
def cus(dev):
    n = int(dev.info()["compute_units"])
    assert n >= 1
    return n


@pytest.fixture(scope="module")
def raws(cus):
    """Two independent random captures, long enough for the longest range of section 1 from any first sample."""
    n = tl.looping_tiles(cus) * tl.FINE_TILE + 5 + 2 * 4200
    return tl.random_capture(n, 20261), tl.random_capture(n, 20262)


@pytest.fixture(scope="module")
def caps(dev, raws):
    held = [dev.capture(r) for r in raws]
    yield held
    freed(*held)


@pytest.fixture(scope="module")
def d_codes(dev):
    b = dev.alloc(cr.parity_codes().nbytes).upload(cr.parity_codes())
    yield b
    b.free()


@pytest.fixture(scope="module")
def d_tables(dev):
    """kind -> (taps, rot) of the alignment on the device."""
    held = {}
    for kind in ("mid", "wide"):
        t, r = ar.tables(kind)
        held[kind] = (dev.alloc(t.nbytes).upload(t), dev.alloc(r.nbytes).upload(r))
    yield held
    for pair in held.values():
        freed(*pair)


def same_bytes(got, want, what):
    """Every byte equal; on a difference, where the first one lies."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        at = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
        raise AssertionError(f"{what}: {at.size} of {got.size} values differ, the first at {at[:8].tolist()} (tile {int(at[0]) // 8192} if these are output bytes)")


def same_records(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        bad = [k for k in range(got.shape[0]) if got[k].tobytes() != want[k].tobytes()]
        raise AssertionError(f"{what}: {len(bad)} of {got.shape[0]} records differ, the first {bad[:8]}: {got[bad[0]]} for {want[bad[0]]}")


# ------------------------------------------------------------------------------------------------ 1. every workgroup's second tile
@pytest.mark.parametrize("kind", ["mid", "wide"])
@pytest.mark.parametrize("name", ["fastest step", "slowest step"])
def test_align_where_every_workgroup_takes_a_second_tile(dev, cus, raws, caps, d_tables, name, kind):
    tiles = tl.looping_tiles(cus)
    assert tiles > 2 * ALIGN_PER_CU * cus
    print(f"{cus} CUs: {tiles} tiles of {tl.ALIGN_TILE} on {ALIGN_PER_CU * cus} workgroups")
    assert ar.CASES[name][1] == ar.ONE + (ar.MAX_DRIFT if name == "fastest step" else -ar.MAX_DRIFT), "the largest drifts"
    n_out = tiles * tl.ALIGN_TILE + 5
    n_src = n_out + 300
    case, what = ar.CASES[name], f"align {name} tables {kind} n_out {n_out}"
    want, wrec = tl.align_in_pieces(raws[0][:2 * n_src], case, *ar.tables(kind), n_out)
    got, rec = run_align(dev, caps[0], 2 * n_src, case, *d_tables[kind], n_out)
    same_bytes(got, want, what)
    same_records(rec, wrec, what)
    bare, none = run_align(dev, caps[0], 2 * n_src, case, *d_tables[kind], n_out, records=False, out_offset=2)
    assert none is None
    same_bytes(bare, want, what + " records off, output 2 bytes off alignment")


@pytest.mark.parametrize("flags, seed", [(1, 0xC0FFEE11), (0, 0)])
@pytest.mark.parametrize("B", [48, 4096])
def test_subtract_where_every_workgroup_takes_a_second_tile(dev, cus, raws, caps, d_codes, B, flags, seed):
    tiles = tl.looping_tiles(cus)
    assert tiles > 2 * SUBTRACT_PER_CU * cus
    print(f"{cus} CUs: {tiles} tiles of {tl.SUB_TILE} on {SUBTRACT_PER_CU * cus} workgroups")
    n = tiles * tl.SUB_TILE + 5
    codes, channels = cr.parity_codes(), cr.parity_channels(3)
    amps = sr.random_amps(3, cr.blocks(n, B), 2 ** 14, seed=B)
    what = f"subtract n {n} B {B} flags {flags} seed {seed}"
    want, wrec = sr.subtract(raws[0], FIRST, n, B, codes, channels, amps, flags, seed)
    got, rec = run_subtract(dev, caps[0], FIRST, n, B, d_codes, len(codes), channels, amps, flags, seed)
    same_bytes(got, want, what)
    same_records(rec, wrec, what)
    bare, none = run_subtract(dev, caps[0], FIRST, n, B, d_codes, len(codes), channels, amps, flags, seed, records=False, out_offset=2)
    assert none is None
    same_bytes(bare, want, what + " records off, output 2 bytes off alignment")


@pytest.mark.parametrize("centre, half", [(3, 2), (-4099, 16)])
def test_fine_where_every_workgroup_takes_a_second_tile(dev, cus, raws, caps, centre, half):
    tiles = tl.looping_tiles(cus)
    assert tiles > 2 * FINE_PER_CU * cus
    print(f"{cus} CUs: {tiles} tiles of {tl.FINE_TILE} on at most {FINE_PER_CU * cus} workgroups")
    n = tiles * tl.FINE_TILE + 5
    a, b = caps
    what = f"fine n {n} centre {centre} half {half}"
    want = fr.fine(raws[0], raws[1], centre, half, FINE_FIRST_A, FINE_FIRST_B, n)
    total, blocks = run_fine(dev, a, b, FINE_FIRST_A, FINE_FIRST_B, n, centre, half)
    same_records(blocks.astype(np.int64), want.blocks, what)
    np.testing.assert_array_equal(total, want.total, err_msg=what + ": the 64-bit sums over a workgroup's tiles")
    bare, none = run_fine(dev, a, b, FINE_FIRST_A, FINE_FIRST_B, n, centre, half, want_blocks=False)
    assert none is None
    np.testing.assert_array_equal(bare, want.total, err_msg=what + " without records")


@pytest.mark.parametrize("B", [48, 256, 4096])
def test_corr_where_every_workgroup_takes_a_second_tile(dev, cus, raws, caps, d_codes, B):
    tiles = tl.looping_tiles(cus)
    n = tiles * tl.corr_tile(B) + B + 5
    tile_blocks = 4096 // B
    assert tile_blocks == {48: 85, 256: 16, 4096: 1}[B]
    assert -(-cr.blocks(n, B) // tile_blocks) > tiles > 2 * CORR_PER_CU * cus
    print(f"{cus} CUs: {-(-cr.blocks(n, B) // tile_blocks)} tiles of {tl.corr_tile(B)} on {CORR_PER_CU * cus} workgroups")
    codes, channels = cr.parity_codes(), cr.parity_channels(4)
    want = cr.bank(raws[0], 1, n, B, codes, channels, TAPS)
    got = run_corr(dev, caps[0], 1, n, B, d_codes, len(codes), channels, TAPS)
    for ch in range(4):
        same_records(got[ch].astype(np.int64), want[ch], f"corr n {n} B {B} channel {ch} (records of {tile_blocks} to a tile)")


def synth_windows(n, one_pass, m=100000):
    """{first sample: samples} of the compared windows: the start, one across each end of a pass of the grid (the
    second runs to the range's end: the third pass is a short one), the end."""
    return {w: min(m, n - w) for w in sorted({0, one_pass - m // 2, 2 * one_pass - m // 2, n - m})}


@pytest.mark.parametrize("first", [0, -123457])
def test_synth_over_two_passes_of_the_grid_and_a_ragged_third(dev, cus, first):
    one_pass = SYNTH_PER_CU * cus * tl.SYNTH_THREADS * tl.SYNTH_GROUP          # samples of one pass of the whole grid
    n = 2 * one_pass + tl.SYNTH_GROUP * 4099 + 5
    blocks = -(-(-(-n // tl.SYNTH_GROUP)) // tl.SYNTH_THREADS)
    assert blocks > 2 * SYNTH_PER_CU * cus, "every thread takes a second group and some a third"
    print(f"{cus} CUs: {n} samples, {blocks} blocks' worth on {SYNTH_PER_CU * cus} blocks")
    # the jammer comes on 5000 samples in front of the first pass's end and goes 7000 behind it, seen 37 samples late
    spec = StreamSpec(seed=31, antenna=1, delay=37, jam_start=first + one_pass - 5000 - 37, jam_end=first + one_pass + 7000 - 37,
                      jam_sigma=60.0, dc_i_q8=300, dc_q_q8=-200)
    m = 100000
    want = {w: generate(spec, mw, first_sample=first + w) for w, mw in synth_windows(n, one_pass, m).items()}
    assert all(0 <= w and 2 * w + bytes_.size <= 2 * n for w, bytes_ in want.items())
    across = want[one_pass - m // 2]
    assert across[:2 * (m // 2 - 5000)].std() < 0.5 * across[2 * (m // 2 - 5000):2 * (m // 2 + 7000)].std(), "the jammer straddles the pass's end"
    for offset in ((0, 2) if first == 0 else (0,)):                              # 2: the byte-wise store path
        out = Guarded(dev, 2 * n, offset)
        try:
            dev.synth_dev(spec, n, out.ptr, first_sample=first)
            out.check_pads("output")
            for w, bytes_ in want.items():
                same_bytes(out.read(np.uint8, bytes_.size, 2 * w), bytes_, f"synth first {first} offset {offset} window at {w}")
        finally:
            out.free()


# ------------------------------------------------------------------------------------------------ 2. past byte 2^32
BIG = 2 ** 32 + 2 ** 20
WINDOW_AT = 2 ** 32 + 2                         # byte offset of the ranges: sample 2^31 + 1, an odd one
S0 = WINDOW_AT // 2
FAR_SAMPLES = 3 * 4096 + 5
FAR_B = S0 + 4096 + 7                           # fine's second range, in the same buffer
FAR_UPLOAD = 4096 + 7 + FAR_SAMPLES             # samples uploaded at S0


class TestPastByte2To32:
    @pytest.fixture(scope="class")
    def big(self, dev):
        """4 GiB + 1 MiB, never filled: only the window that is uploaded is ever read.  An allocation failure fails.
        Class-scoped: it is gone before section 3 allocates."""
        b = dev.alloc(BIG)
        assert b.ptr and b.nbytes == BIG
        window = tl.random_capture(FAR_UPLOAD, 20263)
        b.upload(window, offset=WINDOW_AT)
        assert b.download(np.uint8, 64, offset=WINDOW_AT).tobytes() == window[:64].tobytes()
        yield b, window
        b.free()

    def test_subtract_past_byte_2_32(self, dev, big, d_codes):
        """The dither's key is the ABSOLUTE index: from sample 2^31 on its upper word counts."""
        buf, window = big
        assert WINDOW_AT > 2 ** 32 and S0 == 2 ** 31 + 1 and WINDOW_AT + 2 * FAR_UPLOAD <= BIG
        codes, channels = cr.parity_codes(), cr.parity_channels(3)
        amps = sr.random_amps(3, cr.blocks(FAR_SAMPLES, 256), 2 ** 14)
        seed = 0xC0FFEE11
        want, wrec = sr.subtract(tl.sparse_capture(S0 + FAR_SAMPLES, {S0: window[:2 * FAR_SAMPLES]}), S0, FAR_SAMPLES, 256, codes, channels,
                                 amps, sr.DITHER, seed)
        near, _ = sr.subtract(np.concatenate((np.zeros(2, np.uint8), window[:2 * FAR_SAMPLES])), 1, FAR_SAMPLES, 256, codes, channels, amps,
                              sr.DITHER, seed)
        assert near.tobytes() != want.tobytes(), "the same bytes from sample 1: the upper word of the key is seen"
        got, rec = run_subtract(dev, buf, S0, FAR_SAMPLES, 256, d_codes, len(codes), channels, amps, sr.DITHER, seed)
        same_bytes(got, want, "subtract past sample 2^31")
        same_records(rec, wrec, "subtract past sample 2^31")

    def test_corr_and_fine_past_byte_2_32(self, dev, big, d_codes):
        buf, window = big
        codes, channels = cr.parity_codes(), cr.parity_channels(4)
        for B in (48, 4096):
            want = cr.bank(window, 0, FAR_SAMPLES, B, codes, channels, TAPS)
            got = run_corr(dev, buf, S0, FAR_SAMPLES, B, d_codes, len(codes), channels, TAPS)
            same_records(got.astype(np.int64).reshape(-1, 2 * len(TAPS)), want.reshape(-1, 2 * len(TAPS)), f"corr past sample 2^31, B {B}")
        for centre, half in ((3, 2), (-4099, 16)):
            want = fr.fine(window, window, centre, half, 0, FAR_B - S0, FAR_SAMPLES)
            total, blocks = run_fine(dev, buf, buf, S0, FAR_B, FAR_SAMPLES, centre, half)
            same_records(blocks.astype(np.int64), want.blocks, f"fine past sample 2^31, centre {centre}")
            np.testing.assert_array_equal(total, want.total)

    def test_a_range_that_ends_one_sample_past_the_buffer_is_refused(self, dev, big, d_codes):
        buf, _ = big
        codes, channels = cr.parity_codes(), cr.parity_channels(3)
        table = np.array(channels, gpsjam.CORR_CHANNEL_DTYPE)
        amps = sr.random_amps(3, cr.blocks(FAR_SAMPLES, 256), 2 ** 14)
        out, rec = Guarded(dev, 2 * FAR_SAMPLES), Guarded(dev, 8 * 3 * cr.blocks(FAR_SAMPLES, 256) * len(TAPS))
        d_ch, d_amp = dev.alloc(table.nbytes).upload(table), dev.alloc(amps.nbytes).upload(amps)
        try:
            for first in (BIG // 2 - FAR_SAMPLES + 1, BIG // 2):
                calls = {
                    "subtract": lambda: dev.subtract_dev(buf, BIG, first, FAR_SAMPLES, 256, d_codes, len(codes), d_ch, 3, d_amp, sr.DITHER, 1, out.ptr, rec.ptr),
                    "corr": lambda: dev.corr_bank_dev(buf, BIG, first, FAR_SAMPLES, 256, d_codes, len(codes), d_ch, 3, TAPS, rec.ptr),
                    "fine, range a": lambda: dev.xcorr_fine_dev(buf, BIG, first, buf, BIG, S0, FAR_SAMPLES, 0, 2, out.ptr, rec.ptr),
                    "fine, range b": lambda: dev.xcorr_fine_dev(buf, BIG, S0, buf, BIG, first, FAR_SAMPLES, 0, 2, out.ptr, rec.ptr),
                }
                refused(dev, lambda name: calls[name](), [((name,), GJ_ERR_INVALID) for name in calls], out, rec)
            # the last range that fits is taken
            dev.corr_bank_dev(buf, BIG, BIG // 2 - FAR_SAMPLES, FAR_SAMPLES, 256, d_codes, len(codes), d_ch, 3, TAPS, rec.ptr)
            dev.synchronize()
            rec.check_pads("records")
        finally:
            freed(out, rec, d_ch, d_amp)


# ------------------------------------------------------------------------------------------------ 3. n = 2^28
LIMIT_TILES = tl.LIMIT // 4096                  # 65 536 tiles of align, subtract and (B = 4096) corr alike
LIMIT_SPEC = StreamSpec(seed=77, antenna=2, delay=3, jam_start=-(1 << 40), jam_end=1 << 40, jam_sigma=40.0, dc_i_q8=-90, dc_q_q8=120)


class TestAtTheLimit:
    @pytest.fixture(scope="class")
    def source(self, dev):
        """2^28 + 64 samples made on the device by the synthesiser (512 MiB, nothing uploaded): loud noise, no two
        tiles alike.  tests/test_round2_gpu.py and the synth test above hold those bytes to gpsjam/synth.py."""
        b = dev.alloc(2 * tl.LIMIT_SOURCE_SAMPLES)
        dev.synth_dev(LIMIT_SPEC, tl.LIMIT_SOURCE_SAMPLES, b)
        dev.synchronize()
        head = b.download(np.uint8, 2 * 4096)
        assert head.tobytes() == generate(LIMIT_SPEC, 4096).tobytes() and head.std() > 20
        yield b
        b.free()

    def test_corr_at_the_limit(self, dev, cus, source, d_codes):
        codes, channels = cr.parity_codes(), tl.limit_channels()
        table = np.array(channels, gpsjam.CORR_CHANNEL_DTYPE)
        out = Guarded(dev, 8 * 2 * LIMIT_TILES)
        d_ch = dev.alloc(table.nbytes).upload(table)
        try:
            dev.corr_bank_dev(source, source.nbytes, 1, tl.LIMIT, 4096, d_codes, len(codes), d_ch, 2, (-1,), out.ptr)
            out.check_pads("records")
            got = out.read(np.int32).reshape(2, LIMIT_TILES, 1, 2)
        finally:
            freed(out, d_ch)
        assert not np.any(got.view(np.uint32) == 0xA5A5A5A5), "every record was written (the sentinel is outside a record's bound)"
        for tile in tl.limit_windows(LIMIT_TILES, CORR_PER_CU * cus):
            t1 = tile * 4096
            window = source.download(np.uint8, 2 * 4096, offset=2 * (1 + t1))
            want = cr.bank(window, 0, 4096, 4096, codes, [tl.moved_channel(ch, t1) for ch in channels], (-1,))
            assert got[:, tile].astype(np.int64).tolist() == want[:, 0].tolist(), f"corr at the limit: tile {tile}"

    def test_subtract_at_the_limit(self, dev, cus, source, d_codes):
        codes, channels = cr.parity_codes(), tl.limit_channels()
        table = np.array(channels, gpsjam.CORR_CHANNEL_DTYPE)
        amps = sr.random_amps(2, LIMIT_TILES, 2 ** 14)
        seed = 0xC0FFEE11
        out, rec = Guarded(dev, 2 * tl.LIMIT, fill=False), Guarded(dev, 24 * LIMIT_TILES)
        d_ch, d_amp = dev.alloc(table.nbytes).upload(table), dev.alloc(amps.nbytes).upload(amps)
        try:
            dev.subtract_dev(source, source.nbytes, 1, tl.LIMIT, 4096, d_codes, len(codes), d_ch, 2, d_amp, sr.DITHER, seed, out.ptr, rec.ptr)
            out.check_pads("output")
            rec.check_pads("records")
            records = rec.read(gpsjam.SUB_DTYPE)
            for tile in tl.limit_windows(LIMIT_TILES, SUBTRACT_PER_CU * cus):
                t1 = tile * 4096
                window = source.download(np.uint8, 2 * 4096, offset=2 * (1 + t1))
                want, wrec = sr.subtract(tl.sparse_capture(1 + t1 + 4096, {1 + t1: window}), 1 + t1, 4096, 4096, codes,
                                         [tl.moved_channel(ch, t1) for ch in channels], amps[:, tile:tile + 1], sr.DITHER, seed)
                same_bytes(out.read(np.uint8, 2 * 4096, 2 * t1), want, f"subtract at the limit: tile {tile}")
                assert records[tile].tobytes() == wrec[0].tobytes(), f"subtract at the limit: record {tile}: {records[tile]} for {wrec[0]}"
                assert int(wrec[0]["removed"]) > 0
        finally:
            freed(out, rec, d_ch, d_amp)

    def test_align_at_the_limit(self, dev, cus, source, d_tables):
        case, tables, n_src = tl.LIMIT_ALIGN_CASE, ar.tables("mid"), tl.LIMIT_SOURCE_SAMPLES
        out, rec = Guarded(dev, 2 * tl.LIMIT, fill=False), Guarded(dev, 16 * LIMIT_TILES)
        try:
            dev.align_dev(source, source.nbytes, case, *d_tables["mid"], tl.LIMIT, out.ptr, rec.ptr)
            out.check_pads("output")
            rec.check_pads("records")
            records = rec.read(gpsjam.ALIGN_DTYPE)
            windows = tl.limit_windows(LIMIT_TILES, ALIGN_PER_CU * cus)
            for tile in windows:
                part = tl.moved_align(case, tile * 4096)
                lo, hi = tl.align_span(part, 4096, n_src)
                span = source.download(np.uint8, 2 * (hi - lo), offset=2 * lo)
                want, wrec = ar.align(span, *tl.on_span(part, lo), *tables, 4096)
                got = out.read(np.uint8, 2 * 4096, 2 * tile * 4096)
                same_bytes(got, want, f"align at the limit: tile {tile}")
                assert records[tile].tobytes() == wrec[0].tobytes(), f"align at the limit: record {tile}: {records[tile]} for {wrec[0]}"
                if tile >= LIMIT_TILES - 2:                    # the position has left the source: mid level, every sample an edge
                    assert np.all(got == 128) and int(records[tile]["n_edge"]) == 4096, tile
                elif tile:
                    assert int(records[tile]["n_edge"]) == 0 and np.unique(got).size > 16, tile
            assert int(records[0]["n_edge"]) > 0, "the range starts in front of the source"
        finally:
            freed(out, rec)
