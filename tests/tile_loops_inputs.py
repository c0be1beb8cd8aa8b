"""Sizes, cases and helpers of the tile-loop tests.  Not a test module: tests/test_tile_loops_host.py and
tests/tile_loops/test_round6_gpu.py import it.

Five kernels run a fixed number of workgroups, each of which walks the range tile by tile (k_align, k_subtract, k_fine,
k_corr, k_synth).  The tests run them at sizes where EVERY workgroup takes a second tile, past byte 2^32 of a capture,
and at the limit n = 2^28.  Nothing here restates a definition: the helpers only MOVE the arguments of the existing
restatements (tests/align_restatement.py, corr_restatement.py, subtract_restatement.py) to a sub-range, and
tests/test_tile_loops_host.py holds every one of them to the restatement of the whole range."""
import numpy as np

import align_restatement as ar
import corr_restatement as cr

ALIGN_TILE, SUB_TILE, FINE_TILE = 4096, 4096, 8192      # samples of a workgroup's tile
SYNTH_GROUP, SYNTH_THREADS = 8, 256                      # samples of a thread and threads of a block of k_synth
LIMIT = 1 << 28                                          # the largest n of gj_corr_bank_dev, gj_subtract_dev and gj_align_dev
M32 = 0xFFFFFFFF


def corr_tile(B):
    """Samples of a tile of k_corr: as many whole blocks as fit 4096."""
    return (4096 // int(B)) * int(B)


def looping_tiles(cus):
    """Tiles of a run in which every workgroup of a grid of at most 4 per CU takes a second tile and three of them a
    third; at 8 per CU three workgroups would still take a second."""
    return 8 * int(cus) + 3


def moved_channel(channel, t1):
    """The corr / subtract channel (code_phase, code_step, carr_phase, carr_step, row, reserved) whose sample 0 is the
    given channel's sample t1: Python ints throughout."""
    code_phase, code_step, carr_phase, carr_step, row, reserved = (int(v) for v in channel)
    return ((code_phase + int(t1) * code_step) % cr.PERIOD, code_step, (carr_phase + int(t1) * carr_step) % 2 ** 32, carr_step, row, reserved)


def moved_align(case, n1):
    """The align case (pos0, pos_step, rot_phase, rot_step) whose output 0 is the given case's output n1."""
    pos0, step, phase, rot_step = (int(v) for v in case)
    return (pos0 + int(n1) * step, step, (phase + int(n1) * rot_step) & M32, rot_step)


def align_span(case, n_out, n_src):
    """[lo, hi): the source samples that outputs 0 .. n_out - 1 of ``case`` read (16 taps from k - 7), cut to the source.
    Where lo > 0 the first tap of the first output is sample lo itself, and where hi < n_src the last tap of the last
    output is sample hi - 1: the restatement on source[lo:hi] counts the same edge samples as on the whole source.  The
    span is never empty (ar.align wants a sample): a range that lies wholly outside keeps the source's nearest sample,
    which none of its taps reaches."""
    pos0, step = int(case[0]), int(case[1])
    k0 = (pos0 + (1 << 23)) >> 32
    k1 = (pos0 + (int(n_out) - 1) * step + (1 << 23)) >> 32
    lo = min(max(0, k0 - 7), int(n_src) - 1)
    return lo, max(lo + 1, min(int(n_src), k1 + 9))


def on_span(case, lo):
    """``case`` on a source that starts ``lo`` samples later."""
    return (int(case[0]) - (int(lo) << 32),) + tuple(int(v) for v in case[1:])


def align_in_pieces(raw, case, taps, rot, n_out, piece=64 * ALIGN_TILE):
    """ar.align of the whole range, made ``piece`` outputs (whole tiles) at a time, each on the span of the source it
    reads: the same bytes and records (tests/test_tile_loops_host.py), a fraction of the memory."""
    assert piece % ar.BLOCK == 0
    raw = np.asarray(raw, np.uint8)
    out, rec = [], []
    for n1 in range(0, int(n_out), piece):
        m = min(piece, int(n_out) - n1)
        part = moved_align(case, n1)
        lo, hi = align_span(part, m, raw.size // 2)
        o, r = ar.align(raw[2 * lo:2 * hi], *on_span(part, lo), taps, rot, m)
        out.append(o)
        rec.append(r)
    return np.concatenate(out), np.concatenate(rec)


def limit_windows(n_tiles, slots):
    """The tiles of a run of ``n_tiles`` that the tests at the limit compare, on a grid of ``slots`` workgroups: the
    first two, those around a workgroup's second and third tile, the middle, the last two and one at a third.  A fixed
    list, sorted, without repeats, inside the run."""
    T, S = int(n_tiles), int(slots)
    want = [0, 1, S - 1, S, S + 1, 2 * S - 1, 2 * S, 2 * S + 1, T // 2 - 1, T // 2, T - 2, T - 1, T // 3]
    return sorted({t for t in want if 0 <= t < T})


def sparse_capture(n_samples, windows):
    """uint8[2 n_samples], zero but for ``windows`` = {first sample: bytes}.  The zeros are never touched, so only the
    windows' pages are ever resident: a restatement that takes (raw, first) can be given first > 2^31."""
    raw = np.zeros(2 * int(n_samples), np.uint8)
    for first, data in windows.items():
        raw[2 * int(first):2 * int(first) + len(data)] = data
    return raw


def random_capture(n_samples, seed):
    """uint8[2 n_samples] from one seeded stream: no two tiles alike."""
    return np.random.default_rng(seed).integers(0, 256, 2 * int(n_samples), dtype=np.uint8)


def limit_channels():
    """The two channels of the runs at n = 2^28: the largest code step from the last phase of the period, so that
    t code_step reaches 2^62 as csrc/replica.h says, and a realistic one."""
    from gpsjam import postcorr
    return [(cr.PERIOD - 1, cr.MAX_CODE_STEP - 1, 0x9E3779B9, 0xFFFFFFFF, 1, 0), tuple(postcorr.channel(2, 511.25, -3400.0, cr.FS, 0.77))]


# n_out = 2^28 at the fastest step, from a few samples in front of the source: the position ends 2^20 samples past a
# source of 2^28 + 64 samples
LIMIT_ALIGN_CASE = (-(5 << 32) - 0x4CCCCCCC, ar.ONE + ar.MAX_DRIFT, 0x12345678, 0x9E3779B9)
LIMIT_SOURCE_SAMPLES = LIMIT + 64
