"""The subtraction of tracked signals (gj_subtract_track_dev, include/gpsjam.h) restated with integers, and the inputs,
the GPU run helper and the judge of its tests.  Not a test module: tests/test_subtract_track_host.py and
tests/subtract_track/test_round6_gpu.py import it.

    r = t - start;  the channel is silent at t if r < 0 or r >= E B;  m, u = r div B, r mod B;  rec = records[ch][m]
    silent too if rec.code_phase >= 1023 2^32 or rec.code_step >= 2^34
    chip = ((rec.code_phase + u rec.code_step) mod 1023 2^32) >> 32;  i = ((rec.carr_phase + u rec.carr_step) mod 2^32) >> 28
    a = clamp(amp[ch][m], -2^19, +2^19);  R, d, q, the byte and the records: subtract_restatement's

A CHANNEL is (start, code_row); RECORDS are gpsjam.TRACK_EPOCH_DTYPE[n_channels][E], the bytes gj_track_dev writes and
gj_subtract_track_dev reads, of which only carr_phase, carr_step, code_phase and code_step count.  ``brute`` is the
definition sample by sample with Python ints; ``subtract_tracked`` the same in numpy int64, with a sample window for
long ranges.  Everything is exact: the GPU is held to every byte and every record.  The float chain
(gpsjam.track.amplitudes, gpsjam.spoof.remove_tracked) is NOT restated: the tests feed it these integers.
"""
import numpy as np

import corr_restatement as cr
import gpsjam
import gpu_lib
import subtract_restatement as sr
import track_restatement as tr
from gpsjam import gnss, postcorr

EPOCH = gpsjam.TRACK_EPOCH_DTYPE
MAX_AMP, DITHER, SUB_BLOCK = sr.MAX_AMP, sr.DITHER, sr.SUB_BLOCK


def table_bad(codes, channels, E, B, n):
    """The header's rule for a launch that writes nothing."""
    return any(not 0 <= row < len(codes) or start + E * B > n for start, row in channels)


def record_bad(rec):
    """The header's rule for a record that adds nothing (a scalar record)."""
    return int(rec["code_phase"]) >= cr.PERIOD or int(rec["code_step"]) >= cr.MAX_CODE_STEP


def brute(raw, first, n, B, E, codes, channels, records, amps, flags=0, seed=0):
    """The definition with Python ints: (bytes list[2 n], records list of (total, removed, n_clipped)).  ``raw`` is
    indexed byte by byte: anything with __getitem__ serves."""
    assert not table_bad(codes, channels, E, B, n)
    out, blocks = [], [[0, 0, 0] for _ in range(sr.blocks(n))]
    for t in range(n):
        R = [0, 0]
        for ch, (start, row) in enumerate(channels):
            r = t - start
            if r < 0 or r >= E * B:
                continue
            m, u = r // B, r % B
            rec = records[ch][m]
            if record_bad(rec):
                continue
            chip = ((int(rec["code_phase"]) + u * int(rec["code_step"])) % cr.PERIOD) >> 32
            i = ((int(rec["carr_phase"]) + u * int(rec["carr_step"])) % 2 ** 32) >> 28
            aI, aQ = (max(-MAX_AMP, min(MAX_AMP, int(v))) for v in amps[ch][m])
            c = -1 if int(codes[row][chip]) < 0 else 1
            R[0] += c * (aI * cr.COS[i] + aQ * cr.SIN[i])
            R[1] += c * (aQ * cr.COS[i] - aI * cr.SIN[i])
        for comp in (0, 1):
            d = sr.dither_one(first + t, comp, seed) if flags & DITHER else 32768
            assert -2 ** 31 <= R[comp] + d < 2 ** 31
            q = (R[comp] + d) // 65536
            x = int(raw[2 * (first + t) + comp])
            want = x - q
            got = max(0, min(255, want))
            out.append(got)
            b = blocks[t // SUB_BLOCK]
            b[0] += (x - 128) ** 2
            b[1] += (x - got) ** 2
            b[2] += got != want
    return out, [tuple(b) for b in blocks]


def replica(lo, hi, B, E, codes, channels, records, amps):
    """int64[hi - lo][2]: (R_I, R_Q) of samples lo .. hi - 1 of the range."""
    records = np.asarray(records).reshape(len(channels), E)
    amps = np.clip(np.asarray(amps, np.int64).reshape(len(channels), E, 2), -MAX_AMP, MAX_AMP)
    code_sign = np.where(np.asarray(codes, np.int64) < 0, -1, 1)
    cos, sin = np.array(cr.COS, np.int64), np.array(cr.SIN, np.int64)
    R = np.zeros((hi - lo, 2), np.int64)
    piece = 1 << 20
    for t0 in range(lo, hi, piece):
        t = np.arange(t0, min(hi, t0 + piece), dtype=np.int64)
        for ch, (start, row) in enumerate(channels):
            r = t - int(start)
            live = (r >= 0) & (r < E * B)
            if not live.any():
                continue
            m = np.clip(r // B, 0, E - 1)
            u = np.where(live, r - m * B, 0)
            rec = records[ch][m]
            live &= (rec["code_phase"] < np.uint64(cr.PERIOD)) & (rec["code_step"] < np.uint64(cr.MAX_CODE_STEP))
            code_phase = np.where(live, rec["code_phase"], 0).astype(np.int64)
            code_step = np.where(live, rec["code_step"], 0).astype(np.int64)
            chip = ((code_phase + u * code_step) >> 32) % cr.CODE_LEN               # u code_step < 2^46
            i = ((rec["carr_phase"].astype(np.int64) + u * rec["carr_step"].astype(np.int64)) & 0xFFFFFFFF) >> 28
            c = code_sign[row][chip] * live
            aI, aQ = amps[ch, m, 0], amps[ch, m, 1]
            R[t - lo, 0] += c * (aI * cos[i] + aQ * sin[i])
            R[t - lo, 1] += c * (aQ * cos[i] - aI * sin[i])
    assert np.abs(R).max(initial=0) <= sr.R_BOUND
    return R


def subtract_tracked(raw, first, n, B, E, codes, channels, records, amps, flags=0, seed=0, window=None):
    """The definition in numpy int64: (uint8[2 n], sr.DTYPE[blocks(n)]).  ``window`` = (lo, hi), lo a multiple of 4096
    and hi one or n: the bytes of samples lo .. hi - 1 of the range and the records of their tiles alone."""
    lo, hi = (0, n) if window is None else (int(window[0]), int(window[1]))
    assert 0 <= lo < hi <= n and lo % SUB_BLOCK == 0 and (hi % SUB_BLOCK == 0 or hi == n)
    assert B % 16 == 0 and 16 <= B <= cr.MAX_BLOCK and 1 <= len(channels) <= cr.MAX_CHANNELS and not flags & ~DITHER
    assert 1 <= n <= cr.MAX_SAMPLES and E >= 1 and E * B <= n and not table_bad(codes, channels, E, B, n)
    src = np.asarray(raw[2 * (first + lo):2 * (first + hi)], np.uint8)      # sliced first: ``raw`` may be a stub that holds a far window
    assert src.size == 2 * (hi - lo), "the range runs past the capture"
    R = replica(lo, hi, B, E, codes, channels, records, amps)
    d = sr.dither(first + lo, hi - lo, seed) if flags & DITHER else np.full((hi - lo, 2), 32768, np.int64)
    q = (R + d) >> 16
    x = src.astype(np.int64).reshape(hi - lo, 2)
    want = x - q
    got = np.clip(want, 0, 255)
    starts = np.arange(0, hi - lo, SUB_BLOCK)
    rec = np.zeros(starts.size, sr.DTYPE)
    rec["total"] = np.add.reduceat(((x - 128) ** 2).sum(axis=1), starts)
    rec["removed"] = np.add.reduceat(((x - got) ** 2).sum(axis=1), starts)
    rec["n_clipped"] = np.add.reduceat((got != want).sum(axis=1), starts)
    return got.astype(np.uint8).reshape(-1), rec


# ---------------------------------------------------------------------------------------------------- inputs
def random_records(n_channels, E, seed=0, steps=None):
    """EPOCH[n_channels][E]: every epoch's NCOs drawn anew -- no continuity from one epoch to the next, so that a wrong
    epoch index shows -- and every other field random as well: they are not read.  ``steps``: the code steps to draw
    from (default corr_restatement.code_steps()'s first three, less a little)."""
    rng = np.random.default_rng(5200 + seed + 11 * n_channels + E)
    steps = cr.code_steps()[:3] if steps is None else steps
    rec = np.zeros((n_channels, E), EPOCH)
    for f in ("early", "prompt", "late"):
        rec[f] = rng.integers(-2 ** 31, 2 ** 31, (n_channels, E, 2))
    rec["e"], rec["c"] = rng.integers(-2 ** 31, 2 ** 31, (2, n_channels, E))
    rec["carr_phase"], rec["carr_step"] = rng.integers(0, 2 ** 32, (2, n_channels, E))
    rec["code_phase"] = rng.integers(0, cr.PERIOD, (n_channels, E))
    rec["code_step"] = np.maximum(rng.choice(np.array(steps, np.int64), (n_channels, E)) - rng.integers(0, 1000, (n_channels, E)), 0)
    return rec


def advanced_records(channel, E, B):
    """EPOCH[E]: one constant channel (six ints) advanced by m B samples per epoch, what all-zero gains track."""
    rec = np.zeros(E, EPOCH)
    for m in range(E):
        ch = postcorr.advance(postcorr.Channel(*channel), m * B)
        rec[m]["code_phase"], rec[m]["code_step"], rec[m]["carr_phase"], rec[m]["carr_step"] = ch.code_phase, ch.code_step, ch.carr_phase, ch.carr_step
    return rec


def records_from_rows(rows):
    """EPOCH[...] of track_restatement's int64[...][12] records."""
    rows = np.asarray(rows, np.int64)
    rec = np.zeros(rows.shape[:-1], EPOCH)
    rec["early"], rec["prompt"], rec["late"] = rows[..., 0:2], rows[..., 2:4], rows[..., 4:6]
    rec["carr_phase"], rec["carr_step"], rec["code_phase"], rec["code_step"] = (rows[..., k] for k in (6, 7, 8, 9))
    rec["e"], rec["c"] = rows[..., 10], rows[..., 11]
    return rec


# ---------------------------------------------------------------------------------------------------- the GPU call
def run(dev, capture, first, n, B, E, d_rows, n_rows, channels, records, amps, flags, seed, want_records=True, out_offset=0,
        nbytes=None, d_epochs=None):
    """(uint8[2 n], sr.DTYPE[blocks] or None) through gj_subtract_track_dev, into sentinel-guarded buffers;
    ``out_offset``: bytes by which d_out is moved off its 256-byte aligned place; ``d_epochs``: a device buffer that
    already holds the records, used as it is."""
    table = np.array([tuple(c) for c in channels], gpsjam.SUB_TRACK_CHANNEL_DTYPE)
    amps = np.ascontiguousarray(amps, np.int32)
    assert amps.shape == (len(channels), E, 2)
    d_ch, d_amp = dev.alloc(table.nbytes).upload(table), dev.alloc(amps.nbytes).upload(amps)
    d_rec = None
    if d_epochs is None:
        host = np.ascontiguousarray(records).reshape(-1)
        assert host.dtype == EPOCH and host.size == len(channels) * E
        d_rec = dev.alloc(host.nbytes).upload(host)
    try:
        got, rec = gpu_lib._bytes_and_records(
            dev, n, sr.blocks(n), gpsjam.SUB_DTYPE, want_records,
            lambda d_out, d_blk: dev.subtract_track_dev(capture, capture.nbytes if nbytes is None else nbytes, first, n, B, E, d_rows, n_rows,
                                                        d_ch, len(channels), d_rec if d_epochs is None else d_epochs, d_amp, flags, seed,
                                                        d_out, d_blk), out_offset)
        return got, rec if want_records else None
    finally:
        gpu_lib.freed(d_ch, d_amp, d_rec)


# ---------------------------------------------------------------------------------------------------- end to end
# The judge: what is left of the loop capture's signal (track_restatement.loop_capture: PRN 9 at 45 dB-Hz under a
# 50 Hz/s ramp) in a byte array, read at the TRUTH -- one channel per epoch from the LOOP_* constants through
# postcorr.channel -- against the prompts of PRN 17's code, which is not in the capture, at the same channels.
ABSENT_PRN = 17


def truth_channels():
    """One channel per epoch of the loop capture's signal, at sample LOOP_START + m LOOP_B: the code phase and the
    carrier phase of that sample, the Doppler of the epoch's middle."""
    out = []
    for m in range(tr.LOOP_EPOCHS):
        t = (tr.LOOP_START + m * tr.LOOP_B) / cr.FS
        cycles = tr.LOOP_DOPPLER * t + 0.5 * tr.LOOP_RAMP * t * t
        chips = (t - tr.LOOP_CODE_INDEX / cr.FS) * gnss.CA_RATE + cycles * gnss.CA_RATE / postcorr.L1_HZ
        out.append(postcorr.channel(0, chips, float(tr.loop_truth_doppler(m)), cr.FS, cycles))
    return out


def epoch_prompts(raw, channels, code, first_epoch=0):
    """complex128[len(channels) - first_epoch]: the bank's prompt of every epoch from ``first_epoch`` on, epoch m over the
    LOOP_B samples from LOOP_START + m LOOP_B of ``raw`` at channels[m], with the code row ``code``: the bank's integers
    (corr_restatement), all epochs at once."""
    chans = channels[first_epoch:]
    B = tr.LOOP_B
    lo = tr.LOOP_START + first_epoch * B
    x = np.asarray(raw)[2 * lo:2 * (lo + len(chans) * B)].astype(np.int64).reshape(len(chans), B, 2) - 128
    u = np.arange(B, dtype=np.int64)[None, :]
    col = lambda k: np.array([c[k] for c in chans], np.int64)[:, None]
    i = ((col(2) + u * col(3)) & 0xFFFFFFFF) >> 28
    chip = ((col(0) + u * col(1)) >> 32) % cr.CODE_LEN
    c = np.asarray(code, np.int64)[chip]
    cos, sin = np.array(cr.COS, np.int64)[i], np.array(cr.SIN, np.int64)[i]
    wI, wQ = cos * x[..., 0] - sin * x[..., 1], sin * x[..., 0] + cos * x[..., 1]
    return (wI * c).sum(axis=1).astype(np.float64) + 1j * (wQ * c).sum(axis=1).astype(np.float64)


def residue_db(raw):
    """dB by which the signal's prompt power at the truth stands above the absent PRN's, in the mean |P|^2 over the last
    LOOP_WINDOW epochs of ``raw`` (bytes on the loop capture's sample grid)."""
    chans, at = truth_channels(), tr.LOOP_EPOCHS - tr.LOOP_WINDOW
    own = epoch_prompts(raw, chans, gnss.ca_code(tr.LOOP_PRN), at)
    absent = epoch_prompts(raw, chans, gnss.ca_code(ABSENT_PRN), at)
    return float(10.0 * np.log10(np.mean(np.abs(own) ** 2) / np.mean(np.abs(absent) ** 2)))


def open_loop_amplitudes(prompts):
    """int32[1][epochs][2]: one amplitude per epoch from open-loop prompts, by gpsjam.track.amplitudes' rule."""
    alpha = np.asarray(prompts, np.complex128) / (tr.LOOP_B * postcorr.MIXER_GAIN) * 2.0 ** postcorr.SUB_FRAC
    return np.stack([np.floor(alpha.real + 0.5), np.floor(alpha.imag + 0.5)], axis=-1).astype(np.int32)[None]


# Measured on the CPU by tests/test_subtract_track_host.py: track_restatement.loop_track()'s records through
# gpsjam.track.amplitudes and subtract_tracked above, and the open-loop variant -- track_restatement.loop_channel() held
# for all 1200 epochs, one amplitude per epoch from loop_open() -- through subtract_restatement.subtract; dither on, seed
# 0.  That test re-measures each to within 10 % and prints it.  The untouched capture reads 15.31 dB on the same yardstick;
# the loop capture is 1.2 s long, and the open-loop replica, 133 Hz off at its end, still removes most of the signal.  The
# GPU's end-to-end test allows twice the tracked figure: its chain differs only in the acquisition's cell.
E2E_CPU_RESIDUE_TRACKED_DB = 1.37            # dB over the absent PRN's floor, replicas at the tracked NCOs
E2E_CPU_RESIDUE_OPEN_DB = 5.07               # ... at the grid channel, open loop
