"""The tracking loops (gj_track_dev, include/gpsjam.h) restated with integers, and the inputs and constants of their tests.
Not a test module: tests/test_track_host.py and tests/track/test_round6_gpu.py import it.

    (E, P, L) = the bank's records of one epoch of B samples at taps (+d, 0, -d), with the channel as it stands
    e = angle(P);  c = floor((|E| - |L|) 2^16 / (|E| + |L|))         angle and length by a 16-step CORDIC in int64
    dn = floor((pll_p (e - e_prev) + pll_i e + fll f) / 2^32);  dc = floor((dll_p (c - c_prev) + dll_i c) / 2^24)
    advance the phases by B old steps;  carr_step -= dn;  code_step = clamp(code_step + dc + aid)

``brute`` is the definition with Python ints on ``corr_restatement.brute``; ``track`` the same per epoch on
``corr_restatement.bank`` for long captures.  A STATE is a tuple of thirteen ints in the order of gj_track_state
(code_phase, code_step, carr_phase, carr_step, code_row, 0, carr_nco, start, e_prev, c_prev, primed, 0, 0); PARAMS are
(spacing, aid_div, pll_p, pll_i, fll, dll_p, dll_i); a RECORD is the twelve ints of gj_track_epoch (E_I, E_Q, P_I, P_Q,
L_I, L_Q, carr_phase, carr_step, code_phase, code_step, e, c).  Everything is exact: the GPU is held to every bit of
every record and every state.  The float chain (gpsjam/track.py) is NOT restated: the tests feed it these integers.
"""
import functools
import math

import numpy as np

import corr_restatement as cr
from gpsjam import gnss, postcorr

MAX_CHANNELS, MAX_EPOCHS, MAX_GAIN = 4096, 1 << 17, 1 << 30
PLL_SHIFT, DLL_SHIFT = 32, 24
# the table from the formula; tests/test_track_host.py holds the header's integers to it
ATAN = tuple(int(math.floor(math.atan(2.0 ** -k) / (2.0 * math.pi) * 2.0 ** 32 + 0.5)) for k in range(16))
ANGLE_BOUND = sum(ATAN)                      # 1 191 629 338
CORDIC_GAIN = 1.6468                         # prod sqrt(1 + 4^-k), to four places
# The largest errors of ``cordic`` that tests/test_track_host.py measures over 10^5 random vectors of |v| >= 1000 up to the
# record bound, the axes among them; that test re-measures each to within 10 % and prints it.
CORDIC_ERROR_ANGLE = 6.16e-6                 # cycles, against math.atan2 of the folded vector
CORDIC_ERROR_LENGTH = 3.0e-5                 # relative, against 2^8 CORDIC_GAIN |v|


def wrap64(v):
    return (int(v) + 2 ** 63) % 2 ** 64 - 2 ** 63


def cordic(I, Q):
    """(angle in 2^-32 cycles, length) of the vector (I, Q), folded into the right half plane: the header's CORDIC."""
    x, y, z = int(I) << 8, int(Q) << 8, 0
    if x == 0 and y == 0:
        return 0, 0                          # a rule of its own: the steps alone would turn by the whole table
    if x < 0:
        x, y = -x, -y
    for k in range(16):
        if y >= 0:
            x, y, z = x + (y >> k), y - (x >> k), z + ATAN[k]
        else:
            x, y, z = x - (y >> k), y + (x >> k), z - ATAN[k]
    return z, x


def state(channel, start=0):
    """A fresh state: the channel (six ints) at sample first_sample + start, everything else 0."""
    return tuple(int(v) for v in channel) + (0, int(start), 0, 0, 0, 0, 0)


def state_bad(s, n_code_rows, n_epochs, B, n_samples):
    """The header's rule for a bad channel."""
    code_phase, code_step, carr_phase, carr_step, row, ch_reserved, nco, start, e_prev, c_prev, primed, r0, r1 = s
    return (ch_reserved != 0 or not 0 <= row < n_code_rows or code_phase >= cr.PERIOD or code_step >= cr.MAX_CODE_STEP
            or r0 != 0 or r1 != 0 or primed not in (0, 1) or start + n_epochs * B > n_samples)


def bad_states(s, n_code_rows, n_epochs, B, n_samples):
    """The good state ``s`` made bad in each way the header names, one at a time."""
    s = tuple(s)
    put = lambda at, v: s[:at] + (v,) + s[at + 1:]
    return [put(5, 1), put(4, n_code_rows), put(4, -1), put(0, cr.PERIOD), put(1, cr.MAX_CODE_STEP), put(11, 1), put(12, -1),
            put(10, 2), put(10, -1), put(7, n_samples - n_epochs * B + 1)]


def update(s, E, P, L, params, B):
    """One epoch's loop update: (record, next state) from the three sums [I, Q]."""
    code_phase, code_step, carr_phase, carr_step, row, ch_reserved, nco, start, e_prev, c_prev, primed, r0, r1 = s
    d, aid_div, pll_p, pll_i, fll, dll_p, dll_i = params
    e, _ = cordic(*P)
    _, mE = cordic(*E)
    _, mL = cordic(*L)
    c = ((mE - mL) << 16) // (mE + mL) if mE + mL else 0
    if primed == 0:
        e_prev, c_prev, primed = e, c, 1
    f = e - e_prev
    if f > 2 ** 30:
        f = 2 ** 31 - f
    elif f < -2 ** 30:
        f = -2 ** 31 - f
    acc = pll_p * (e - e_prev) + pll_i * e + fll * f
    assert abs(acc) < 2 ** 63
    dn = acc >> PLL_SHIFT
    dc = (dll_p * (c - c_prev) + dll_i * c) >> DLL_SHIFT
    rec = (int(E[0]), int(E[1]), int(P[0]), int(P[1]), int(L[0]), int(L[1]), carr_phase, carr_step, code_phase, code_step, e, c)
    code_phase = (code_phase + B * code_step) % cr.PERIOD
    carr_phase = (carr_phase + B * carr_step) % 2 ** 32
    nco2 = wrap64(nco - dn)
    aid = nco2 // aid_div - nco // aid_div if aid_div else 0
    carr_step = (carr_step - dn) % 2 ** 32
    code_step = min(max(code_step + dc + aid, 0), cr.MAX_CODE_STEP - 1)
    return rec, (code_phase, code_step, carr_phase, carr_step, row, ch_reserved, nco2, start, e, c, primed, r0, r1)


def _run(sums, raw, first, n, B, n_epochs, codes, states, params):
    d = int(params[0])
    assert B % 16 == 0 and 16 <= B <= cr.MAX_BLOCK and 1 <= n_epochs <= MAX_EPOCHS and n_epochs * B <= n <= cr.MAX_SAMPLES
    assert 1 <= d <= cr.MAX_TAP_OFFSET and params[1] >= 0 and all(abs(g) <= MAX_GAIN for g in params[2:])
    assert 2 * (first + n) <= np.asarray(raw).size
    records, after = [], []
    for s in states:
        s = tuple(int(v) for v in s)
        if state_bad(s, len(codes), n_epochs, B, n):
            records.append(None)
            after.append(s)
            continue
        rows = []
        for m in range(n_epochs):
            got = sums(raw, first + s[7] + m * B, B, B, codes, [s[:6]], (d, 0, -d))[0][0]
            rec, s = update(s, got[0], got[1], got[2], params, B)
            rows.append(rec)
        records.append(rows)
        after.append(s[:7] + (s[7] + n_epochs * B,) + s[8:])
    return records, after


def brute(raw, first, n, B, n_epochs, codes, states, params):
    """The definition sample by sample with Python ints: (records, states after); a bad channel's records are None and
    its state is as it was."""
    return _run(cr.brute, raw, first, n, B, n_epochs, codes, states, params)


def track(raw, first, n, B, n_epochs, codes, states, params):
    """The same on corr_restatement.bank."""
    return _run(cr.bank, raw, first, n, B, n_epochs, codes, states, params)


def gains(pll_hz, fll_hz, dll_hz, block_samples, fs, spacing=1, aid_div=1540):
    """PARAMS from the reference's loop bandwidths (sdrinit.c:196-206), restated apart from gpsjam.track.gains."""
    dt = block_samples / fs

    def second_order(b):
        return (b / 0.53) ** 2, 1.414 * b / 0.53

    w2, aw = second_order(pll_hz)
    w2d, awd = second_order(dll_hz)
    fllw = fll_hz / 0.25
    r = lambda v: int(math.floor(v + 0.5))
    return (spacing, aid_div, r(2.0 * aw / fs * 2.0 ** 32), r(2.0 * w2 * dt / fs * 2.0 ** 32), r(2.0 * math.pi * fllw * dt / fs * 2.0 ** 32),
            r(awd / fs * 2.0 ** 40), r(w2d * dt / fs * 2.0 ** 40))


WIDE, NARROW = (30.0, 200.0, 5.0), (20.0, 50.0, 2.0)      # the reference's two sets: PLL, FLL, DLL bandwidth in Hz


def as_array(records):
    """int64[n_channels][n_epochs][12] of the records of good channels."""
    return np.array(records, np.int64)


def epochs_as_array(rec):
    """The same of gpsjam.TRACK_EPOCH_DTYPE records (any shape)."""
    cols = [rec["early"][..., 0], rec["early"][..., 1], rec["prompt"][..., 0], rec["prompt"][..., 1], rec["late"][..., 0],
            rec["late"][..., 1], rec["carr_phase"], rec["carr_step"], rec["code_phase"], rec["code_step"], rec["e"], rec["c"]]
    return np.stack([np.asarray(c).astype(np.int64) for c in cols], axis=-1)


def states_as_tuples(rec):
    """Thirteen-int tuples of gpsjam.TRACK_STATE_DTYPE records."""
    return [tuple(int(s["ch"][f]) for f in ("code_phase", "code_step", "carr_phase", "carr_step", "code_row", "reserved"))
            + (int(s["carr_nco"]), int(s["start"]), int(s["e_prev"]), int(s["c_prev"]), int(s["primed"]),
               int(s["reserved"][0]), int(s["reserved"][1])) for s in np.asarray(rec).reshape(-1)]


# ---------------------------------------------------------------------------------------------------- loop behaviour
LOOP_B = 2048
LOOP_EPOCHS = 1200
LOOP_PULL_IN = 200
LOOP_SAMPLES = 1202 * LOOP_B
LOOP_PRN, LOOP_CN0, LOOP_SIGMA, LOOP_SEED = 9, 45.0, 12.0, 4242
LOOP_DOPPLER, LOOP_RAMP = 1873.0, 50.0       # Hz at sample 0, Hz/s
LOOP_CODE_INDEX = 1503.81                    # samples after the first at which the code starts
LOOP_GRID_DOPPLER, LOOP_START = 1800.0, 1504 # what the acquisition's grid makes of them
LOOP_WINDOW = 1000                           # the last epochs, over which the figures are taken
# Measured on the CPU by tests/test_track_host.py with this restatement over the last LOOP_WINDOW epochs; that test
# re-measures each to within 10 % and prints it.  The GPU's end-to-end test allows twice the two errors.
LOOP_CPU_DOPPLER_RMS = 2.56                  # Hz, tracked Doppler against the truth at each epoch's middle
LOOP_CPU_LOCK = 0.984                        # sum |I_P| / sum |P|
LOOP_CPU_CN0_TRACKED = 43.44                 # dB-Hz, postcorr.cn0 of the tracked prompts
LOOP_CPU_CN0_OPEN = 43.13                    # dB-Hz, postcorr.cn0 of the open-loop bank's prompts at the grid channel


@functools.lru_cache(maxsize=None)
def loop_capture():
    """LOOP_SAMPLES samples: one PRN under a Doppler ramp, the code rate following the Doppler, random navigation bits
    every 20 code periods, in white noise.  Read-only uint8."""
    rng = np.random.default_rng(LOOP_SEED)
    n = LOOP_SAMPLES
    t = np.arange(n, dtype=np.float64) / cr.FS
    cycles = LOOP_DOPPLER * t + 0.5 * LOOP_RAMP * t * t                       # the integral of the Doppler
    chips = (t - LOOP_CODE_INDEX / cr.FS) * gnss.CA_RATE + cycles * gnss.CA_RATE / postcorr.L1_HZ
    bits = rng.choice((-1.0, 1.0), size=n // (20 * 2046) + 3)
    nav = bits[(np.floor(chips / cr.CODE_LEN).astype(np.int64) + 20) // 20]
    s = cr.amplitude(LOOP_CN0, LOOP_SIGMA) * gnss.ca_code(LOOP_PRN)[np.floor(chips % cr.CODE_LEN).astype(np.int64) % cr.CODE_LEN] * nav
    s = s * np.exp(-2j * np.pi * cycles + 0.7j)
    raw = cr.quantise(s + rng.normal(0.0, LOOP_SIGMA, n) + 1j * rng.normal(0.0, LOOP_SIGMA, n))
    raw.setflags(write=False)
    return raw


def loop_codes():
    return postcorr.codes([LOOP_PRN])


def loop_channel():
    """The channel an acquisition on the grid hands over: code phase 0 at LOOP_START, the bin's Doppler."""
    return tuple(postcorr.channel(0, 0.0, LOOP_GRID_DOPPLER, cr.FS))


def loop_truth_doppler(epoch):
    """Hz at the middle of an epoch (an array of epoch numbers)."""
    return LOOP_DOPPLER + LOOP_RAMP * (LOOP_START + (np.asarray(epoch, np.float64) + 0.5) * LOOP_B) / cr.FS


def loop_figures(rec):
    """(Doppler rms error in Hz, lock ratio, C/N0 in dB-Hz) of int64[n_epochs][12] records over their last LOOP_WINDOW."""
    rec = np.asarray(rec, np.int64)
    m = np.arange(rec.shape[0])[-LOOP_WINDOW:]
    w = rec[-LOOP_WINDOW:]
    step = ((w[:, 7] + 2 ** 31) % 2 ** 32 - 2 ** 31).astype(np.float64)
    dop = step / 2.0 ** 32 * cr.FS
    prompts = w[:, 2].astype(np.float64) + 1j * w[:, 3].astype(np.float64)
    rms = float(np.sqrt(np.mean((dop - loop_truth_doppler(m)) ** 2)))
    lock = float(np.abs(prompts.real).sum() / np.abs(prompts).sum())
    return rms, lock, postcorr.cn0(prompts, LOOP_B / cr.FS)


def loop_schedule():
    """[(n_epochs, params)]: the pull-in at WIDE, the rest at NARROW."""
    return [(LOOP_PULL_IN, gains(*WIDE, LOOP_B, cr.FS)), (LOOP_EPOCHS - LOOP_PULL_IN, gains(*NARROW, LOOP_B, cr.FS))]


@functools.lru_cache(maxsize=None)
def loop_track():
    """(int64[LOOP_EPOCHS][12], state after) of the restatement over loop_capture with loop_schedule."""
    raw, codes = loop_capture(), loop_codes()
    states, rows = [state(loop_channel(), LOOP_START)], []
    for n_epochs, params in loop_schedule():
        rec, states = track(raw, 0, LOOP_SAMPLES, LOOP_B, n_epochs, codes, states, params)
        rows += rec[0]
    return np.array(rows, np.int64), states[0]


@functools.lru_cache(maxsize=None)
def loop_open():
    """complex prompts of the open-loop bank at the grid channel over the same epochs."""
    iq = cr.bank(loop_capture(), LOOP_START, LOOP_EPOCHS * LOOP_B, LOOP_B, loop_codes(), [loop_channel()], (0,))
    return iq[0, :, 0, 0].astype(np.float64) + 1j * iq[0, :, 0, 1].astype(np.float64)
