"""The correlator bank (gj_corr_bank_dev, include/gpsjam.h) restated with integers, and the inputs and constants of the
post-correlation and spoofing tests.  Not a test module: tests/test_corr_host.py and tests/corr/test_round6_gpu.py import it.

    I, Q = byte - 128;  theta = (carr_phase + t carr_step) mod 2^32;  i = theta >> 28
    wI = C[i] I - S[i] Q;  wQ = S[i] I + C[i] Q;  C[i] = floor(cos(2 pi i / 16) 32 + 0.5);  S[i] = C[(i - 4) & 15]
    chip = floor((code_phase + (t + d) code_step) / 2^32) mod 1023;  c = codes[code_row][chip]
    record (channel, block m, tap j) = (sum wI c, sum wQ c) over t in [m B, (m + 1) B)

``brute`` is the definition sample by sample with Python ints; ``bank`` the same in numpy int64 for long ranges.  The
field check, the carrier index and the chip index stand once, for both and for tests/subtract_restatement.py: the same
operators are exact on a Python int and floor and wrap alike on an int64 array.
Everything is exact: the GPU is held to every bit of every record.  The float chain (gpsjam/postcorr.py,
gpsjam/spoof.py) is NOT restated: the tests feed it these integers.
"""
import functools
import math

import numpy as np

from gpsjam import gnss, postcorr

CODE_LEN = 1023
PERIOD = CODE_LEN << 32
MAX_BLOCK, MAX_TAPS, MAX_TAP_OFFSET, MAX_CHANNELS = 4096, 9, 64, 64
MAX_SAMPLES, MAX_CODE_STEP = 1 << 28, 1 << 34
# the tables from the formula (the reference's SSE2 mixer table); tests/test_corr_host.py holds the header's integers to them
COS = tuple(int(math.floor(math.cos(2.0 * math.pi * i / 16.0) * 32.0 + 0.5)) for i in range(16))
SIN = tuple(COS[(i - 4) & 15] for i in range(16))
W_BOUND = 128 * 46                          # |w| <= 128 (|C| + |S|)
RECORD_BOUND = MAX_BLOCK * W_BOUND          # 24 117 248 < 2.5e7
FS = 2.048e6


def blocks(n, B):
    return -(-int(n) // int(B))


def check_channels(codes, channels):
    """Every field of every channel inside the bounds of gj_corr_channel."""
    for (code_phase, code_step, carr_phase, carr_step, row, reserved) in channels:
        assert reserved == 0 and 0 <= row < len(codes) and 0 <= code_phase < PERIOD and 0 <= code_step < MAX_CODE_STEP
        assert 0 <= carr_phase < 2 ** 32 and 0 <= carr_step < 2 ** 32


def carrier_index(carr_phase, carr_step, t):
    """i = ((carr_phase + t carr_step) mod 2^32) >> 28 of sample t: a Python int, or an int64 array (t carr_step < 2^60)."""
    return ((int(carr_phase) + t * int(carr_step)) & 0xFFFFFFFF) >> 28


def chip_index(code_phase, code_step, t):
    """The chip of sample t, tap offset included (t < 0 at a range's start; the arithmetic shift is the floor): a Python
    int, or an int64 array (|sum| < 2^63)."""
    return ((int(code_phase) + t * int(code_step)) >> 32) % CODE_LEN


def brute(raw, first, n, B, codes, channels, taps):
    """The definition with Python ints: nested lists [channel][block][tap] = [I, Q]."""
    raw = np.asarray(raw, np.uint8)
    check_channels(codes, channels)
    out = []
    for (code_phase, code_step, carr_phase, carr_step, row, _) in channels:
        rec = [[[0, 0] for _ in taps] for _ in range(blocks(n, B))]
        for t in range(n):
            I, Q = int(raw[2 * (first + t)]) - 128, int(raw[2 * (first + t) + 1]) - 128
            i = carrier_index(carr_phase, carr_step, t)
            wI, wQ = COS[i] * I - SIN[i] * Q, SIN[i] * I + COS[i] * Q
            for j, d in enumerate(taps):
                c = int(codes[row][chip_index(code_phase, code_step, t + int(d))])
                rec[t // B][j][0] += wI * c
                rec[t // B][j][1] += wQ * c
        out.append(rec)
    return out


def bank(raw, first, n, B, codes, channels, taps):
    """The definition in numpy int64, a million samples of whole blocks at a time:
    int64[n_channels][n_blocks][n_taps][2]; every value fits int32."""
    src = np.asarray(raw, np.uint8)[2 * first:2 * (first + n)]
    assert src.size == 2 * n and 1 <= n <= MAX_SAMPLES, "the range runs past the capture"
    codes = np.asarray(codes, np.int64)
    cos, sin = np.array(COS, np.int64), np.array(SIN, np.int64)
    out = np.zeros((len(channels), blocks(n, B), len(taps), 2), np.int64)
    check_channels(codes, channels)
    piece = B * max(1, (1 << 20) // B)
    for t0 in range(0, n, piece):
        t1 = min(n, t0 + piece)
        I, Q = src[2 * t0:2 * t1:2].astype(np.int64) - 128, src[2 * t0 + 1:2 * t1:2].astype(np.int64) - 128
        t = np.arange(t0, t1, dtype=np.int64)
        starts = np.arange(0, t1 - t0, B)
        m0 = t0 // B
        for k, (code_phase, code_step, carr_phase, carr_step, row, _) in enumerate(channels):
            i = carrier_index(carr_phase, carr_step, t)
            wI, wQ = cos[i] * I - sin[i] * Q, sin[i] * I + cos[i] * Q
            for j, d in enumerate(taps):
                c = codes[row][chip_index(code_phase, code_step, t + int(d))]
                out[k, m0:m0 + starts.size, j, 0] = np.add.reduceat(wI * c, starts)
                out[k, m0:m0 + starts.size, j, 1] = np.add.reduceat(wQ * c, starts)
    assert np.abs(out).max() <= RECORD_BOUND
    return out


def code_steps():
    """The code steps of the parity tests: 2.048 MS/s (two wraps inside a 4096 block), 0.512 MS/s (about 2 chips per
    sample), the largest allowed, and 0 (one chip throughout)."""
    return (postcorr.channel(0, 0.0, 0.0, 2.048e6)[1], postcorr.channel(0, 0.0, 0.0, 0.512e6)[1], MAX_CODE_STEP - 1, 0)


# ---------------------------------------------------------------------------------------------------- parity input
PARITY_SEED = 3117
PARITY_SAMPLES = 3 * 4096 + 5 + 64          # the longest parity range (B = 4096, n = 3 B + 5) and an odd start's room
PARITY_PRNS = (3, 11, 25)


@functools.lru_cache(maxsize=None)
def parity_capture():
    """PARITY_SAMPLES samples: PRN 11 at 2.048 MS/s under loud noise, the four corners of the byte range among the
    samples.  Read-only uint8."""
    rng = np.random.default_rng(PARITY_SEED)
    n = PARITY_SAMPLES
    t = np.arange(n)
    chip = ((t - 37) * gnss.CA_RATE / FS) % CODE_LEN
    z = 20.0 * gnss.ca_code(11)[chip.astype(np.int64)] * np.exp(-2j * np.pi * 1200.0 * t / FS)
    z = z + rng.normal(0.0, 40.0, n) + 1j * rng.normal(0.0, 40.0, n)
    raw = quantise(z).copy()
    raw[10:18] = (0, 0, 0, 255, 255, 0, 255, 255)
    raw[-8:] = (255, 255, 255, 0, 0, 255, 0, 0)
    raw.setflags(write=False)
    return raw


@functools.lru_cache(maxsize=None)
def parity_codes():
    """int16[4][1023]: three C/A codes and a row of ones."""
    rows = [gnss.ca_code(p) for p in PARITY_PRNS] + [np.ones(CODE_LEN, np.int16)]
    out = np.stack(rows).astype(np.int16)
    out.setflags(write=False)
    return out


def parity_channels(n_channels, seed=0):
    """n_channels channels over the edges of every field: the code phases 0 and 1023 2^32 - 1, the four code steps, the
    carrier steps 0, 1, 0xFFFFFFFF and 0x80000000, a carrier phase that crosses a table index inside a block, and two
    channels that share a code row; the rest random."""
    s = code_steps()
    fixed = [(0, s[0], 0, 0, 0, 0),
             (PERIOD - 1, s[0], 5 * 2 ** 28 - 1, 1, 1, 0),                 # index 4 -> 5 at sample 1
             (12345678901, s[1], 0x12345678, 0xFFFFFFFF, 1, 0),            # the same row as the channel above
             (PERIOD - 1, s[2], 9 * 2 ** 28 - 1, 0x80000000, 2, 0),
             (700 << 32, s[3], 0, postcorr.channel(0, 0.0, -3400.0, FS)[3], 2, 0),
             (0, s[2], 0xFFFFFFFF, 1, 0, 0)]
    rng = np.random.default_rng(PARITY_SEED + seed)
    out = list(fixed[:n_channels])
    while len(out) < n_channels:
        out.append((int(rng.integers(0, PERIOD)), int(rng.choice(s[:3])) - int(rng.integers(0, 1000)), int(rng.integers(0, 2 ** 32)),
                    int(rng.integers(0, 2 ** 32)), int(rng.integers(0, 4)), 0))
    return out


def quantise(z):
    """Complex samples -> interleaved uint8 around 128 (rounded, clipped): I = byte - 128 undoes it."""
    iq = np.empty(2 * z.size, np.float64)
    iq[0::2], iq[1::2] = z.real, z.imag
    return np.clip(np.floor(iq + 128.5), 0, 255).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------- end to end
E2E_SAMPLES = 204800                         # 100 ms
E2E_SIGMA = 12.0                             # noise per component, LSB
E2E_SEED = 777
E2E_PRNS = (4, 9, 14, 21, 30, 27)            # five, and a sixth for the mixed pair
E2E_CN0 = (44.0, 45.0, 46.0, 47.0, 48.0, 46.0)                  # dB-Hz
E2E_DOPPLER = (-2431.0, 1873.0, 356.0, 3390.0, -788.0, 2605.0)   # Hz: off the 200 Hz grid by 31 .. 95 Hz
E2E_CODE_INDEX = (211.37, 1503.81, 77.5, 1999.12, 640.66, 1234.25)   # samples after the first at which the code starts
E2E_CARRIER = (0.9, -2.2, 2.9, 0.1, -1.3, 1.7)                  # carrier phase at antenna a, rad
E2E_AUTHENTIC = (0.3, 2.4, -1.9, -0.6, 1.5)                     # inter-antenna phases, rad: no four within one 0.3 rad arc
E2E_SPOOF_PHASE = 1.1
E2E_TOL = 0.15                               # common_direction's half arc
E2E_KINDS = {                                # kind -> (indices into E2E_PRNS, inter-antenna phase of each)
    "authentic": ((0, 1, 2, 3, 4), E2E_AUTHENTIC),
    "spoofed": ((0, 1, 2, 3, 4), (E2E_SPOOF_PHASE,) * 5),
    "mixed": ((0, 1, 2, 3, 4, 5), (0.3, E2E_SPOOF_PHASE, E2E_SPOOF_PHASE, -0.6, E2E_SPOOF_PHASE, E2E_SPOOF_PHASE)),
}
E2E_MIXED_COMMON = tuple(E2E_PRNS[k] for k in (1, 2, 4, 5))
# The largest errors over the PRNs of the three pairs, measured on the CPU by tests/test_corr_host.py with this
# restatement, channels from the truth rounded to the acquisition grid (200 Hz, one sample) and gpsjam.postcorr /
# gpsjam.spoof at their defaults; that test re-measures each to within 10 % and prints it.  The GPU test allows twice
# that: its chain differs only in which cell the real AcqSearch picks.
E2E_CPU_ERROR_PHASE = 0.039                  # rad
E2E_CPU_ERROR_DOPPLER = 0.148                # Hz
E2E_CPU_ERROR_CN0 = 1.91                     # dB
E2E_TOL_PHASE, E2E_TOL_DOPPLER, E2E_TOL_CN0 = 2.0 * E2E_CPU_ERROR_PHASE, 2.0 * E2E_CPU_ERROR_DOPPLER, 2.0 * E2E_CPU_ERROR_CN0


def amplitude(cn0_dbhz, sigma=E2E_SIGMA, fs=FS):
    """Signal amplitude in LSB: C / N0 = A^2 / (2 sigma^2 / fs)."""
    return math.sqrt(10.0 ** (cn0_dbhz / 10.0) * 2.0 * sigma * sigma / fs)


@functools.lru_cache(maxsize=None)
def e2e_pair(kind):
    """(raw_a, raw_b): E2E_SAMPLES samples of two sample-aligned antennas on one clock.  Each PRN is
    A code(t) bit(t) exp(-2j pi f t + j carrier) at antenna a and the same turned by its inter-antenna phase at b; the
    code rate follows the Doppler; navigation bits flip at random every 20 code periods; independent noise."""
    idx, phases = E2E_KINDS[kind]
    rng = np.random.default_rng(E2E_SEED + len(kind))
    n = E2E_SAMPLES
    t = np.arange(n, dtype=np.float64)
    za, zb = np.zeros(n, np.complex128), np.zeros(n, np.complex128)
    for k, psi in zip(idx, phases):
        rate = gnss.CA_RATE * (1.0 + E2E_DOPPLER[k] / 1575.42e6) / FS
        chips = (t - E2E_CODE_INDEX[k]) * rate
        bits = rng.choice((-1.0, 1.0), size=n // (20 * 2046) + 3)
        nav = bits[(np.floor(chips / CODE_LEN).astype(np.int64) + 20) // 20]
        s = amplitude(E2E_CN0[k]) * gnss.ca_code(E2E_PRNS[k])[np.floor(chips % CODE_LEN).astype(np.int64) % CODE_LEN] * nav
        s = s * np.exp(-2j * np.pi * E2E_DOPPLER[k] * t / FS + 1j * E2E_CARRIER[k])
        za += s
        zb += s * np.exp(1j * psi)
    out = []
    for z in (za, zb):
        raw = quantise(z + rng.normal(0.0, E2E_SIGMA, n) + 1j * rng.normal(0.0, E2E_SIGMA, n))
        raw.setflags(write=False)
        out.append(raw)
    return tuple(out)


class GridSearch:
    """What postcorr and spoof ask of a gnss.AcqSearch, answered from the truth rounded to the acquisition grid: the
    Doppler to the nearest 200 Hz bin, the code start to the nearest sample."""

    def __init__(self, kind, fs=FS):
        self.kind, self.fs, self.nsamp = kind, fs, 2048
        self.freqs = gnss.doppler_bins()
        self.prns = [E2E_PRNS[k] for k in E2E_KINDS[kind][0]]

    def search(self, capture, first_sample=0):
        out = []
        for k in E2E_KINDS[self.kind][0]:
            b = int(np.argmin(np.abs(self.freqs - E2E_DOPPLER[k])))
            code = int(math.floor(E2E_CODE_INDEX[k] - first_sample + 0.5)) % self.nsamp
            out.append(gnss.AcqResult(E2E_PRNS[k], True, 10.0, E2E_CN0[k], code, b, float(self.freqs[b]), 1, 0.0, 0.0, 0.0))
        return out


def wrap(x):
    """A phase difference into (-pi, pi]."""
    return (np.asarray(x, np.float64) + np.pi) % (2.0 * np.pi) - np.pi
