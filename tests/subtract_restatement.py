"""The counterfeit-signal subtraction (gj_subtract_dev, include/gpsjam.h) restated with integers, and the inputs and
constants of its tests.  Not a test module: tests/test_subtract_host.py and tests/subtract/test_round6_gpu.py import it.

    a(ch, m) = clamp(amp[ch][m], -2^19, +2^19), m = t // B;  c, i = the bank's chip at tap 0 and carrier index (corr_restatement)
    R_I = sum_ch c (aI C[i] + aQ S[i]);  R_Q = sum_ch c (aQ C[i] - aI S[i])
    d = 32768, or with the dither h(key) >> 16:  k = 2 (first + t) + comp;  key = (k mod 2^32) ^ ((k >> 32) 0x9e3779b9 mod 2^32) ^ seed
    h: v ^= v >> 16; v *= 0x7feb352d; v ^= v >> 15; v *= 0x846ca68b; v ^= v >> 16   (mod 2^32)
    q = floor((R + d) / 65536);  out = clamp(in - q, 0, 255)
    record per 4096 samples: total = sum (I - 128)^2 + (Q - 128)^2, removed = sum (in - out)^2, n_clipped = bytes the clamp changed

``brute`` is the definition sample by sample with Python ints; ``subtract`` the same in numpy int64 for long ranges.
Everything is exact: the GPU is held to every byte and every record.  The float chain (gpsjam.postcorr.amplitudes,
gpsjam.spoof.remove, gpsjam.mitigate.clean_spoofed) is NOT restated: the tests feed it these integers.

The end-to-end inputs are tests/peaks_restatement.py's overpowered pair and tests/corr_restatement.py's authentic pair,
read-only.
"""
import numpy as np

import corr_restatement as cr

SUB_BLOCK, FRAC, MAX_AMP, DITHER = 4096, 16, 1 << 19, 1
R_BOUND = cr.MAX_CHANNELS * MAX_AMP * 46            # 1 543 503 872; + 65535 < 2^31
DTYPE = np.dtype([("total", np.uint64), ("removed", np.uint64), ("n_clipped", np.int32), ("reserved", np.int32)])
M32 = 0xFFFFFFFF


def blocks(n):
    return -(-int(n) // SUB_BLOCK)


def hash32(v):
    """The header's h on one Python int."""
    v ^= v >> 16
    v = (v * 0x7feb352d) & M32
    v ^= v >> 15
    v = (v * 0x846ca68b) & M32
    v ^= v >> 16
    return v


def dither_one(sample, comp, seed):
    """d of component ``comp`` of the ABSOLUTE sample ``sample``, with Python ints."""
    k = (2 * sample + comp) % 2 ** 64
    key = (k & M32) ^ (((k >> 32) * 0x9e3779b9) & M32) ^ (seed & M32)
    return hash32(key) >> 16


def dither(first, n, seed):
    """int64[n][2]: d of the samples first .. first + n - 1 (absolute) and both components, in numpy uint64."""
    k = (np.uint64(2) * (np.uint64(first) + np.arange(n, dtype=np.uint64)))[:, None] + np.arange(2, dtype=np.uint64)[None, :]
    m = np.uint64(M32)
    v = (k & m) ^ (((k >> np.uint64(32)) * np.uint64(0x9e3779b9)) & m) ^ np.uint64(seed & M32)
    v ^= v >> np.uint64(16)
    v = (v * np.uint64(0x7feb352d)) & m
    v ^= v >> np.uint64(15)
    v = (v * np.uint64(0x846ca68b)) & m                # v < 2^32 and the constant < 2^32: the product fits uint64
    v ^= v >> np.uint64(16)
    return (v >> np.uint64(16)).astype(np.int64)


def brute(raw, first, n, B, codes, channels, amps, flags=0, seed=0):
    """The definition with Python ints: (bytes list[2 n], records list of (total, removed, n_clipped))."""
    raw = np.asarray(raw, np.uint8)
    cr.check_channels(codes, channels)
    out, rec = [], [[0, 0, 0] for _ in range(blocks(n))]
    for t in range(n):
        R = [0, 0]
        for ch, (code_phase, code_step, carr_phase, carr_step, row, _) in enumerate(channels):
            aI, aQ = (max(-MAX_AMP, min(MAX_AMP, int(v))) for v in amps[ch][t // B])
            i = cr.carrier_index(carr_phase, carr_step, t)
            c = -1 if int(codes[row][cr.chip_index(code_phase, code_step, t)]) < 0 else 1
            R[0] += c * (aI * cr.COS[i] + aQ * cr.SIN[i])
            R[1] += c * (aQ * cr.COS[i] - aI * cr.SIN[i])
        for comp in (0, 1):
            d = dither_one(first + t, comp, seed) if flags & DITHER else 32768
            assert -2 ** 31 <= R[comp] + d < 2 ** 31
            q = (R[comp] + d) // 65536                  # Python's floor division
            x = int(raw[2 * (first + t) + comp])
            want = x - q
            got = max(0, min(255, want))
            out.append(got)
            r = rec[t // SUB_BLOCK]
            r[0] += (x - 128) ** 2
            r[1] += (x - got) ** 2
            r[2] += got != want
    return out, [tuple(r) for r in rec]


def replica(first, n, B, codes, channels, amps):
    """int64[n][2]: (R_I, R_Q) of every sample of the range."""
    cr.check_channels(codes, channels)
    amps = np.clip(np.asarray(amps, np.int64).reshape(len(channels), -1, 2), -MAX_AMP, MAX_AMP)
    assert amps.shape[1] == cr.blocks(n, B), "one amplitude pair per channel and block"
    code_sign = np.where(np.asarray(codes, np.int64) < 0, -1, 1)
    cos, sin = np.array(cr.COS, np.int64), np.array(cr.SIN, np.int64)
    R = np.zeros((n, 2), np.int64)
    piece = 1 << 20
    for t0 in range(0, n, piece):
        t = np.arange(t0, min(n, t0 + piece), dtype=np.int64)
        m = t // B
        for ch, (code_phase, code_step, carr_phase, carr_step, row, _) in enumerate(channels):
            i = cr.carrier_index(carr_phase, carr_step, t)
            c = code_sign[row][cr.chip_index(code_phase, code_step, t)]
            aI, aQ = amps[ch, m, 0], amps[ch, m, 1]
            R[t, 0] += c * (aI * cos[i] + aQ * sin[i])
            R[t, 1] += c * (aQ * cos[i] - aI * sin[i])
    assert np.abs(R).max(initial=0) <= R_BOUND
    return R


def subtract(raw, first, n, B, codes, channels, amps, flags=0, seed=0):
    """The definition in numpy int64: (uint8[2 n], DTYPE[blocks(n)])."""
    src = np.asarray(raw, np.uint8)[2 * first:2 * (first + n)]
    assert src.size == 2 * n and 1 <= n <= cr.MAX_SAMPLES, "the range runs past the capture"
    assert B % 16 == 0 and 16 <= B <= cr.MAX_BLOCK and 1 <= len(channels) <= cr.MAX_CHANNELS and not flags & ~DITHER
    R = replica(first, n, B, codes, channels, amps)
    d = dither(first, n, seed) if flags & DITHER else np.full((n, 2), 32768, np.int64)
    q = (R + d) >> 16                                    # arithmetic shift of int64: the floor
    x = src.astype(np.int64).reshape(n, 2)
    want = x - q
    got = np.clip(want, 0, 255)
    starts = np.arange(0, n, SUB_BLOCK)
    rec = np.zeros(starts.size, DTYPE)
    rec["total"] = np.add.reduceat(((x - 128) ** 2).sum(axis=1), starts)
    rec["removed"] = np.add.reduceat(((x - got) ** 2).sum(axis=1), starts)
    rec["n_clipped"] = np.add.reduceat((got != want).sum(axis=1), starts)
    return got.astype(np.uint8).reshape(-1), rec


def random_amps(n_channels, n_blocks, bound, seed=0):
    """int32[n_channels][n_blocks][2], uniform within +-bound."""
    rng = np.random.default_rng(4100 + seed + 7 * n_channels + n_blocks)
    return rng.integers(-bound, bound + 1, (n_channels, n_blocks, 2)).astype(np.int32)


# ---------------------------------------------------------------------------------------------------- end to end
# Measured on the CPU by tests/test_subtract_host.py: gpsjam.mitigate.clean_spoofed on peaks_restatement.overpowered_pair()
# with candidates from the truth rounded to the acquisition grid (peaks_restatement.TruthSearch), the bank and the
# subtraction restated (corr_restatement.bank, subtract above), gpsjam.postcorr / gpsjam.spoof at their defaults.  That
# test re-measures each to within 10 % and prints it.
#
# What that run gave, on cleaned antenna a, over the oracle's 10-step surfaces of 71 x 2048 cells (gamma = 3.928):
#   PRN            4      9      14     21     30
#   first peak     14.70  22.48  21.53  39.56  36.45   times the floor, each at the authentic cell
#   second peak    3.00   2.93   3.20   3.27   3.34
#   C/N0 cleaned   43.40  43.67  45.75  46.87  47.62   dB-Hz (truth 44 .. 48; 41.9 .. 45.8 before cleaning)
# The ten suppressions were 20.0 .. 29.1 dB, the counterfeit signals' moments C/N0 fell from 44.9 .. 52.0 to 28.8 .. 33.1
# dB-Hz, no byte was clipped, and 18.9 % of the capture's power went out with the five signals.
E2E_CPU_MIN_SUPPRESSION_DB = 19.99           # the smallest of the ten removals (five counterfeit signals, two antennas), in the mean |prompt|^2
# the largest errors of the AUTHENTIC signals on the cleaned pair: spoof.scan with corr_restatement.GridSearch("authentic")
E2E_CPU_ERROR_PHASE = 0.0259                 # rad (PRN 14)
E2E_CPU_ERROR_CN0 = 1.33                     # dB (PRN 9; 2.57 under the copies: peaks_restatement.E2E_CPU_ERROR_CN0)
E2E_TOL_PHASE, E2E_TOL_CN0 = 2.0 * E2E_CPU_ERROR_PHASE, 2.0 * E2E_CPU_ERROR_CN0
E2E_GPU_MIN_SUPPRESSION_DB = E2E_CPU_MIN_SUPPRESSION_DB - 6.0   # a factor of two on the residual amplitude
