"""The time-domain pulse blanker (gj_blank_dev, include/gpsjam.h) restated in numpy int64, and the inputs and constants
of the blanking tests.  Not a test module: tests/test_blank_host.py and tests/blank/test_round6_gpu.py import it.

    e[t] = (2 I_t - o2)^2 + (2 Q_t - o2)^2,  o2 = 2 offset;  0 outside the range
    S[t] = sum of e[t - W//2 : t - W//2 + W]                     a difference of two cumulative sums
    D[t] = S[t] > floor(4 W threshold)                           threshold as float32, the product in double
    B[t] = any D[t - G : t + G + 1] inside the range             a difference of two cumulative sums of D
    out  = the input where not B; mid-level where B (o2 odd: the two nearest bytes, alternating on first_sample + t)

Everything is exact: the GPU is held to every byte and every record field.
"""
import functools
import math

import numpy as np

import excise_restatement as er
import ridge_restatement as rr

RECORD = np.dtype([("total", np.uint64), ("removed", np.uint64), ("n_blanked", np.int32), ("n_rising", np.int32)])
BLOCK = 4096
FS = er.FS
CONVENTIONS = er.CONVENTIONS                # (127.5, 1/127.5): o2 odd;  (128, 1/128): o2 even


class Blanked:
    """out: uint8[2 n]; records: RECORD[ceil(n / 4096)]; blanked: bool[n]; e, S: int64[n]; T: int or None (never)."""

    def __init__(self, out, records, blanked, e, S, T):
        self.out, self.records, self.blanked, self.e, self.S, self.T = out, records, blanked, e, S, T


def threshold_sum(threshold, window):
    """T = floor(4 W threshold) with the threshold rounded to float32 first; None where nothing is ever blanked."""
    thr = float(np.float32(threshold))
    assert thr >= 0.0, "the library refuses a NaN or negative threshold"
    prod = 4.0 * window * thr
    if math.isinf(prod) or prod >= 2.0 ** 63:
        return None
    return int(math.floor(prod))


def blank(raw, threshold, window=16, guard=8, first_sample=0, n_samples=None, offset=127.5):
    """The definition on the bytes `raw`."""
    raw = np.asarray(raw, np.uint8)
    if n_samples is None:
        n_samples = raw.size // 2 - first_sample
    n, W, G = int(n_samples), int(window), int(guard)
    assert n >= 1 and first_sample + n <= raw.size // 2 and 1 <= W <= 1024 and 0 <= G <= 1024
    o2 = int(round(2 * offset))
    assert o2 == 2 * offset
    src = raw[2 * first_sample:2 * (first_sample + n)]
    i, q = 2 * src[0::2].astype(np.int64) - o2, 2 * src[1::2].astype(np.int64) - o2
    e = i * i + q * q
    t = np.arange(n)
    p = np.concatenate(([0], np.cumsum(e)))
    S = p[np.clip(t - W // 2 + W, 0, n)] - p[np.clip(t - W // 2, 0, n)]
    T = threshold_sum(threshold, W)
    D = np.zeros(n, np.int64) if T is None else (S > T).astype(np.int64)
    c = np.concatenate(([0], np.cumsum(D)))
    B = c[np.clip(t + G + 1, 0, n)] - c[np.clip(t - G, 0, n)] > 0
    if o2 % 2 == 0:
        mid_i = mid_q = np.full(n, o2 // 2)
    else:
        at = first_sample + t
        mid_i, mid_q = (o2 - 1) // 2 + (at & 1), (o2 - 1) // 2 + ((at + 1) & 1)
    out = src.copy()
    out[0::2] = np.where(B, mid_i, src[0::2])
    out[1::2] = np.where(B, mid_q, src[1::2])
    nb = -(-n // BLOCK)
    rec = np.zeros(nb, RECORD)
    rising = B & ~np.concatenate(([False], B[:-1]))
    for b in range(nb):
        s = slice(b * BLOCK, min((b + 1) * BLOCK, n))
        rec[b] = (e[s].sum(), e[s][B[s]].sum(), B[s].sum(), rising[s].sum())
    return Blanked(out, rec, B, e, S, T)


# ---------------------------------------------------------------------------------------------------- parity input
PARITY_FIRST = 5                            # odd on purpose
PARITY_SAMPLES = 3 * BLOCK + 1234           # three whole record blocks and a ragged one: two tiles of the kernel
PARITY_TAIL = 64                            # samples of the capture behind the range: loud, and never to be read
PARITY_SIGMA = rr.NOISE_SIGMA               # 6.25 LSB
PARITY_AMP = 100.0
PARITY_SEED = 731
PARITY_WINDOWS = (1, 2, 16, 63, 1024)
PARITY_GUARDS = (0, 1, 8, 1024)
PARITY_THRESHOLD = 4.0 * 2.0 * PARITY_SIGMA ** 2     # 4 x the noise power, LSB^2
# (first sample, length) of the 100-LSB pulses, relative to the range: at t = 0, across both block seams (the second
# is also the kernel's tile seam), ending on the last sample, one sample long, and pairs of one-sample pulses
# 2 G and 2 G + 2 apart for G = 1, 8 and 1024: at W = 1 the dilation by G joins the first pair of each and leaves a
# sample between the second
PARITY_PULSES = ((0, 40), (BLOCK - 16, 40), (2 * BLOCK - 12, 20), (PARITY_SAMPLES - 20, 20), (1000, 1),
                 (1500, 1), (1502, 1), (1600, 1), (1604, 1),
                 (2000, 1), (2016, 1), (2100, 1), (2118, 1),
                 (4500, 1), (4500 + 2048, 1), (9000, 1), (9000 + 2050, 1))
PARITY_EXTREMES = ((3000, 0, 255), (3001, 255, 0), (3002, 0, 0), (3003, 255, 255), (3100, 255, 255), (3200, 0, 0))   # t, I, Q


@functools.lru_cache(maxsize=None)
def parity_capture():
    """PARITY_FIRST + PARITY_SAMPLES + PARITY_TAIL samples.  Read-only uint8."""
    rng = np.random.default_rng(PARITY_SEED)
    n = PARITY_FIRST + PARITY_SAMPLES + PARITY_TAIL
    z = rr._noise(rng, n, PARITY_SIGMA).astype(np.complex128)
    for at, length in PARITY_PULSES:
        z[PARITY_FIRST + at:PARITY_FIRST + at + length] += PARITY_AMP * np.exp(0.25j * np.pi)
    raw = rr.quantise(z)
    for at, i, q in PARITY_EXTREMES:
        raw[2 * (PARITY_FIRST + at):2 * (PARITY_FIRST + at) + 2] = (i, q)
    # what lies outside the range is as loud as bytes get: e = 0 there all the same
    raw[:2 * PARITY_FIRST:2], raw[1:2 * PARITY_FIRST:2] = 255, 0
    raw[2 * (PARITY_FIRST + PARITY_SAMPLES):] = 255
    raw.setflags(write=False)
    return raw


@functools.lru_cache(maxsize=None)
def parity_reference(window, guard, offset=127.5):
    """The restatement of the parity range, computed once and shared."""
    return blank(parity_capture(), PARITY_THRESHOLD, window, guard, PARITY_FIRST, PARITY_SAMPLES, offset)


# ---------------------------------------------------------------------------------------------------- strictness input
STRICT_I, STRICT_Q, STRICT_SAMPLES, STRICT_WINDOW = 140, 120, 2 * BLOCK, 16
STRICT_E = (2 * STRICT_I - 255) ** 2 + (2 * STRICT_Q - 255) ** 2      # 850 at offset 127.5
STRICT_THRESHOLD = STRICT_E / 4.0                                       # 212.5: exact in float32; T = W e = every full window's sum


def strict_capture():
    raw = np.empty(2 * STRICT_SAMPLES, np.uint8)
    raw[0::2], raw[1::2] = STRICT_I, STRICT_Q
    return raw


# ---------------------------------------------------------------------------------------------------- end to end
# excise_restatement.e2e_capture's satellites, noise and lead-in (the same generator, the same seed: the jammer-free
# capture is er.e2e_capture(None) byte for byte) under a pulse train from sample 2^17 on
E2E_KINDS = ("gated carrier", "gated noise", "gated sweep")
E2E_PRF_HZ, E2E_DUTY, E2E_AMP = 1000.0, 0.3, 110.0
E2E_SWEEP_HZ, E2E_SWEEP_S = 20e6, 10e-6               # the sweep covers 20 MHz in 10 us: 2e12 Hz/s
E2E_NOISE_SEED = 77
E2E_EXCISOR_NFFT, E2E_EXCISOR_RISE_DB = 1024, 12.0    # mitigate.clean, which the blanker must beat on noise and sweep
# mitigate.clean_pulsed's `window` is the blanker's: K4's goes in as onset_window
E2E_ONSET_ARGS = {("onset_window" if k == "window" else k): v for k, v in er.E2E_ONSET_ARGS.items()}
E2E_MIN_LOSS_DB = 5.0                                 # before cleaning every PRN sits at least this far under jammer-free
# The residual cn0 - cn0_free - 10 log10(1 - blanked share of the blocks from 2^17 on), measured on the CPU with this
# restatement and the oracle's acquisition over the three kinds and the three PRNs (tests/test_blank_host.py re-measures
# it and prints every figure): the worst magnitude, and the GPU test's tolerance, twice that.
E2E_CPU_RESIDUAL_MEASURED = 0.435         # gated noise, PRN 3: -0.435 dB; the largest positive one +0.382 dB (PRN 25)
E2E_CPU_RESIDUAL_DB = 0.44
E2E_CN0_TOL_DB = 2.0 * E2E_CPU_RESIDUAL_DB


def e2e_gate(n=er.E2E_AFTER):
    """1 where the jammer is on: the first E2E_DUTY of every period of E2E_PRF_HZ, from sample 2^17 on."""
    t = np.arange(n) / FS
    return (((t * E2E_PRF_HZ) % 1.0) < E2E_DUTY).astype(np.float64)


@functools.lru_cache(maxsize=None)
def e2e_capture(kind):
    """uint8 I/Q of er.E2E_LEAD + er.E2E_AFTER samples; kind: one of E2E_KINDS, or None for er.e2e_capture(None)."""
    from gpsjam import gnss
    if kind is None:
        return er.e2e_capture(None)
    n, m = er.E2E_LEAD + er.E2E_AFTER, er.E2E_AFTER
    rng = np.random.default_rng(4)
    k = np.arange(n)
    z = rng.normal(0, er.E2E_SIGMA, n) + 1j * rng.normal(0, er.E2E_SIGMA, n)
    for prn, dop, delay, amp in er.E2E_SATS:
        chip = ((k - delay) * 1.023e6 / FS) % 1023
        z += amp * gnss.ca_code(prn)[chip.astype(np.int64)] * np.exp(-2j * np.pi * dop * (k / FS))
    gate = e2e_gate(m)
    if kind == "gated carrier":                       # pulsedJammer.py: a carrier at 0 Hz times a square wave
        z[er.E2E_LEAD:] += E2E_AMP * gate * np.exp(0.25j * np.pi)
    elif kind == "gated noise":
        r2 = np.random.default_rng(E2E_NOISE_SEED)
        s = E2E_AMP / math.sqrt(2.0)
        z[er.E2E_LEAD:] += gate * (r2.normal(0, s, m) + 1j * r2.normal(0, s, m))
    elif kind == "gated sweep":                       # from -10 MHz at 2e12 Hz/s, restarted with every pulse: it aliases across
        tp = ((np.arange(m) / FS * E2E_PRF_HZ) % 1.0) / E2E_PRF_HZ        # the 2.048 MHz band once per sample
        rate = E2E_SWEEP_HZ / E2E_SWEEP_S
        phase = 2.0 * np.pi * (-0.5 * E2E_SWEEP_HZ * tp + 0.5 * rate * tp * tp)
        z[er.E2E_LEAD:] += E2E_AMP * gate * np.exp(1j * phase)
    else:
        raise ValueError(kind)
    iq = np.empty(2 * n, np.float64)
    iq[0::2], iq[1::2] = z.real, z.imag
    raw = (np.clip(np.round(iq), -128, 127) + 128).astype(np.uint8)
    raw.setflags(write=False)
    return raw


def e2e_blanked_share(records, n_samples):
    """Share of blanked samples over the record blocks from sample 2^17 on (2^17 is a multiple of the block)."""
    b0 = er.E2E_LEAD // BLOCK
    return float(records["n_blanked"][b0:].sum()) / float(n_samples - er.E2E_LEAD)


def e2e_residual_db(cn0, cn0_free, share):
    """What is left of the C/N0 loss once the samples that were blanked are accounted for."""
    return cn0 - cn0_free - 10.0 * math.log10(1.0 - share)


def compare(got, rec, want, what):
    """GPU bytes and records against a Blanked: all of them equal."""
    assert got.size == want.out.size and rec.size == want.records.size, what
    differ = int(np.sum(got != want.out))
    print(f"{what}: {int(want.blanked.sum())} of {want.blanked.size} samples blanked on {int(want.records['n_rising'].sum())} rising edges, "
          f"{differ} bytes differ")
    for key in RECORD.names:
        np.testing.assert_array_equal(rec[key], want.records[key], err_msg=f"{what} {key}")
    assert differ == 0, (what, differ, np.flatnonzero(got != want.out)[:8])
