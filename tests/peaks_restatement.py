"""The K-peak search (gj_acq_peaks_dev, include/gpsjam.h) restated with a plain argmax, and the inputs and constants of the
same-PRN spoofing tests.  Not a test module: tests/test_peaks_host.py and tests/peaks/test_round6_gpu.py import it.

    peak j  = the first maximum (smallest flat index f nsamp + c) over the cells whose column no earlier peak excludes
    a peak at column c0 excludes the columns c with min(|c - c0|, nsamp - |c - c0|) <= guard, in every row
    floor   = the mean of the cells in the columns no peak excludes

``top_k`` masks excluded cells one by one and takes numpy's argmax of the whole surface: no per-column records, none of
the kernel's structure.  Peaks are exact; the floor is numpy's sum, which the GPU is held to within
n_cells 2^-53 relative: the bound for ANY order of adding non-negative doubles.

The end-to-end pair ("overpowered") reuses tests/corr_restatement.py's constants and signal model, read-only.
"""
import functools
import math

import numpy as np

import corr_restatement as cr
from gpsjam import gnss

MAX_PEAKS = 8
MIN_SAMP, MAX_SAMP, MAX_FREQ = 8, 65536, 4096


def excluded(nsamp, code_index, guard):
    """bool[nsamp]: the columns a peak at ``code_index`` excludes."""
    d = np.abs(np.arange(nsamp) - int(code_index))
    return np.minimum(d, nsamp - d) <= int(guard)


def top_k(surface, k, guard):
    """(peaks, (mean, kept)) of ONE PRN's surface float64[n_freq][nsamp]: peaks = [(power, code_index, freq_index)] * k."""
    P = np.asarray(surface, np.float64)
    n_freq, nsamp = P.shape
    assert MIN_SAMP <= nsamp <= MAX_SAMP and 1 <= n_freq <= MAX_FREQ and 1 <= k <= MAX_PEAKS and guard >= 0
    assert k * (2 * guard + 1) < nsamp
    out_cols = np.zeros(nsamp, bool)
    peaks = []
    for _ in range(k):
        masked = np.where(out_cols[None, :], -np.inf, P)
        flat = int(np.argmax(masked))                      # the first maximum in flat order
        f, c = divmod(flat, nsamp)
        peaks.append((float(P[f, c]), c, f))
        out_cols |= excluded(nsamp, c, guard)
    kept = int((~out_cols).sum())
    return peaks, (float(P[:, ~out_cols].sum() / (n_freq * kept)), kept)


def top_k_all(surfaces, k, guard):
    """``top_k`` of every PRN of float64[n_prn][n_freq][nsamp]: (power[n_prn][k], code[n_prn][k], freq[n_prn][k],
    mean[n_prn], kept[n_prn])."""
    rows = [top_k(s, k, guard) for s in surfaces]
    power = np.array([[p[0] for p in r[0]] for r in rows], np.float64)
    code = np.array([[p[1] for p in r[0]] for r in rows], np.int32)
    freq = np.array([[p[2] for p in r[0]] for r in rows], np.int32)
    return power, code, freq, np.array([r[1][0] for r in rows]), np.array([r[1][1] for r in rows], np.int32)


def floor_bound(n_freq, kept):
    """Relative bound between two orders of adding n_freq * kept non-negative doubles."""
    return n_freq * kept * 2.0 ** -53


@functools.lru_cache(maxsize=None)
def random_surfaces(n_prn, n_freq, nsamp, seed=0):
    """Sums of ten unit exponentials (what a noise cell is), with a few cells raised; read-only."""
    rng = np.random.default_rng(9000 + 131 * n_prn + 17 * n_freq + nsamp + seed)
    P = rng.gamma(10.0, 1.0, (n_prn, n_freq, nsamp))
    for p in range(n_prn):
        for _ in range(3):
            P[p, rng.integers(n_freq), rng.integers(nsamp)] *= 4.0
    P.setflags(write=False)
    return P


# ---------------------------------------------------------------------------------------------------- end to end
# Every E2E PRN of corr_restatement is in the air twice: authentic as in cr.e2e_pair("authentic"), and a counterfeit copy
# 4 dB stronger, at another code phase and (but for PRN 14) another Doppler bin, all copies from ONE direction.
SPOOF_GAIN_DB = 4.0
SPOOF_DOPPLER_OFFSET = (700.0, 700.0, 40.0, 700.0, 700.0)       # Hz; PRN 14: the same 200 Hz bin as the authentic signal
SPOOF_CARRIER_OFFSET = 1.0                                      # rad, carrier of the copy against the authentic one at antenna a
PFA = 1e-3
E2E_SEED = 4243                              # see E2E_MAX_THIRD_RATIO for the seeds that were turned down
E2E_IDX = (0, 1, 2, 3, 4)
ABSENT_PRNS = (1, 27)                        # searched by the GPU test, in neither pair's signals
# tests/test_peaks_host.py, on the surfaces of the oracle's correlator over the pair's first 11 ms (10 steps, 71 x 2048
# cells, gamma = 3.928): the smallest authentic ratio and the largest ratio of a third peak or of an absent PRN's first,
# re-measured there.  The threshold treats every cell as noise; ten signals at 44 .. 52 dB-Hz lift some cells by their
# cross-correlation, and of the seeds 4242 .. 4248 three were turned down for it BEFORE any GPU run: 4242 (absent PRN 27
# at 4.05), 4244 (a third peak at 4.01), and 4245 (3.81: too near).  The inputs were fixed, not the threshold.
E2E_MIN_AUTHENTIC_RATIO = 9.70               # PRN 4; the authentic signals stand at 9.7 .. 29.5 times the floor
E2E_MAX_THIRD_RATIO = 3.51                   # PRN 21's third peak; the others and the absent PRNs at 3.0 .. 3.4
# The largest errors of the AUTHENTIC candidates, measured on the CPU by tests/test_peaks_host.py: candidates from the truth
# rounded to the acquisition grid (``TruthSearch``), the bank restated (corr_restatement.bank), gpsjam.postcorr and
# gpsjam.spoof at their defaults.  That test re-measures each to within 10 % and prints it; the GPU test allows twice that.
E2E_CPU_ERROR_PHASE = 0.0286                 # rad
E2E_CPU_ERROR_DOPPLER = 0.1033               # Hz
E2E_CPU_ERROR_CN0 = 2.57                     # dB: the moments estimator reads low under a stronger copy of the same code
E2E_TOL_PHASE, E2E_TOL_DOPPLER, E2E_TOL_CN0 = 2.0 * E2E_CPU_ERROR_PHASE, 2.0 * E2E_CPU_ERROR_DOPPLER, 2.0 * E2E_CPU_ERROR_CN0


def spoof_code_index(k):
    return (cr.E2E_CODE_INDEX[k] + 300.0 + 97.0 * k) % 2048.0


def spoof_doppler(k):
    return cr.E2E_DOPPLER[k] + SPOOF_DOPPLER_OFFSET[k]


def truth():
    """[(prn, is_counterfeit, cn0, doppler, code_index, inter-antenna phase)]: ten signals, per PRN the strong one first."""
    out = []
    for k in E2E_IDX:
        out.append((cr.E2E_PRNS[k], True, cr.E2E_CN0[k] + SPOOF_GAIN_DB, spoof_doppler(k), spoof_code_index(k), cr.E2E_SPOOF_PHASE))
        out.append((cr.E2E_PRNS[k], False, cr.E2E_CN0[k], cr.E2E_DOPPLER[k], cr.E2E_CODE_INDEX[k], cr.E2E_AUTHENTIC[k]))
    return out


def _signal(rng, t, prn, cn0, doppler, code_index, carrier):
    """cr.e2e_pair's signal model: A code(t) bit(t) exp(-2j pi f t + j carrier), code rate tied to the Doppler,
    navigation bits of its own flipping at random every 20 code periods."""
    rate = gnss.CA_RATE * (1.0 + doppler / 1575.42e6) / cr.FS
    chips = (t - code_index) * rate
    bits = rng.choice((-1.0, 1.0), size=t.size // (20 * 2046) + 3)
    nav = bits[(np.floor(chips / cr.CODE_LEN).astype(np.int64) + 20) // 20]
    s = cr.amplitude(cn0) * gnss.ca_code(prn)[np.floor(chips % cr.CODE_LEN).astype(np.int64) % cr.CODE_LEN] * nav
    return s * np.exp(-2j * np.pi * doppler * t / cr.FS + 1j * carrier)


@functools.lru_cache(maxsize=None)
def overpowered_pair():
    """(raw_a, raw_b): cr.E2E_SAMPLES samples (100 ms) of two sample-aligned antennas on one clock, 12-LSB noise."""
    rng = np.random.default_rng(E2E_SEED)
    n = cr.E2E_SAMPLES
    t = np.arange(n, dtype=np.float64)
    za, zb = np.zeros(n, np.complex128), np.zeros(n, np.complex128)
    for prn, fake, cn0, doppler, code_index, psi in truth():
        k = cr.E2E_PRNS.index(prn)
        s = _signal(rng, t, prn, cn0, doppler, code_index, cr.E2E_CARRIER[k] + (SPOOF_CARRIER_OFFSET if fake else 0.0))
        za += s
        zb += s * np.exp(1j * psi)
    out = []
    for z in (za, zb):
        raw = cr.quantise(z + rng.normal(0.0, cr.E2E_SIGMA, n) + 1j * rng.normal(0.0, cr.E2E_SIGMA, n))
        raw.setflags(write=False)
        out.append(raw)
    return tuple(out)


class TruthSearch:
    """What postcorr and spoof ask of a gnss.AcqSearch for the K-peak chain, answered from the truth rounded to the
    acquisition grid (nearest 200 Hz bin, nearest sample): per PRN its signals strongest first, significant, and after them
    insignificant peaks up to ``k``.  ``kind``: "overpowered" (two signals per PRN) or "authentic" (cr.e2e_pair's, one)."""

    def __init__(self, kind, fs=cr.FS):
        self.kind, self.fs, self.nsamp, self.nsampchip = kind, fs, 2048, 2
        self.freqs = gnss.doppler_bins()
        self.prns = [cr.E2E_PRNS[k] for k in E2E_IDX]

    def peaks(self, capture, first_sample=0, k=2, guard=None, pfa=PFA):
        out = []
        for prn in self.prns:
            rows = [s for s in truth() if s[0] == prn and (self.kind == "overpowered" or not s[1])]
            peaks = []
            for _, _, cn0, doppler, code_index, _ in rows[:k]:
                b = int(np.argmin(np.abs(self.freqs - doppler)))
                code = int(math.floor(code_index - first_sample + 0.5)) % self.nsamp
                ratio = 1.0 + 10.0 ** (cn0 / 10.0) * 1e-3                # of the order a 10 ms surface gives
                peaks.append(gnss.AcqPeak(ratio, ratio, code, b, float(self.freqs[b]), True))
            while len(peaks) < k:
                peaks.append(gnss.AcqPeak(2.0, 2.0, (peaks[0].code_index + 1000 + len(peaks)) % self.nsamp, 0, float(self.freqs[0]), False))
            out.append(gnss.AcqPeaks(prn, 10, 1.0, peaks))
        return out
