"""The three-antenna per-bin canceller (gj_cancel2_dev, include/gpsjam.h) restated in float64 numpy, the same computation
in complex64, a frame-by-frame loop, and the inputs and constants of its tests.  Not a test module:
tests/test_cancel2_host.py and tests/cancel2/test_round6_gpu.py import it.  Everything the two-antenna canceller's
restatement (tests/cancel_restatement.py) already states is taken from there.

    A_f, B_f, C_f = fft(w * x[s_f : s_f + N]) of captures a, b, c at first_a, first_b, first_c;  s_f = f N/2
    Y_f     = (A_f - W1[set(f)] * B_f) - W2[set(f)] * C_f,   set(f) = min(f // frames_per_set, n_sets - 1)
    P_f, the mask, y_f, the overlap-add, the bytes and the records: cancel_restatement's, total_in being A's power

cancel2 and cancel2_loop are cr.cancel_aux and cr.cancel_aux_loop with two auxiliaries.
"""
import functools
import math

import numpy as np

import cancel_restatement as cr
import csd_restatement as cs
import excise_restatement as er
import ridge_restatement as rr

FS = cr.FS
NFFT = cr.NFFT                              # 16 .. 4096
CONVENTIONS = cr.CONVENTIONS
NEAR_TIE = cr.NEAR_TIE
RECORD64 = cr.RECORD64
Cancelled = cr.Cancelled
set_of = cr.set_of
PARITY_SAMPLES = cr.PARITY_SAMPLES          # 2^15
PARITY_FIRST_A, PARITY_FIRST_B, PARITY_FIRST_C = cr.PARITY_FIRST_A, cr.PARITY_FIRST_B, 7      # odd, and all different
PARITY_FRAMES_PER_SET = cr.PARITY_FRAMES_PER_SET                                             # 5
# capture c: the source of cs.parity_pair() 1.75 samples EARLIER, under its own noise, with the pair's tone
PARITY_DELAY_C = -1.75
PARITY_SEED_C = 22
# the two hand-set bins of every set, FFT order, (bin, W1, W2): b subtracted whole and c not at all, and a pair of weights
# no estimate would give
PARITY_HAND = ((3, 1.0 + 0.0j, 0.0j), (-2, -0.6 + 0.3j, 0.5 - 0.7j))
# The estimated weights are scaled down to |W1|, |W2| <= 1 and shrunk by this factor.  It and the second hand-set pair are
# chosen so that the restatement alone keeps every P_f[k] of every parity input NEAR_TIE away from its threshold and the
# tie-band share under TIE_SHARE_MAX (tests/test_cancel2_host.py asserts both and prints the smallest margin)
PARITY_SHRINK = 0.97
# Largest |y_complex64 - y_float64| over the parity inputs (every size, both conventions), measured on the CPU with
# scipy.fft on complex64 input and both predictions and subtractions in complex64.  The factor 8 is the excisor's and
# the canceller's, kept for the same reason: a transform with other radices and twiddles errs by a like amount.
E32_MEASURED = 1.2847493081835637e-05     # 9.7e-6 at 16 points .. 1.28e-5 at 4096 points
E32 = 1.3e-5
TIE_BAND = 8 * E32
TIE_SHARE_MAX = cr.TIE_SHARE_MAX            # 0.2 %


def _weights(weights, nfft):
    """complex64[n_sets][2][nfft] of what a caller hands in: [2][nfft] is one set."""
    w = np.asarray(weights, np.complex64)
    assert w.ndim in (2, 3) and w.shape[-2:] == (2, nfft), w.shape
    return w.reshape(-1, 2, nfft)                                     # the library takes float32 pairs


def cancel2(raw_a, raw_b, raw_c, weights, thr, nfft, first_a=0, first_b=0, first_c=0, n_samples=None, frames_per_set=None,
            offset=127.5, scale=1.0 / 127.5, single=False):
    """The definition on the bytes of the triple: cr.cancel_aux with two auxiliaries.  weights: complex[2][nfft] or
    [n_sets][2][nfft]; thr None: +inf.  single=True: the transforms, both predictions and both subtractions in complex64."""
    return cr.cancel_aux(raw_a, first_a, [(raw_b, first_b), (raw_c, first_c)], _weights(weights, nfft), thr, nfft, n_samples,
                         frames_per_set, offset, scale, single)


def cancel2_loop(raw_a, raw_b, raw_c, weights, thr, nfft, first_a, first_b, first_c, n_samples, frames_per_set, offset=127.5,
                 scale=1.0 / 127.5):
    """The same definition frame by frame with numpy's own transforms: (out, records)."""
    return cr.cancel_aux_loop(raw_a, first_a, [(raw_b, first_b), (raw_c, first_c)], _weights(weights, nfft), thr, nfft, n_samples,
                              frames_per_set, offset, scale)


def solve2(sbb, scc, sab, sac, sbc):
    """(W1, W2) of  W1 Sbb + W2 Sbc = conj(Sab),  W1 conj(Sbc) + W2 Scc = conj(Sac)  with Sxy = sum Y conj(X), float64."""
    det = sbb * scc - np.abs(sbc) ** 2
    return (np.conj(sab) * scc - np.conj(sac) * sbc) / det, (np.conj(sac) * sbb - np.conj(sab) * np.conj(sbc)) / det


# ---------------------------------------------------------------------------------------------------- parity inputs
@functools.lru_cache(maxsize=None)
def parity_triple():
    """cr.parity_pair() and a third capture of the same source: PARITY_SAMPLES samples behind each first sample, and not
    a byte more.  Read-only."""
    a, b = cr.parity_pair()
    rng = np.random.default_rng(cs.PARITY_SEED)                  # the pair's source is this generator's first draw
    n = cs.PARITY_SAMPLES
    src = cs.band_noise(rng, n, cs.PARITY_SOURCE_SIGMA, -0.5 * FS, 0.5 * FS)
    own = np.random.default_rng(PARITY_SEED_C)
    z = cs.delayed(src, PARITY_DELAY_C) + rr._noise(own, n, rr.NOISE_SIGMA) + rr.tone(n, rr.PARITY_TONE_HZ, 25.0)
    c = rr.quantise(z)[:2 * (PARITY_FIRST_C + PARITY_SAMPLES)].copy()
    c.setflags(write=False)
    return a, b, c


def parity_sets(nfft):
    return cr.parity_sets(nfft)


@functools.lru_cache(maxsize=None)
def parity_weights(nfft, offset=127.5):
    """complex64[n_sets][2][nfft]: the 2 x 2 solution of the triple's own restated sums over each set's frames, each weight
    scaled down to |W| = 1 where it is larger (five frames estimate it loosely) and shrunk by PARITY_SHRINK, plus the two
    hand-set bins.  Read-only."""
    a, b, c = parity_triple()
    A = cr.frame_spectra(a, nfft, PARITY_FIRST_A, PARITY_SAMPLES, offset)
    B = cr.frame_spectra(b, nfft, PARITY_FIRST_B, PARITY_SAMPLES, offset)
    Cc = cr.frame_spectra(c, nfft, PARITY_FIRST_C, PARITY_SAMPLES, offset)
    n_sets = parity_sets(nfft)
    sets = set_of(A.shape[0], PARITY_FRAMES_PER_SET, n_sets)
    w = np.zeros((n_sets, 2, nfft), np.complex128)
    for s in range(n_sets):
        m = sets == s
        with np.errstate(divide="ignore", invalid="ignore"):
                w[s] = solve2((np.abs(B[m]) ** 2).sum(axis=0), (np.abs(Cc[m]) ** 2).sum(axis=0), (B[m] * np.conj(A[m])).sum(axis=0),
                          (Cc[m] * np.conj(A[m])).sum(axis=0), (Cc[m] * np.conj(B[m])).sum(axis=0))
    w = np.where(np.isfinite(w), w, 0.0)                         # a short last set may hold a single frame: det = 0
    w *= PARITY_SHRINK / np.maximum(np.abs(w), 1.0)
    for k, v1, v2 in PARITY_HAND:
        w[:, 0, k], w[:, 1, k] = v1, v2
    w = w.astype(np.complex64)
    w /= np.maximum(np.abs(w), 1.0).astype(np.float32)           # the rounding to float32 may have carried |W| past 1
    w.setflags(write=False)
    return w


def parity_threshold(nfft, scale=1.0 / 127.5):
    return er.parity_threshold(nfft, scale)                      # the excisor's: flat, 16 x the nominal noise floor


@functools.lru_cache(maxsize=None)
def parity_reference(nfft, offset=127.5, scale=1.0 / 127.5, single=False):
    """The restatement of the parity call, computed once and shared."""
    a, b, c = parity_triple()
    return cancel2(a, b, c, parity_weights(nfft, offset), parity_threshold(nfft, scale), nfft, PARITY_FIRST_A, PARITY_FIRST_B,
                   PARITY_FIRST_C, PARITY_SAMPLES, PARITY_FRAMES_PER_SET, offset, scale, single)


# ---------------------------------------------------------------------------------------------------- end to end
# er.e2e_capture's three satellites at half amplitude in its noise at each of three antennas; from sample 2^17 on two
# independent full-band Gaussian jammers of sigma 30 LSB.  Seen from b and c the two jammers' phase differences are
# a quarter turn apart in opposite senses: the 2 x 2 steering matrix is as well conditioned as it gets, and each single
# auxiliary is half blind -- its one null fits one jammer.
E2E_SAT_SCALE = cr.E2E_SAT_SCALE            # 0.5
E2E_JAM_SIGMA = cr.E2E_JAM_SIGMA            # 30
E2E_SEED_NOISE = (4, 40, 42)                # a (er.e2e_capture's), b, c
E2E_SEED_JAM = (41, 43)
E2E_SAT_PHASE = ((math.pi / 2, -2.5), (2.8, 0.4), (-0.4, 3.0))        # each satellite's phase at (b, c)
# per jammer: (delay, phase) at b, (delay, phase) at c
E2E_JAM_AT = (((0.4, 1.3), (-0.3, -0.9)), ((0.3, 1.3 - math.pi / 2), (-0.2, -0.9 + math.pi / 2)))
E2E_NFFT, E2E_FRAMES_PER_ROW = 256, 128     # 2^17 / (128 * 256) = 4 quiet rows, then one jammed row of 2^15 samples
E2E_P_FA = 1e-6
# Largest |cleaned C/N0 - (jammer-free + e2e_predicted_db)| of the float64 chain over the three satellites on the CPU
# (tests/test_cancel2_host.py re-measures it); the GPU test's tolerance is twice that, cr.E2E_CN0_TOL_DB's factor and
# for the same reason: another transform's rounding moves a 1-ms acquisition peak by a like amount
E2E_CPU_RESIDUAL_MEASURED = 0.889         # PRN 3: -0.889 dB; PRN 17 -0.745 dB, PRN 25 -0.377 dB
E2E_CPU_RESIDUAL_DB = 0.89
E2E_CN0_TOL_DB = 2.0 * E2E_CPU_RESIDUAL_DB


@functools.lru_cache(maxsize=None)
def e2e_triple(jammed=True):
    """(main, aux_b, aux_c), read-only uint8 of er.E2E_LEAD + er.E2E_AFTER samples each."""
    from gpsjam import gnss
    n = er.E2E_LEAD + er.E2E_AFTER
    k = np.arange(n)
    z = []
    for seed in E2E_SEED_NOISE:
        rng = np.random.default_rng(seed)
        z.append(rng.normal(0, er.E2E_SIGMA, n) + 1j * rng.normal(0, er.E2E_SIGMA, n))
    for (prn, dop, delay, amp), (psi_b, psi_c) in zip(er.E2E_SATS, E2E_SAT_PHASE):
        chip = ((k - delay) * 1.023e6 / FS) % 1023
        s = E2E_SAT_SCALE * amp * gnss.ca_code(prn)[chip.astype(np.int64)] * np.exp(-2j * np.pi * dop * (k / FS))
        z[0] += s
        z[1] += s * np.exp(1j * psi_b)
        z[2] += s * np.exp(1j * psi_c)
    if jammed:
        m = er.E2E_AFTER
        for seed, ((delay_b, phase_b), (delay_c, phase_c)) in zip(E2E_SEED_JAM, E2E_JAM_AT):
            rj = np.random.default_rng(seed)
            spec = np.fft.fft(rj.normal(0, E2E_JAM_SIGMA, m) + 1j * rj.normal(0, E2E_JAM_SIGMA, m))
            z[0][er.E2E_LEAD:] += cs.delayed(spec, 0.0)
            z[1][er.E2E_LEAD:] += cs.delayed(spec, delay_b) * np.exp(1j * phase_b)
            z[2][er.E2E_LEAD:] += cs.delayed(spec, delay_c) * np.exp(1j * phase_c)
    out = []
    for v in z:
        iq = np.empty(2 * n, np.float64)
        iq[0::2], iq[1::2] = v.real, v.imag
        raw = (np.clip(np.round(iq), -128, 127) + 128).astype(np.uint8)
        raw.setflags(write=False)
        out.append(raw)
    return tuple(out)


def e2e_predicted_db(w1, w2, psi_b, psi_c):
    """What the canceller costs a satellite whose phases at the auxiliaries are psi_b and psi_c, over the bins whose weights
    are w1 and w2: the signal goes through |1 - W1 e^{j psi_b} - W2 e^{j psi_c}|^2, the noise rises by 1 + |W1|^2 + |W2|^2."""
    w1, w2 = np.asarray(w1, np.complex128), np.asarray(w2, np.complex128)
    gain = np.mean(np.abs(1.0 - w1 * np.exp(1j * psi_b) - w2 * np.exp(1j * psi_c)) ** 2)
    return 10.0 * math.log10(gain / np.mean(1.0 + np.abs(w1) ** 2 + np.abs(w2) ** 2))


def compare(got, rec, want, what):
    """GPU bytes and records against a Cancelled of this restatement: the two-antenna comparison with this file's tie band."""
    cr.compare(got, rec, want, what, TIE_BAND)


def f32(w):
    return np.ascontiguousarray(w, np.complex64).view(np.float32)
