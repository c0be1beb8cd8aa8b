"""The two-antenna per-bin canceller (gj_cancel_dev, include/gpsjam.h) restated in float64 numpy, the same computation in
complex64, and the inputs and constants of its tests.  Not a test module: tests/test_cancel_host.py and
tests/cancel/test_round6_gpu.py import it.

    x_a[t]  = (I - offset) + j (Q - offset) of capture a at sample first_a + t          likewise x_b at first_b
    A_f     = fft(w * x_a[s_f : s_f + N]),  s_f = f N/2,  w the periodic Hann window      B_f likewise
    Y_f     = A_f - W[min(f // frames_per_set, n_sets - 1)] * B_f
    P_f[k]  = |Y_f[k]|^2 * scale^2
    y_f     = ifft(Y_f where P_f <= thr else 0)
    y[t]    = y_{f-1}[t - s_{f-1}] + y_f[t - s_f];  u = clip(rint(float32(y + offset)), 0, 255) on samples [N/2, F N/2);
              the other samples are capture a's

cancel_aux states it once for a list of auxiliaries, Y_f = (A_f - W_1 X_1f) - W_2 X_2f ..., for this canceller and the
three-antenna one (tests/cancel2_restatement.py); everything from P_f on is the excisor's own text (er.finish).
"""
import functools
import math

import numpy as np
import scipy.fft

import csd_restatement as cs
import excise_restatement as er
import ridge_restatement as rr

RECORD64 = np.dtype([("total_in", np.float64), ("total", np.float64), ("removed", np.float64), ("n_excised", np.int32)])

FS = rr.FS
NFFT = er.NFFT                              # 16 .. 4096
CONVENTIONS = er.CONVENTIONS
NEAR_TIE = er.NEAR_TIE                      # no P_f[k] of a GPU input may lie within 1e-4 relative of its threshold
PARITY_SAMPLES = 1 << 15                    # of cs.parity_pair(): 4096 points still get 15 frames
PARITY_FIRST_A, PARITY_FIRST_B = 1, 4       # odd, and different
PARITY_FRAMES_PER_SET = 5                   # the last set is short wherever 5 does not divide the frame count
# the two hand-set bins of every set, FFT order: b subtracted whole, and a weight no estimate would give
PARITY_HAND = ((3, 1.0 + 0.0j), (-2, -0.6 + 0.3j))
# The estimated weights are shrunk by this factor.  It and the second hand-set value are chosen so that the restatement
# alone keeps every P_f[k] of every parity input NEAR_TIE away from its threshold (tests/test_cancel_host.py asserts it
# and prints the smallest margin): 65520 powers at 16 points leave little room, and the pair's seed is csd's
PARITY_SHRINK = 0.97
# Largest |y_complex64 - y_float64| over the parity inputs (every size, both conventions), measured on the CPU with
# scipy.fft on complex64 input and the prediction W B in complex64: E32_MEASURED.  The factor 8 is the excisor's (a
# transform with other radices and twiddles errs by a like amount, and the final + offset).
E32_MEASURED = 1.2459745136084166e-05     # 7.5e-6 at 16 points .. 1.25e-5 at 2048 points
E32 = 1.25e-5
TIE_BAND = 8 * E32
TIE_SHARE_MAX = 0.002                       # at most 0.2 % of the output values may lie inside the tie band


class Cancelled:
    """out: uint8[2 n_samples]; records: RECORD64[F]; value: float64[2 (F-1) N/2], y + offset of the range [N/2, F N/2)
    before rounding, interleaved like the bytes; power: P[F][N]; cut: the mask's zeros, bool[F][N]."""

    def __init__(self, out, records, value, power, cut, nfft):
        self.out, self.records, self.value, self.power, self.cut, self.nfft = out, records, value, power, cut, nfft

    @property
    def lo(self):
        return self.nfft                     # first cancelled byte (sample N/2)

    @property
    def hi(self):
        return self.records.size * self.nfft    # one past the last cancelled byte (sample F N/2)


def set_of(n_frames, frames_per_set, n_sets):
    """set(f) of every frame."""
    return np.minimum(np.arange(n_frames) // int(frames_per_set), int(n_sets) - 1)


def frame_spectra(raw, nfft, first, n_samples, offset=127.5, single=False):
    """X[F][nfft] of the excisor's frames (hop N/2) over samples first .. first + n_samples, LSB units."""
    raw = np.asarray(raw, np.uint8)
    nf = er.frames_loop(n_samples, nfft)
    assert nf >= 1 and first + n_samples <= raw.size // 2
    x = er.unpack_lsb(raw[2 * first:2 * (first + n_samples)], offset)
    idx = ((nfft // 2) * np.arange(nf))[:, None] + np.arange(nfft)[None, :]
    seg = x[idx] * er.hann(nfft)[None, :]
    return scipy.fft.fft(seg.astype(np.complex64) if single else seg, axis=1)


def cancel_aux(raw_a, first_a, aux, weights, thr, nfft, n_samples=None, frames_per_set=None, offset=127.5, scale=1.0 / 127.5,
               single=False):
    """The definition for any number of auxiliaries: aux = [(raw, first), ...], weights complex[n_sets][n_aux][nfft] (or
    anything that reshapes to it); thr None: +inf.  Y = A, then Y = Y - W_i X_i for i in order.  single=True: the
    transforms, every prediction and every subtraction in complex64, everything else alike (er.finish)."""
    ins = [(np.asarray(raw, np.uint8), first) for raw, first in [(raw_a, first_a), *aux]]
    if n_samples is None:
        n_samples = min(raw.size // 2 - first for raw, first in ins)
    w = np.asarray(weights, np.complex64).reshape(-1, len(aux), nfft)     # the library takes float32 pairs
    A, *X = (frame_spectra(raw, nfft, first, n_samples, offset, single) for raw, first in ins)
    nf = A.shape[0]
    fps = nf if frames_per_set is None else int(frames_per_set)
    assert fps >= 1 and (frames_per_set is not None or w.shape[0] == 1)
    wf = w[set_of(nf, fps, w.shape[0])]
    if not single:
        wf = wf.astype(np.complex128)
    Y = A
    for i, Xi in enumerate(X):
        Y = Y - wf[:, i] * Xi
    assert Y.dtype == (np.complex64 if single else np.complex128)
    P, cut, sums, value, out = er.finish(Y, ins[0][0][2 * first_a:2 * (first_a + n_samples)], thr, nfft, offset, scale)
    rec = np.zeros(nf, RECORD64)
    rec["total_in"] = ((np.abs(A.astype(np.complex128)) ** 2) * (scale * scale)).sum(axis=1)
    rec["total"], rec["removed"], rec["n_excised"] = sums
    return Cancelled(out, rec, value, P, cut, nfft)


def cancel(raw_a, raw_b, weights, thr, nfft, first_a=0, first_b=0, n_samples=None, frames_per_set=None, offset=127.5,
           scale=1.0 / 127.5, single=False):
    """The definition on the bytes of the pair: cancel_aux with one auxiliary.  weights: complex[nfft] or [n_sets][nfft]."""
    return cancel_aux(raw_a, first_a, [(raw_b, first_b)], weights, thr, nfft, n_samples, frames_per_set, offset, scale, single)


def cancel_aux_loop(raw_a, first_a, aux, weights, thr, nfft, n_samples, frames_per_set, offset=127.5, scale=1.0 / 127.5):
    """The same definition frame by frame with numpy's own transforms: (out, records)."""
    h, w = nfft // 2, np.asarray(weights, np.complex64).reshape(-1, len(aux), nfft).astype(np.complex128)
    xs = [er.unpack_lsb(np.asarray(raw, np.uint8)[2 * first:2 * (first + n_samples)], offset)
          for raw, first in [(raw_a, first_a), *aux]]
    win = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(nfft) / nfft)
    thr = np.asarray(thr, np.float32).astype(np.float64)
    acc = np.zeros(n_samples, np.complex128)
    rec, f = [], 0
    while f * h + nfft <= n_samples:
        a, *others = (np.fft.fft(win * x[f * h:f * h + nfft]) for x in xs)
        y = a
        for wi, xi in zip(w[min(f // frames_per_set, w.shape[0] - 1)], others):
            y = y - wi * xi
        p = (y.real ** 2 + y.imag ** 2) * scale * scale
        keep = ~(p > thr)
        rec.append((float(np.sum(np.abs(a) ** 2) * scale * scale), float(p.sum()), float(p[~keep].sum()), int(np.sum(~keep))))
        acc[f * h:f * h + nfft] += np.fft.ifft(np.where(keep, y, 0))
        f += 1
    out = np.asarray(raw_a, np.uint8)[2 * first_a:2 * (first_a + n_samples)].copy()
    body = np.empty(2 * (f - 1) * h)
    body[0::2], body[1::2] = acc[h:f * h].real + offset, acc[h:f * h].imag + offset
    out[2 * h:2 * f * h] = np.clip(np.rint(body.astype(np.float32)), 0, 255).astype(np.uint8)
    return out, np.array(rec, RECORD64)


def cancel_loop(raw_a, raw_b, weights, thr, nfft, first_a, first_b, n_samples, frames_per_set, offset=127.5, scale=1.0 / 127.5):
    return cancel_aux_loop(raw_a, first_a, [(raw_b, first_b)], weights, thr, nfft, n_samples, frames_per_set, offset, scale)


# ---------------------------------------------------------------------------------------------------- parity inputs
@functools.lru_cache(maxsize=None)
def parity_pair():
    """The head of cs.parity_pair(): PARITY_SAMPLES samples behind each first sample, and not a byte more."""
    a, b = cs.parity_pair()
    a, b = a[:2 * (PARITY_FIRST_A + PARITY_SAMPLES)].copy(), b[:2 * (PARITY_FIRST_B + PARITY_SAMPLES)].copy()
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


def parity_sets(nfft):
    return -(-er.frames_loop(PARITY_SAMPLES, nfft) // PARITY_FRAMES_PER_SET)


@functools.lru_cache(maxsize=None)
def parity_weights(nfft, offset=127.5):
    """complex64[n_sets][nfft]: conj(Sab) / Sbb of the pair's own restated sums over each set's frames, scaled down to
    |W| = 1 where it is larger (five frames estimate it loosely) and shrunk by PARITY_SHRINK, plus the two hand-set bins.  Read-only."""
    a, b = parity_pair()
    A = frame_spectra(a, nfft, PARITY_FIRST_A, PARITY_SAMPLES, offset)
    B = frame_spectra(b, nfft, PARITY_FIRST_B, PARITY_SAMPLES, offset)
    n_sets = parity_sets(nfft)
    sets = set_of(A.shape[0], PARITY_FRAMES_PER_SET, n_sets)
    w = np.zeros((n_sets, nfft), np.complex128)
    for s in range(n_sets):
        m = sets == s
        sab, sbb = (B[m] * np.conj(A[m])).sum(axis=0), (np.abs(B[m]) ** 2).sum(axis=0)
        w[s] = np.conj(sab) / sbb
    w *= PARITY_SHRINK / np.maximum(np.abs(w), 1.0)
    for k, v in PARITY_HAND:
        w[:, k] = v
    w = w.astype(np.complex64)
    w /= np.maximum(np.abs(w), 1.0).astype(np.float32)         # the rounding to float32 may have carried |W| past 1
    w.setflags(write=False)
    return w


def parity_threshold(nfft, scale=1.0 / 127.5):
    return er.parity_threshold(nfft, scale)                    # the excisor's: flat, 16 x the nominal noise floor


@functools.lru_cache(maxsize=None)
def parity_reference(nfft, offset=127.5, scale=1.0 / 127.5, single=False):
    """The restatement of the parity call, computed once and shared."""
    a, b = parity_pair()
    return cancel(a, b, parity_weights(nfft, offset), parity_threshold(nfft, scale), nfft, PARITY_FIRST_A, PARITY_FIRST_B,
                  PARITY_SAMPLES, PARITY_FRAMES_PER_SET, offset, scale, single)


# ---------------------------------------------------------------------------------------------------- end to end
# er.e2e_capture's three satellites at half amplitude in its noise; from sample 2^17 on a full-band Gaussian jammer, 9.5 dB
# above the receiver noise, which the second antenna sees 0.4 sample later and turned by 1.3 rad under its own noise
E2E_SAT_SCALE = 0.5
E2E_JAM_SIGMA = 30.0
E2E_JAM_DELAY, E2E_JAM_PHASE = 0.4, 1.3
# each satellite's inter-antenna phase, as an offset from the jammer's at band centre: at least 90 degrees away, so that
# none sits in the null the canceller steers at the jammer
E2E_SAT_DPHI = (math.pi, 0.75 * math.pi, -2.0 * math.pi / 3.0)
E2E_NFFT, E2E_FRAMES_PER_ROW = 1024, 32     # 2^17 / (32 * 1024) = 4 quiet rows, then one jammed row of 2^15 samples
E2E_SEED_AUX_NOISE, E2E_SEED_JAM = 40, 41
# Largest |cleaned - (jammer-free + 10 log10(|1 - W e^{j dphi}|^2 / (1 + |W|^2)))| of the float64 chain on the CPU, W the
# median |W| of the jammed row (tests/test_cancel_host.py re-measures it); the GPU test's tolerance is twice that
E2E_CPU_RESIDUAL_MEASURED = 3.068         # PRN 3 (dphi = pi): -3.068 dB; PRN 17 -0.527 dB, PRN 25 +0.386 dB
E2E_CPU_RESIDUAL_DB = 3.07
E2E_CN0_TOL_DB = 2.0 * E2E_CPU_RESIDUAL_DB


@functools.lru_cache(maxsize=None)
def e2e_pair(jammed=True):
    """(main, aux), read-only uint8 of er.E2E_LEAD + er.E2E_AFTER samples each."""
    from gpsjam import gnss
    n = er.E2E_LEAD + er.E2E_AFTER
    rng = np.random.default_rng(4)                             # er.e2e_capture's noise
    k = np.arange(n)
    za = rng.normal(0, er.E2E_SIGMA, n) + 1j * rng.normal(0, er.E2E_SIGMA, n)
    r2 = np.random.default_rng(E2E_SEED_AUX_NOISE)
    zb = r2.normal(0, er.E2E_SIGMA, n) + 1j * r2.normal(0, er.E2E_SIGMA, n)
    for (prn, dop, delay, amp), dphi in zip(er.E2E_SATS, E2E_SAT_DPHI):
        chip = ((k - delay) * 1.023e6 / FS) % 1023
        s = E2E_SAT_SCALE * amp * gnss.ca_code(prn)[chip.astype(np.int64)] * np.exp(-2j * np.pi * dop * (k / FS))
        za += s
        zb += s * np.exp(1j * (E2E_JAM_PHASE + dphi))
    if jammed:
        r3 = np.random.default_rng(E2E_SEED_JAM)
        m = er.E2E_AFTER
        spec = np.fft.fft(r3.normal(0, E2E_JAM_SIGMA, m) + 1j * r3.normal(0, E2E_JAM_SIGMA, m))
        za[er.E2E_LEAD:] += cs.delayed(spec, 0.0)
        zb[er.E2E_LEAD:] += cs.delayed(spec, E2E_JAM_DELAY) * np.exp(1j * E2E_JAM_PHASE)
    out = []
    for z in (za, zb):
        iq = np.empty(2 * n, np.float64)
        iq[0::2], iq[1::2] = z.real, z.imag
        raw = (np.clip(np.round(iq), -128, 127) + 128).astype(np.uint8)
        raw.setflags(write=False)
        out.append(raw)
    return tuple(out)


def e2e_predicted_db(w_abs, dphi):
    """What the canceller costs a satellite whose inter-antenna phase is dphi from the jammer's: the signal goes through
    |1 - W e^{j dphi}|^2 and the noise rises by 1 + |W|^2."""
    return 10.0 * math.log10(abs(1.0 - w_abs * np.exp(1j * dphi)) ** 2 / (1.0 + w_abs * w_abs))


RTOL = 1e-5                                     # of total_in: the project's figure for a K2 value summed in another order


def compare(got, rec, want, what, band=TIE_BAND):
    """GPU bytes and records against a Cancelled; ``band``: the tie band of the canceller that made them."""
    assert rec.size == want.records.size and got.size == want.out.size, what
    # the mask on every bin: per frame the count is equal, and no bin of the restatement is near its threshold, so a
    # differing bin would have to be matched by another differing the other way at a margin of 1e-4 each
    np.testing.assert_array_equal(rec["n_excised"], want.records["n_excised"], err_msg=str(what))
    tin = want.records["total_in"]
    for key in ("total_in", "total", "removed"):
        err = float(np.max(np.abs(rec[key] - want.records[key]) / tin))
        print(f"{what} {key}: {err:.2e} of total_in")
        assert err <= RTOL, (what, key, err)
    assert np.array_equal(got[:want.lo], want.out[:want.lo]) and np.array_equal(got[want.hi:], want.out[want.hi:]), (what, "edges")
    body, ref = got[want.lo:want.hi].astype(np.int16), want.out[want.lo:want.hi].astype(np.int16)
    clear = er.tie_distance(want.value) > band
    diff = np.abs(body - ref)
    print(f"{what}: {int(np.sum(diff != 0))} of {diff.size} bytes differ, {int(np.sum(~clear))} lie in the tie band")
    assert not diff[clear].any(), (what, int(np.sum(diff[clear] != 0)), "bytes differ outside the tie band")
    assert diff.max(initial=0) <= 1, (what, int(diff.max()))
