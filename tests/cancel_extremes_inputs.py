"""Inputs, constants and recorded measurements of the cancellers' extreme tests (gj_cancel_dev, gj_cancel2_dev): constant
weights whose result has a closed form without a transform in it, the saturated and degenerate captures of
tests/extremes_inputs.py in the roles a | b (| c) under weights of modulus up to 4, and the inputs of the runs past byte
2^32 and at the ends of size_t.  Not a test module: tests/test_cancel_extremes_host.py and
tests/cancel_extremes/test_round6_gpu.py import it.

What these inputs have and the parity inputs of tests/cancel_restatement.py never do: |W| > 1, so that the output leaves
[0, 255] before rounding at both ends; full-scale lines whose rounding error reaches the samples that remain; frames
without any power.  Every figure below that a GPU test relies on is measured on the float64 and complex64 restatements
alone by tests/test_cancel_extremes_host.py, which asserts that what is recorded here is what it measures.
"""
import functools

import numpy as np

import cancel2_restatement as c2
import cancel_restatement as cr
import csd_restatement as cs
import excise_restatement as er
import extremes_inputs as xi

CONVENTIONS = er.CONVENTIONS                # (127.5, 1/127.5) and (128, 1/128)
FIRSTS = (1, 4, 9)                          # first_a, first_b, first_c: odd, and all different
FRAMES_PER_SET = 5
RECORD_KEYS = ("total_in", "total", "removed")


def aux_of(raws):
    """[(raw, first), ...] of the auxiliaries of a pair or triple."""
    return [(raw, first) for raw, first in zip(raws[1:], FIRSTS[1:])]


def envelope(raws, weights, nfft, n_samples, frames_per_set, offset, scale):
    """D_f = scale^2 sum_k (|A| + |W1| |B| + |W2| |C|)^2 in float64: the magnitude Y is a difference of, which bounds
    what rounding can do to `total` and `removed` where `total` itself is small, or 0, by cancellation."""
    spectra = [cr.frame_spectra(raw, nfft, first, n_samples, offset) for raw, first in zip(raws, FIRSTS)]
    nf = spectra[0].shape[0]
    w = np.asarray(weights, np.complex64).reshape(-1, len(raws) - 1, nfft).astype(np.complex128)
    wf = np.abs(w[cr.set_of(nf, nf if frames_per_set is None else frames_per_set, w.shape[0])])
    mag = np.abs(spectra[0])
    for i, x in enumerate(spectra[1:]):
        mag = mag + wf[:, i] * np.abs(x)
    return (mag * mag).sum(axis=1) * (scale * scale)


def record_ratio(got, want, d_f):
    """Largest |got - want| of total_in in units of the restated total_in, and of total and removed in units of D_f, over
    the frames where those units are not 0 (there the difference must be 0, which record_errors checks apart)."""
    worst = 0.0
    for key in RECORD_KEYS:
        unit = want["total_in"] if key == "total_in" else d_f
        live = unit > 0
        if live.any():
            worst = max(worst, float(np.max(np.abs(got[key][live].astype(np.float64) - want[key][live]) / unit[live])))
    return worst


def record_errors(got, want, d_f, tol):
    """Names of the record fields that are further than tol * unit from the restatement on some frame: unit is the restated
    total_in for total_in and D_f for total and removed.  Nothing is divided, so where the unit is 0 the field must be 0."""
    bad = []
    for key in RECORD_KEYS:
        unit = want["total_in"] if key == "total_in" else d_f
        if np.any(np.abs(got[key].astype(np.float64) - want[key]) > tol * unit):
            bad.append(key)
    return bad


# ------------------------------------------------------------------------------------------- 1. constant weights
# With W[s][k] = c on every set and bin and every threshold +inf the periodic Hann window at hop N/2 sums to 1, and the
# definition collapses to y[t] = x_a[t] - c x_b[t] on samples [N/2, F N/2): no transform is left in it.  For a Gaussian
# integer c every y + offset is an integer under offset 128, and under 127.5 where Re c and Im c have the same parity
# (c = 3 there puts every value on a tie).  Uniform random bytes in every capture: 12 % to 48 % of the values leave
# [0, 255] at each end, so the clamp decides them.
CLOSED_SAMPLES = 1 << 13
CLOSED_SEEDS = (101, 102, 103)              # captures a, b, c
CLOSED_NFFT = cr.NFFT                       # 16 .. 4096
CLOSED_RAIL_SHARE_MIN = 0.05                # at least this share of the values is clamped at each end, in every case
CLOSED_TIE_MIN = 0.25                       # no value is nearer than this to a rounding tie (they are integers)
# (weights of one set, offset, scale)
CLOSED_CASES = ((-2.0 + 0.0j, 127.5, 1.0 / 127.5), (-2.0j, 127.5, 1.0 / 127.5),
                (-1.0 + 0.0j, 128.0, 1.0 / 128.0), (1.0j, 128.0, 1.0 / 128.0), (-16.0 + 0.0j, 128.0, 1.0 / 128.0))
CLOSED_CASES2 = (((-1.0 + 0.0j, 1.0j), 128.0, 1.0 / 128.0), ((-2.0 + 0.0j, -2.0j), 127.5, 1.0 / 127.5),
                 ((-2.0j, 0.0j), 127.5, 1.0 / 127.5), ((0.0j, -1.0 + 0.0j), 128.0, 1.0 / 128.0))
# the one case of each canceller that also runs as three equal sets at five frames per set
CLOSED_THREE_SETS = 0


@functools.lru_cache(maxsize=None)
def closed_captures():
    """Uniform random bytes, CLOSED_SAMPLES samples behind each first sample and not a byte more.  Read-only."""
    out = []
    for seed, first in zip(CLOSED_SEEDS, FIRSTS):
        raw = np.random.default_rng(seed).integers(0, 256, 2 * (first + CLOSED_SAMPLES), dtype=np.uint8)
        raw.setflags(write=False)
        out.append(raw)
    return tuple(out)


def closed_weights(c, nfft, n_sets=1):
    """complex64[n_sets][nfft] of one constant, or [n_sets][2][nfft] of a pair of them."""
    c = np.atleast_1d(np.asarray(c, np.complex64))
    w = np.empty((n_sets, c.size, nfft), np.complex64)
    w[...] = c[None, :, None]
    return w[:, 0] if c.size == 1 else w


def closed_value(c, offset, nfft):
    """y + offset of samples [N/2, F N/2), interleaved like the bytes, in exact integer arithmetic on the bytes."""
    c = np.atleast_1d(np.asarray(c, np.complex128))
    raws = closed_captures()
    x = [er.unpack_lsb(raw[2 * first:2 * (first + CLOSED_SAMPLES)], offset) for raw, first in zip(raws, FIRSTS)]
    y = x[0]
    for ci, xi_ in zip(c, x[1:]):
        y = y - ci * xi_
    nf = er.frames_loop(CLOSED_SAMPLES, nfft)
    y = y[nfft // 2:nf * (nfft // 2)]
    value = np.empty(2 * y.size)
    value[0::2], value[1::2] = y.real + offset, y.imag + offset
    return value


def closed_bytes(c, offset, nfft):
    """What the call must write: capture a's bytes with clip(rint(closed form), 0, 255) on samples [N/2, F N/2)."""
    out = closed_captures()[0][2 * FIRSTS[0]:2 * (FIRSTS[0] + CLOSED_SAMPLES)].copy()
    value = closed_value(c, offset, nfft)
    out[nfft:nfft + value.size] = np.clip(np.rint(value), 0, 255).astype(np.uint8)
    return out


@functools.lru_cache(maxsize=None)
def closed_reference(c, offset, scale, nfft, single=False):
    """(Cancelled, D_f) of the restatement of a closed-form case, one set."""
    c1 = np.atleast_1d(np.asarray(c, np.complex64))
    raws = closed_captures()[:1 + c1.size]
    w = closed_weights(c, nfft)
    want = cr.cancel_aux(raws[0], FIRSTS[0], aux_of(raws), w, None, nfft, CLOSED_SAMPLES, None, offset, scale, single)
    return want, envelope(raws, w, nfft, CLOSED_SAMPLES, None, offset, scale)


# Largest record_ratio of the complex64 restatement against the float64 one over the closed-form cases of both
# cancellers, per nfft, as tests/test_cancel_extremes_host.py measures it; the GPU test's tolerance is 8 times that
CLOSED_REC32_MEASURED = {16: 1.72e-7, 32: 1.54e-7, 64: 1.28e-7, 128: 1.19e-7, 256: 9.34e-8, 512: 8.34e-8, 1024: 7.1e-8, 2048: 7.86e-8,
                         4096: 6.64e-8}


def closed_record_tol(nfft):
    return 8.0 * CLOSED_REC32_MEASURED[nfft]


# ------------------------------------------------------------------------------ 2. extreme captures, |W| up to 4
EXTREME_NFFT = xi.CHIRP_NFFT                # 16, 64, 1024, 4096
EXTREME_SAMPLES = xi.SAMPLES - FIRSTS[2]    # what all three captures hold behind their first samples
W_MAX = 4.0
THRESHOLD_FLOOR = 1e-6                      # no threshold lies below this share of the case's largest restated power
PAIRS = (("uniform bytes", "saturated tone"), ("saturated tone", "uniform bytes"), ("constant 255", "constant 0"),
         ("constant 0", "uniform bytes"), ("nyquist full scale", "constant 255"), ("quiet then rail to rail", "uniform bytes"),
         ("one impulse", "uniform bytes"), ("uniform bytes", "one impulse"), ("constant 128/127", "saturated tone"),
         ("one impulse", "one impulse"))
TRIPLES = (("uniform bytes", "saturated tone", "quiet then rail to rail"), ("saturated tone", "uniform bytes", "uniform bytes"),
           ("constant 255", "constant 0", "uniform bytes"), ("one impulse", "uniform bytes", "saturated tone"),
           ("quiet then rail to rail", "uniform bytes", "nyquist full scale"), ("one impulse", "one impulse", "one impulse"))
KINDS = ("cut", "inf")                      # the case's own thresholds, and +inf on every bin


def extreme_sets(nfft):
    return -(-er.frames_loop(EXTREME_SAMPLES, nfft) // FRAMES_PER_SET)


@functools.lru_cache(maxsize=None)
def extreme_weights(n_aux, nfft):
    """complex64[n_sets][nfft] (one auxiliary) or [n_sets][2][nfft]: modulus uniform in [0, 4], phase uniform, a set per
    five frames, seeded by nfft.  Read-only."""
    rng = np.random.default_rng(nfft)
    shape = (extreme_sets(nfft), n_aux, nfft)
    w = (rng.uniform(0.0, W_MAX, shape) * np.exp(2j * np.pi * rng.uniform(0.0, 1.0, shape))).astype(np.complex64)
    w = w[:, 0] if n_aux == 1 else w
    w.setflags(write=False)
    return w


def extreme_cases(names_of=None):
    """(names, nfft, offset, scale, kind) of every case of section 2, pairs first."""
    return [(names, nfft, offset, scale, kind) for names in (PAIRS + TRIPLES if names_of is None else names_of)
            for nfft in EXTREME_NFFT for offset, scale in CONVENTIONS for kind in KINDS]


# The thresholds of every "cut" case are flat: this share of the case's largest restated power P_f[k] (float64, over
# every frame and bin).  A share fixed for all cases does not keep er.threshold_margin of the restated powers at
# cr.NEAR_TIE (a case has 65 000 to 130 000 powers), so each case has its own: of 800 candidates between 0.2 % and 50 %
# the one with the widest margin among those that cut 1 % to 40 % of the bins; never below THRESHOLD_FLOOR.  The
# smallest margin is 4.8e-4, and the complex64 restatement cuts the float64 one's bins in every case.
# {names: {nfft: ((share, measured margin) under offset 127.5, the same under 128)}}
THRESHOLD_SHARE = {
    ("uniform bytes", "saturated tone"): {
        16: ((0.313, 1.86e-03), (0.116, 1.62e-03)), 64: ((0.00921, 3.05e-03), (0.105, 3.76e-03)),
        1024: ((0.13, 1.99e-01), (0.13, 1.99e-01)), 4096: ((0.448, 5.93e-01), (0.448, 5.93e-01))},
    ("saturated tone", "uniform bytes"): {
        16: ((0.298, 5.81e-04), (0.212, 9.11e-04)), 64: ((0.252, 2.53e-03), (0.304, 1.40e-03)),
        1024: ((0.0244, 7.88e-04), (0.0244, 7.88e-04)), 4096: ((0.00428, 6.82e-04), (0.00428, 6.82e-04))},
    ("constant 255", "constant 0"): {
        16: ((0.00236, 4.05e-02), (0.00233, 3.43e-02)), 64: ((0.00225, 1.72e-01), (0.00226, 1.43e-01)),
        1024: ((0.0083, 1.00e+00), (0.00842, 1.00e+00)), 4096: ((0.0282, 1.00e+00), (0.0278, 1.00e+00))},
    ("constant 0", "uniform bytes"): {
        16: ((0.282, 5.55e-04), (0.227, 1.04e-03)), 64: ((0.195, 3.21e-03), (0.28, 2.82e-03)),
        1024: ((0.0184, 8.41e-04), (0.0183, 8.33e-04)), 4096: ((0.00365, 1.18e-03), (0.00446, 6.14e-04))},
    ("nyquist full scale", "constant 255"): {
        16: ((0.0021, 2.20e-02), (0.00201, 2.64e-02)), 64: ((0.002, 5.54e-02), (0.002, 6.32e-02)),
        1024: ((0.00515, 3.92e-01), (0.00519, 3.90e-01)), 4096: ((0.0103, 7.96e-01), (0.0104, 7.93e-01))},
    ("quiet then rail to rail", "uniform bytes"): {
        16: ((0.28, 5.10e-04), (0.265, 1.12e-03)), 64: ((0.321, 6.12e-04), (0.321, 6.12e-04)),
        1024: ((0.254, 5.95e-04), (0.254, 5.95e-04)), 4096: ((0.215, 5.83e-04), (0.215, 5.83e-04))},
    ("one impulse", "uniform bytes"): {
        16: ((0.333, 6.68e-04), (0.282, 6.03e-04)), 64: ((0.258, 5.78e-04), (0.268, 5.95e-04)),
        1024: ((0.237, 6.67e-04), (0.237, 6.67e-04)), 4096: ((0.265, 6.63e-04), (0.265, 6.63e-04))},
    ("uniform bytes", "one impulse"): {
        16: ((0.448, 6.25e-04), (0.448, 6.25e-04)), 64: ((0.395, 4.76e-04), (0.395, 4.76e-04)),
        1024: ((0.267, 5.07e-04), (0.267, 5.07e-04)), 4096: ((0.371, 5.68e-04), (0.371, 5.69e-04))},
    ("constant 128/127", "saturated tone"): {
        16: ((0.189, 1.01e-03), (0.286, 1.17e-03)), 64: ((0.0265, 3.57e-03), (0.0889, 3.35e-03)),
        1024: ((0.133, 2.20e-01), (0.133, 2.20e-01)), 4096: ((0.454, 5.94e-01), (0.454, 5.94e-01))},
    ("one impulse", "one impulse"): {
        16: ((0.00253, 5.93e-03), (0.0124, 5.93e-01)), 64: ((0.00341, 1.91e-02), (0.00422, 9.25e-01)),
        1024: ((0.00225, 5.06e-02), (0.0041, 1.32e-01)), 4096: ((0.00283, 3.37e-03), (0.00271, 8.45e-02))},
    ("uniform bytes", "saturated tone", "quiet then rail to rail"): {
        16: ((0.0852, 8.99e-04), (0.306, 1.05e-03)), 64: ((0.0712, 3.36e-03), (0.0785, 1.79e-03)),
        1024: ((0.00365, 1.85e-03), (0.00365, 1.85e-03)), 4096: ((0.393, 3.57e-01), (0.393, 3.57e-01))},
    ("saturated tone", "uniform bytes", "uniform bytes"): {
        16: ((0.265, 8.62e-04), (0.195, 6.12e-04)), 64: ((0.199, 1.20e-03), (0.199, 8.73e-04)),
        1024: ((0.0436, 1.29e-03), (0.0436, 1.29e-03)), 4096: ((0.0111, 7.57e-04), (0.0111, 7.57e-04))},
    ("constant 255", "constant 0", "uniform bytes"): {
        16: ((0.369, 2.04e-03), (0.292, 1.15e-03)), 64: ((0.0753, 3.52e-03), (0.026, 3.85e-03)),
        1024: ((0.366, 3.93e-01), (0.366, 3.95e-01)), 4096: ((0.0269, 8.53e-01), (0.0256, 8.47e-01))},
    ("one impulse", "uniform bytes", "saturated tone"): {
        16: ((0.127, 1.12e-03), (0.235, 7.84e-04)), 64: ((0.0433, 2.79e-03), (0.142, 2.10e-03)),
        1024: ((0.002, 1.48e-03), (0.002, 1.48e-03)), 4096: ((0.5, 4.55e-01), (0.5, 4.55e-01))},
    ("quiet then rail to rail", "uniform bytes", "nyquist full scale"): {
        16: ((0.337, 1.57e-03), (0.337, 1.57e-03)), 64: ((0.0401, 5.05e-03), (0.0401, 5.05e-03)),
        1024: ((0.0185, 2.27e-01), (0.0185, 2.27e-01)), 4096: ((0.0307, 9.57e-01), (0.0307, 9.57e-01))},
    ("one impulse", "one impulse", "one impulse"): {
        16: ((0.00208, 6.73e-03), (0.014, 1.00e+00)), 64: ((0.00217, 1.34e-02), (0.0294, 1.98e-01)),
        1024: ((0.00204, 8.69e-02), (0.002, 9.76e-02)), 4096: ((0.00262, 2.83e-03), (0.00266, 4.92e-02))},
}


def threshold_share(names, nfft, offset):
    """(share, measured margin) of a case."""
    return THRESHOLD_SHARE[names][nfft][[o for o, _ in CONVENTIONS].index(offset)]


@functools.lru_cache(maxsize=None)
def extreme_power_max(names, nfft, offset, scale):
    return float(extreme_reference(names, nfft, offset, scale, "inf")[0].power.max())


def extreme_threshold(names, nfft, offset, scale, kind):
    """float32[nfft], or None for +inf."""
    if kind == "inf":
        return None
    return np.full(nfft, threshold_share(names, nfft, offset)[0] * extreme_power_max(names, nfft, offset, scale), np.float32)


@functools.lru_cache(maxsize=None)
def extreme_reference(names, nfft, offset, scale, kind, single=False):
    """(Cancelled, D_f) of the restatement of one case, computed once and shared."""
    raws = [xi.capture(name) for name in names]
    w = extreme_weights(len(names) - 1, nfft)
    thr = extreme_threshold(names, nfft, offset, scale, kind)
    want = cr.cancel_aux(raws[0], FIRSTS[0], aux_of(raws), w, thr, nfft, EXTREME_SAMPLES, FRAMES_PER_SET, offset, scale, single)
    d_f = None if single else envelope(raws, w, nfft, EXTREME_SAMPLES, FRAMES_PER_SET, offset, scale)
    return want, d_f


# Largest |value(single=True) - value| over the cases of section 2 (both cancellers, both conventions, both kinds), per
# nfft, measured by tests/test_cancel_extremes_host.py: 1.74e-4 at 16 points .. 2.98e-4 at 4096 points, on the triples
# with two full-scale auxiliaries.  Full-scale inputs under |W| up to 4 carry twenty times the parity inputs' rounding
# error into the samples (cr.E32 = 1.25e-5), so the parity band does not carry over; the band is 8 times the figure
# recorded here, the project's own factor for a transform of other radices.  Recorded 10 % above the measurement, so
# that another build of the host's transform still measures no more.
E32_MEASURED = {16: 1.91e-4, 64: 2.58e-4, 1024: 2.94e-4, 4096: 3.28e-4}
# the same for the records: largest record_ratio of the complex64 restatement against the float64 one
REC32_MEASURED = {16: 3.43e-7, 64: 2.88e-7, 1024: 2.52e-7, 4096: 2.42e-7}
TIE_SHARE_MAX = cr.TIE_SHARE_MAX            # 0.2 %


def tie_band(nfft):
    return 8.0 * E32_MEASURED[nfft]


def record_tol(nfft):
    return 8.0 * REC32_MEASURED[nfft]


def tie_share(value, nfft):
    return float(np.mean(er.tie_distance(value) <= tie_band(nfft)))


# The share of a case's restated values that lie inside the tie band, against the cap TIE_SHARE_MAX.  A band of half-width
# b holds 2 b of values that are spread evenly between the integers, and 8 * E32_MEASURED is 1.5e-3 to 2.6e-3: every
# case whose output is noise-like has 0.3 % to 0.5 % of its values in the band, over the cap of 0.2 % by the width of
# the band alone and whatever the seed; the constant pairs and the Nyquist pattern against a constant under offset 127.5
# have nearly every value there (half-integers by construction, shares of 0.6 to 1; the impulse pairs 0.15 to 0.97 once
# their thresholds cut what the impulse adds).  The cap is not raised and no case
# of the issue's list is dropped: the fixed list below names the cases UNDER the cap, every other case is over it, and
# tests/test_cancel_extremes_host.py asserts that the list is exactly that.  Every case, listed or not, is held to the
# same rule on the GPU: bytes within 1 everywhere and equal outside the band.  A listed case must also keep its share.
# {names: ((nfft, offset, kind), ...)}
UNDER_THE_CAP = {
    ("constant 255", "constant 0"): ((16, 128.0, "cut"), (64, 128.0, "cut"), (1024, 127.5, "inf"), (1024, 128.0, "cut"), (1024, 128.0, "inf"),
                                     (4096, 127.5, "inf"), (4096, 128.0, "cut")),
    ("nyquist full scale", "constant 255"): ((16, 128.0, "cut"), (1024, 127.5, "inf"), (1024, 128.0, "cut"), (1024, 128.0, "inf"),
                                             (4096, 127.5, "inf"), (4096, 128.0, "cut"), (4096, 128.0, "inf")),
    ("uniform bytes", "one impulse"): ((16, 128.0, "cut"), (16, 128.0, "inf"), (64, 128.0, "inf"), (1024, 127.5, "inf"), (1024, 128.0, "inf"),
                                       (4096, 127.5, "inf"), (4096, 128.0, "inf")),
    ("one impulse", "one impulse"): ((16, 128.0, "cut"), (16, 128.0, "inf"), (64, 128.0, "cut"), (64, 128.0, "inf"), (1024, 127.5, "inf"),
                                     (1024, 128.0, "cut"), (1024, 128.0, "inf"), (4096, 127.5, "inf"), (4096, 128.0, "cut"), (4096, 128.0, "inf")),
    ("one impulse", "one impulse", "one impulse"): ((16, 128.0, "cut"), (16, 128.0, "inf"), (64, 128.0, "cut"), (64, 128.0, "inf"),
                                                    (1024, 128.0, "cut"), (1024, 128.0, "inf"), (4096, 127.5, "inf"), (4096, 128.0, "cut"),
                                                    (4096, 128.0, "inf")),
}


def under_the_cap(names, nfft, offset, kind):
    return (nfft, offset, kind) in UNDER_THE_CAP.get(names, ())


# ------------------------------------------------------------------------------ 3. past byte 2^32, 4. size_t's ends
FAR_BYTES = 2 ** 32 + 2 ** 20               # one allocation, never filled
FAR_S0 = 2 ** 31                            # the window's first sample: byte 2^32
FAR_NFFT = (64, 4096)
FAR_SAMPLES = cr.PARITY_SAMPLES
SET_NFFT = 256


@functools.lru_cache(maxsize=None)
def far_capture():
    """The bytes that go at byte 2^32: capture a of the parity pair, FAR_SAMPLES samples behind FIRSTS[2]."""
    raw = cs.parity_pair()[0][:2 * (FIRSTS[2] + FAR_SAMPLES)].copy()
    raw.setflags(write=False)
    return raw


# The window's a, b and c are one capture at three first samples, not the pair the parity thresholds were tuned on: at 64
# points the parity threshold has a restated power within 7e-5 (one auxiliary) and 3e-6 (two) of it.  There the
# threshold is the parity one times the factor nearest 1, in steps of 0.01, that keeps every power cr.NEAR_TIE away
# (tests/test_cancel_extremes_host.py asserts the margin): the parity comparison holds n_excised on every frame.
FAR_THRESHOLD_FACTOR = {(1, 64): 1.12, (1, 4096): 1.0, (2, 64): 1.13, (2, 4096): 1.0}


def far_threshold(n_aux, nfft):
    return ((cr if n_aux == 1 else c2).parity_threshold(nfft) * np.float32(FAR_THRESHOLD_FACTOR[(n_aux, nfft)])).astype(np.float32)


@functools.lru_cache(maxsize=None)
def far_reference(n_aux, nfft):
    """The restatement of the window as a small capture of its own: a, b (and c) are far_capture() at FIRSTS, under the
    parity weights of the canceller and far_threshold."""
    raw = far_capture()
    mod = cr if n_aux == 1 else c2
    return cr.cancel_aux(raw, FIRSTS[0], [(raw, first) for first in FIRSTS[1:1 + n_aux]], mod.parity_weights(nfft),
                         far_threshold(n_aux, nfft), nfft, FAR_SAMPLES, cr.PARITY_FRAMES_PER_SET)


def per_frame_weights(n_aux, nfft, n_frames, n_nan):
    """A set per frame, the parity sets taken round and round, and n_nan sets of NaN behind them."""
    w = (cr if n_aux == 1 else c2).parity_weights(nfft)
    sets = w[np.arange(n_frames) % w.shape[0]]
    return np.concatenate([sets, np.full((n_nan,) + w.shape[1:], np.nan + 1j * np.nan, np.complex64)])
