"""Saturated and degenerate captures for the short-time kernels (gj_ridge_dev, gj_chirp_dev, gj_sk_dev) and the two
excisors (gj_excise_dev, gj_excise_chirp_dev): the eight captures of tests/test_extremes_gpu.py regenerated at 2^15
samples by the same recipes, and the constants of their tests.  Not a test module: tests/test_extremes_host.py and
tests/extremes/test_round6_gpu.py import it.

What these inputs have and the parity inputs never do is EXACT ties: an impulse has a flat spectrum (and a de-chirp
leaves an impulse an impulse), a constant or Nyquist capture puts all its power into three bins of the Hann-windowed
transform and leaves exact mid-level when that line is notched.  tests/test_extremes_host.py computes, in float64, where
the ties are; the GPU tests take that from here and never from the GPU's own result.
"""
import functools

import numpy as np

import chirp_restatement as cr
import excise_restatement as er
import ridge_restatement as rr
import skurt_restatement as sr

SAMPLES = 1 << 15
FIRST = 1                                   # odd on purpose
GUARD = 2
RAIL_AT = 3 * SAMPLES // 4                  # the rail-to-rail part of "quiet then rail to rail"
IMPULSE_AT = SAMPLES // 2 + 1               # an odd sample
CONVENTIONS = er.CONVENTIONS                # (127.5, 1/127.5) and (128, 1/128)
NAMES = ("constant 255", "constant 0", "constant 128/127", "nyquist full scale", "uniform bytes", "saturated tone",
         "quiet then rail to rail", "one impulse")
UNIFORM_SEED = 11                           # no seed frees 4094 frames of chance ties: CHANCE_TIE_SHARE_CAP below
SEED = 11

RIDGE_NFFT = rr.PARITY_NFFT                 # ridge and kurtosis: 16 .. 4096
CHIRP_NFFT = (16, 64, 1024, 4096)           # chirp and the two excisors
SK_M = (2, 5, 64)


def hops(nfft):
    return (nfft // 2 + 37, nfft // 2)


def _interleave(i, q):
    raw = np.empty(2 * i.size, np.uint8)
    raw[0::2], raw[1::2] = i, q
    return raw


@functools.lru_cache(maxsize=None)
def capture(name):
    """2^15 samples.  Read-only uint8."""
    n, t = SAMPLES, np.arange(SAMPLES)
    if name == "constant 255":
        raw = np.full(2 * n, 255, np.uint8)
    elif name == "constant 0":
        raw = np.zeros(2 * n, np.uint8)
    elif name == "constant 128/127":
        raw = _interleave(np.full(n, 128, np.uint8), np.full(n, 127, np.uint8))
    elif name == "nyquist full scale":
        raw = _interleave(np.where(t & 1, 255, 0).astype(np.uint8), np.where(t & 1, 0, 255).astype(np.uint8))
    elif name == "uniform bytes":
        raw = np.random.RandomState(UNIFORM_SEED).randint(0, 256, 2 * n).astype(np.uint8)
    elif name == "saturated tone":
        rng = np.random.RandomState(SEED + 1)
        sat = 400.0 * np.exp(2j * np.pi * 0.031 * t) + rng.normal(0, 30, n) + 1j * rng.normal(0, 30, n)   # clips hard
        raw = _interleave((np.clip(np.rint(sat.real), -128, 127) + 128).astype(np.uint8),
                          (np.clip(np.rint(sat.imag), -128, 127) + 128).astype(np.uint8))
    elif name == "quiet then rail to rail":
        rng = np.random.RandomState(SEED + 2)
        raw = (np.clip(np.rint(rng.normal(0, 2.0, 2 * n)), -128, 127) + 128).astype(np.uint8)
        raw[2 * RAIL_AT:] = np.where(rng.randint(0, 2, 2 * (n - RAIL_AT)) == 1, 255, 0)
    elif name == "one impulse":
        raw = np.full(2 * n, 128, np.uint8)
        raw[2 * IMPULSE_AT] = 255
    else:
        raise ValueError(name)
    raw.setflags(write=False)
    return raw


# ---------------------------------------------------------------------------------------------------- ridge
@functools.lru_cache(maxsize=None)
def ridge_reference(name, nfft, hop, offset, scale):
    """(records, margin) of every frame that fits from FIRST on, computed once and shared."""
    rec, margin = rr.ridge(capture(name), nfft, hop, FIRST, None, GUARD, offset, scale)
    rec.setflags(write=False)
    margin.setflags(write=False)
    return rec, margin


def frames_with_the_impulse(nfft, hop, n_frames):
    """Frames of the geometry that hold sample IMPULSE_AT under a non-zero window value (w[0] = 0)."""
    s = FIRST + hop * np.arange(n_frames)
    return np.flatnonzero((s < IMPULSE_AT) & (IMPULSE_AT < s + nfft))


def ridge_not_clear(name, nfft, hop, offset, scale):
    """Frames whose peak bin is decided by rounding: the restatement's margin is under rr.NEAR_TIE."""
    return np.flatnonzero(ridge_reference(name, nfft, hop, offset, scale)[1] < rr.NEAR_TIE)


def frame_spectrum(name, nfft, start, offset, scale, q=0):
    """P[k] of the one frame that starts at sample `start`, de-chirped at rate q, in float64."""
    x = rr.unpack(capture(name), offset, scale)[start:start + nfft]
    return np.abs(np.fft.fft(x * rr.hann(nfft) * cr.dechirp(q, nfft))) ** 2


# ---------------------------------------------------------------------------------------------------- chirp
def chirp_rate_sets(nfft):
    """The single rate 0, a one-sided grid and the lower limit.  No set holds q and -q: a constant capture (and the
    Nyquist pattern) gives them mirrored spectra, an exact tie of two RATES that says nothing about a kernel."""
    return ((0, 1, 1), (1, 2, 3), (-(nfft * nfft // 2), 3, 2))


@functools.lru_cache(maxsize=None)
def chirp_reference(name, nfft, hop, rates, offset, scale):
    scan = cr.chirp_scan(capture(name), nfft, hop, rates, FIRST, None, GUARD, offset, scale)
    for a in scan:
        a.setflags(write=False)
    return scan


def chirp_not_clear(name, nfft, hop, rates, offset, scale):
    scan = chirp_reference(name, nfft, hop, rates, offset, scale)
    return np.flatnonzero((scan.rate_margin < cr.NEAR_TIE) | (scan.bin_margin < cr.NEAR_TIE))


# The captures made of random draws ("uniform bytes", "saturated tone", "quiet then rail to rail") have frames whose
# two best bins or rates lie within NEAR_TIE by chance -- and "quiet then rail to rail", whose quiet part is a few small
# integers, exact ones -- at the rate tests/stft_scale_inputs.py found for 400 000 frames: about one frame in a thousand
# at 16 points.  No seed removes them from 4094 frames x 3 rate sets x 2 conventions.  They are treated like the
# structural ties: the GPU's choice must be a candidate.  Largest share of one case, measured by
# tests/test_extremes_host.py: 2 of 474 frames ("uniform bytes", 64 points, hop 69, rates 1 3 5, offset 128); over all
# cases of a capture it is 29 frames of 38 796.  The cap, a condition on these inputs, is twice the largest.
CHANCE_TIE_SHARE_MEASURED = 4.22e-3
CHANCE_TIE_SHARE_CAP = 2.0 * CHANCE_TIE_SHARE_MEASURED
RANDOM_NAMES = ("uniform bytes", "saturated tone", "quiet then rail to rail")


# ---------------------------------------------------------------------------------------------------- kurtosis
def sk_cases(nfft):
    """(hop, M) with at least one row inside 2^15 samples: M = 64 needs 63 hops and a frame."""
    return [(hop, m) for hop in hops(nfft) for m in SK_M if sr.rows_that_fit(2 * SAMPLES, FIRST, nfft, hop, m) >= 1]


@functools.lru_cache(maxsize=None)
def frame_powers(name, nfft, hop, offset, scale):
    raw = capture(name)
    p = sr.frame_powers(raw, nfft, hop, FIRST, rr.frames_that_fit(raw.size, FIRST, nfft, hop), offset, scale)
    p.setflags(write=False)
    return p


# ---------------------------------------------------------------------------------------------------- excisors
def chirp_identity_rates(nfft):
    """The rates of the chirp excisor's identity runs, each on every frame."""
    return (0, 3, -(nfft * nfft // 2))


# Largest |y_complex64 - y_float64| of the two excisors' restatements over the notch cases below (every capture, size and
# convention that is run), measured by tests/test_extremes_host.py with single=True: 6.12e-5 through the chirp excisor
# and 6.05e-5 through the plain one, both on "saturated tone" at 4096 points, against er.E32 = 2.75e-5 and
# xr.E32_CHIRP = 3.45e-5 on the parity inputs (full-scale lines carry more rounding error into the samples that
# remain).  The band and the cap follow by the rule of er.TIE_BAND and xr.TIE_SHARE_CAP.
E32_MEASURED = 6.12e-5
E32 = 6.2e-5
TIE_BAND = 8 * E32                          # 4.96e-4
TIE_SHARE_CAP = 4 * TIE_BAND                # 1.98e-3: a condition on the inputs, not a tolerance

# Notching with the flat threshold er.parity_threshold(nfft, scale) (16 x the floor of 6.25-LSB noise) through
# gj_excise_dev.  A case runs under both conventions unless it is listed here: under offset 127.5 its reference has more
# bytes inside the tie band than TIE_SHARE_CAP allows (tests/test_extremes_host.py asserts that of every entry, and that
# every case that does run stays inside the cap), so the comparison would hold the kernel to nothing there.
NOTCH_128_ONLY = {
    ("constant 255", 16): "the notched DC line leaves exact mid-level: 127.5, every byte a tie",
    ("constant 255", 64): "the notched DC line leaves exact mid-level: 127.5, every byte a tie",
    ("constant 255", 1024): "the notched DC line leaves exact mid-level: 127.5, every byte a tie",
    ("constant 255", 4096): "the notched DC line leaves exact mid-level: 127.5, every byte a tie",
    ("constant 0", 16): "the notched DC line leaves exact mid-level: 127.5, every byte a tie",
    ("constant 0", 64): "the notched DC line leaves exact mid-level: 127.5, every byte a tie",
    ("constant 0", 1024): "the notched DC line leaves exact mid-level: 127.5, every byte a tie",
    ("constant 0", 4096): "the notched DC line leaves exact mid-level: 127.5, every byte a tie",
    ("constant 128/127", 4096): "at 4096 points even the DC of 0.5 LSB is over the threshold: notched, mid-level is left",
    ("one impulse", 4096): "at 4096 points even the DC of 0.5 LSB is over the threshold: notched, mid-level is left",
    ("nyquist full scale", 4096): "the notched Nyquist line leaves exact mid-level: 127.5, every byte a tie",
    ("uniform bytes", 16): "58 618 of 65 504 bins are notched: what is left lies within a few LSB of 127.5 (share 2.9e-2)",
    ("quiet then rail to rail", 16): "the quiet part is a few LSB around 127.5 (share 8.0e-2)",
}
# ... and these run under neither: under offset 128 the Nyquist pattern is -128 / +127, its notched line leaves a DC of
# -0.5 LSB, which at these sizes is under the threshold and stays: 127.5 again.  At 4096 points that DC is notched too.
NOTCH_NEVER = {
    ("nyquist full scale", 16): "under 128 the line's removal leaves the DC of -0.5 LSB: 127.5, every byte a tie",
    ("nyquist full scale", 64): "under 128 the line's removal leaves the DC of -0.5 LSB: 127.5, every byte a tie",
    ("nyquist full scale", 1024): "under 128 the line's removal leaves the DC of -0.5 LSB: 127.5, every byte a tie",
}


def _cases(only_128, never):
    out = []
    for name in NAMES:
        for nfft in CHIRP_NFFT:
            if (name, nfft) in never:
                continue
            for offset, scale in CONVENTIONS:
                if offset == 127.5 and (name, nfft) in only_128:
                    continue
                out.append((name, nfft, offset, scale))
    return out


def notch_cases():
    """(name, nfft, offset, scale) of every notch case of gj_excise_dev that runs."""
    return _cases(NOTCH_128_ONLY, NOTCH_NEVER)


# The same through gj_excise_chirp_dev with the rates 0, 3 and -N^2/2 on consecutive frames: a third of the frames are
# the plain excisor's, the others spread a line over many bins, part of which stays under the threshold.
_THIRD = "the frames at rate 0 notch the whole line: a third of the bytes are exact mid-level, 127.5 (share 0.31 to 0.37)"
CHIRP_NOTCH_128_ONLY = {
    ("constant 255", 16): _THIRD, ("constant 255", 64): _THIRD, ("constant 255", 1024): _THIRD, ("constant 255", 4096): _THIRD,
    ("constant 0", 16): _THIRD, ("constant 0", 64): _THIRD, ("constant 0", 1024): _THIRD, ("constant 0", 4096): _THIRD,
    ("nyquist full scale", 4096): _THIRD,
    ("uniform bytes", 16): "nearly every bin is notched: what is left lies within a few LSB of 127.5 (share 3.0e-2)",
    ("quiet then rail to rail", 16): "the quiet part is a few LSB around 127.5 (share 7.6e-2)",
    ("quiet then rail to rail", 64): "the quiet part is a few LSB around 127.5 (share 2.2e-3)",
}
_HALF_LSB = "under 128 the frames at rate 0 leave the DC of -0.5 LSB: 127.5 (share 7.7e-3 to 4.2e-2)"
CHIRP_NOTCH_NEVER = {("nyquist full scale", 16): _HALF_LSB, ("nyquist full scale", 64): _HALF_LSB, ("nyquist full scale", 1024): _HALF_LSB}


def chirp_notch_cases():
    return _cases(CHIRP_NOTCH_128_ONLY, CHIRP_NOTCH_NEVER)


def chirp_notch_rates(nfft):
    """One rate per frame of the range FIRST .. end: 0, 3, -N^2/2, 0, ..."""
    cyc = chirp_identity_rates(nfft)
    return np.array([cyc[f % len(cyc)] for f in range(er.frames_loop(SAMPLES - FIRST, nfft))], np.int32)


@functools.lru_cache(maxsize=None)
def chirp_notch_reference(name, nfft, offset, scale, single=False):
    import excise_chirp_restatement as xr
    return xr.excise_chirp(capture(name), er.parity_threshold(nfft, scale), chirp_notch_rates(nfft), nfft, FIRST, None, offset, scale, single)


# No notch case above leaves the uint8 range before rounding (tests/test_extremes_host.py asserts it), so the clamp has
# its own: er.clamp_capture() -- a 127-LSB square wave on both components -- with everything but its fundamental
# notched, whose 4 / pi * 127 LSB overshoot both ends.
CLAMP_NFFT = er.CLAMP_NFFT


@functools.lru_cache(maxsize=None)
def notch_reference(name, nfft, offset, scale, single=False):
    return er.excise(capture(name), er.parity_threshold(nfft, scale), nfft, FIRST, None, offset, scale, single)


@functools.lru_cache(maxsize=None)
def clamp_reference(nfft, single=False):
    return er.excise(er.clamp_capture(), er.clamp_threshold(nfft), nfft, FIRST, None, 127.5, 1.0 / 127.5, single)


def frames_clear_of_the_threshold(want, thr):
    """Frames none of whose bins lies within er.NEAR_TIE (relative) of its threshold."""
    thr = np.asarray(thr, np.float32).astype(np.float64)
    ok = np.isfinite(thr) & (thr > 0)
    if not ok.any():
        return np.ones(want.records.size, bool)
    return np.min(np.abs(want.power[:, ok] / thr[None, ok] - 1.0), axis=1) >= er.NEAR_TIE
