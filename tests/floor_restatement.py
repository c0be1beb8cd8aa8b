"""The noise-floor rule of include/gpsjam.h (gj_power_threshold_dev) restated in numpy float32, and the inputs the host
and GPU tests hold it to -- test infrastructure, never imported by the product.

    baseline  = numpy.percentile(power, pct) with numpy's float32 'linear' rule, 1.0 if <= 0
    threshold = baseline * 10^(rise_db / 10)
    mask[c]   = power[c] > threshold,  stats = {baseline, threshold, count of the mask}

numpy's rule on a float32 map, every operation rounded to float32 on its own: q = float32(pct) / float32(100), virtual
index v = float32(n - 1) * q, lo = floor(v), hi = min(lo + 1, n - 1), g = v - float32(lo), a and b the values of ranks lo
and hi, d = b - a, and the lerp  b - d * (1 - g)  where g >= 0.5,  a + d * g  elsewhere.  A NaN anywhere makes the
baseline NaN (then the threshold is NaN, the mask empty).  tests/test_floor_result_host.py holds `baseline` to
numpy.percentile on every map below.

`once_rounded` is the same lerp with the product and the sum rounded ONCE (what a fused multiply-add gives).  Nothing is
compared with it: it only picks the maps on which one rounding and two roundings differ (SENSITIVE_MAPS,
SENSITIVE_CAPTURES), so that a kernel that fuses the lerp cannot pass.

Denormal powers are out of scope: K1 adds eps = 1e-10 to every chunk power, so no power map holds one."""
import functools
from fractions import Fraction

import numpy as np

f32 = np.float32

# --------------------------------------------------------------------------------------- the rule


def virtual_index(n: int, pct: float):
    """(lo, hi, g) of numpy's 'linear' method on a float32 array of n values."""
    q = f32(pct) / f32(100)
    v = f32(f32(n - 1) * q)
    lo = min(int(np.floor(v)), n - 1)
    hi = min(lo + 1, n - 1)
    return lo, hi, f32(v - f32(lo))


def lerp(a, b, g):
    """numpy's _lerp in float32: the product and the sum are rounded separately."""
    a, b, g = f32(a), f32(b), f32(g)
    with np.errstate(invalid="ignore", over="ignore"):
        d = f32(b - a)
        if g >= f32(0.5):
            return f32(b - f32(d * f32(f32(1) - g)))
        return f32(a + f32(d * g))


def _round_f32(x: Fraction):
    """The float32 nearest to the exact rational x, ties to even."""
    c = f32(float(x))
    cands = [np.nextafter(c, f32(-np.inf)), c, np.nextafter(c, f32(np.inf))]
    cands = [k for k in cands if np.isfinite(k)]
    best = min(abs(Fraction(float(k)) - x) for k in cands)
    near = [k for k in cands if abs(Fraction(float(k)) - x) == best]
    if len(near) > 1:
        near = [k for k in near if (int(k.view(np.uint32)) & 1) == 0]
    return near[0]


def once_rounded(a, b, g):
    """The lerp with its product and sum evaluated exactly and rounded once (finite a, b only).  d and 1 - g are float32
    values as in `lerp`.  Used to choose inputs, never as a reference."""
    a, b, g = f32(a), f32(b), f32(g)
    d = Fraction(float(f32(b - a)))
    if g >= f32(0.5):
        return _round_f32(Fraction(float(b)) - d * Fraction(float(f32(f32(1) - g))))
    return _round_f32(Fraction(float(a)) + d * Fraction(float(g)))


def neighbours(pm: np.ndarray, pct: float):
    """(a, b, g): the two ranks the rule reads and the weight between them."""
    lo, hi, g = virtual_index(pm.size, pct)
    s = np.sort(np.asarray(pm, f32))
    return s[lo], s[hi], g


def baseline(pm: np.ndarray, pct: float):
    """numpy.percentile(pm, pct) restated (before the `<= 0 -> 1.0` rule)."""
    pm = np.asarray(pm, f32)
    if np.isnan(pm).any():
        return f32(np.nan)
    return lerp(*neighbours(pm, pct))


def is_sensitive(pm: np.ndarray, pct: float) -> bool:
    a, b, g = neighbours(pm, pct)
    return bool(once_rounded(a, b, g) != lerp(a, b, g))


def ratio_of(rise_db: float):
    return f32(10.0 ** (float(f32(rise_db)) / 10.0))


def floor_rule(pm: np.ndarray, pct: float, rise_db: float):
    """(baseline, threshold, count, mask) as the header states them."""
    pm = np.asarray(pm, f32)
    base = baseline(pm, pct)
    if base <= 0:
        base = f32(1.0)
    with np.errstate(invalid="ignore", over="ignore"):
        thr = f32(base * ratio_of(rise_db))
        mask = pm > thr
    return base, thr, int(np.count_nonzero(mask)), mask.astype(np.uint8)


# --------------------------------------------------------------------------------------- inputs: maps
GRID_N = (1, 2, 3, 7, 20, 21, 64, 257, 1000, 16383, 16384, 16385, 40000, 100003)
GRID_PCT = (0, 0.1, 1, 2.5, 5, 10, 25, 33.3, 50, 66.6, 75, 90, 95, 99, 99.9, 100)
GRID_RISE = (0, 6, 12.3)
KINDS = ("uniform", "normal_zeros", "five_values", "constant")


@functools.lru_cache(maxsize=None)
def grid_map(kind: str, n: int) -> np.ndarray:
    rng = np.random.default_rng(1000 * KINDS.index(kind) + 7 + n)
    if kind == "uniform":                      # the suite's own maps: dense values in [50, 150)
        pm = rng.uniform(50.0, 150.0, n)
    elif kind == "normal_zeros":               # both signs, every seventh value an exact zero
        pm = rng.standard_normal(n) * 3.0
        pm[::7] = 0.0
    elif kind == "five_values":                # long runs of equal keys: rank lo + 1 is often rank lo's value
        pm = rng.choice(np.array([0.75, 3.0, 3.0000002, 41.5, 1000.0]), n)
    else:
        pm = np.full(n, 73.25)
    out = pm.astype(f32)
    out.setflags(write=False)
    return out


SHORT_N = tuple(range(2, 65))
SHORT_PER_N = 8
SHORT_PCT = (5, 25)


@functools.lru_cache(maxsize=None)
def short_map(n: int, seed: int) -> np.ndarray:
    """A short capture's power map: n chunk powers spread over a decade."""
    rng = np.random.default_rng(50_000 + 97 * n + seed)
    out = (10.0 ** rng.uniform(1.0, 2.0, n)).astype(f32)
    out.setflags(write=False)
    return out


def short_maps():
    return [(n, k) for n in SHORT_N for k in range(SHORT_PER_N)]


# (n, seed, pct): short maps on which one rounding and two roundings of the lerp differ -- found by searching seeds
# 100 .. on the CPU with n = 2 + (7919 seed) mod 63 (about 1 % of random short maps qualify);
# test_floor_result_host.py checks that each still does.  No map is sensitive at 25, 50 or 75 %: q is a power of two
# there, so g is a multiple of 1/4 and the product d * g is exact.
SENSITIVE_MAPS = (
    (8, 129, 5), (3, 368, 5), (7, 391, 5), (55, 415, 5), (2, 441, 5), (9, 497, 5),
    (15, 500, 5), (4, 736, 5), (22, 745, 5), (5, 978, 5), (10, 1054, 5), (28, 1063, 5),
    (47, 306, 1), (27, 317, 1), (39, 323, 1), (50, 339, 1), (27, 128, 10), (2, 189, 10),
    (2, 252, 10), (5, 285, 10), (8, 192, 33.3), (2, 315, 33.3), (3, 494, 33.3), (2, 567, 33.3),
    (24, 473, 95), (29, 612, 95), (8, 696, 95), (13, 709, 95), (13, 142, 2.5), (23, 294, 2.5),
    (23, 357, 2.5), (5, 411, 2.5), (32, 204, 66.6), (6, 275, 66.6), (24, 284, 66.6), (20, 324, 66.6),
    (10, 109, 90), (45, 263, 90), (4, 295, 90), (7, 328, 90),
)


def special_maps():
    """name -> (map, percentiles).  NaN anywhere: baseline and threshold NaN, nothing above.  Infinities at either end,
    all values negative (baseline <= 0 -> 1.0), both zeros, one chunk."""
    rng = np.random.default_rng(4242)
    body = rng.uniform(50.0, 150.0, 41).astype(f32)
    out = {}
    for where, i in (("first", 0), ("middle", 20), ("last", 40)):
        pm = body.copy()
        pm[i] = np.nan
        out[f"nan {where}"] = (pm, (0, 5, 25, 50, 100))
    pm = body.copy()
    pm[13] = np.inf
    out["+inf largest"] = (pm, (95, 100))
    pm = body.copy()
    pm[29] = -np.inf
    out["-inf smallest"] = (pm, (0, 5))
    out["all negative"] = (-body, (0, 5, 25, 50, 100))
    pm = body.copy() - f32(100)
    pm[3], pm[4], pm[30] = -0.0, 0.0, -0.0
    out["signed zeros"] = (pm, tuple(GRID_PCT))
    out["zeros only"] = (np.array([0.0, -0.0, -0.0, 0.0, -0.0], f32), (0, 5, 25, 50, 100))
    out["one chunk"] = (np.array([87.5], f32), tuple(GRID_PCT))
    out["one chunk, negative"] = (np.array([-2.0], f32), tuple(GRID_PCT))
    return out


# --------------------------------------------------------------------------------------- inputs: captures
CAPTURE_CHUNK = 1024


@functools.lru_cache(maxsize=None)
def capture(n_chunks: int, seed: int) -> np.ndarray:
    """uint8 I/Q of n_chunks x 1024 bytes; the noise level is drawn per chunk so that the chunk powers spread over a
    decade (sigma over sqrt(10))."""
    rng = np.random.default_rng(900_000 + 131 * n_chunks + seed)
    sigma = 4.0 * 10.0 ** rng.uniform(0.0, 0.5, n_chunks)
    g = rng.standard_normal((n_chunks, CAPTURE_CHUNK)) * sigma[:, None] + 127.5
    out = np.clip(np.rint(g), 0, 255).astype(np.uint8).reshape(-1)
    out.setflags(write=False)
    return out


def capture_power(raw: np.ndarray, chunk_bytes: int = CAPTURE_CHUNK, eps=1e-10) -> np.ndarray:
    """exact_restatement.chunk_power for whole chunks, vectorised: float32(sum / (4 n)) + float32(eps), the sum an exact
    integer."""
    v = 2 * raw.astype(np.int64).reshape(-1, chunk_bytes) - 255
    s = (v * v).sum(axis=1)
    n = chunk_bytes // 2
    return (np.array([int(x) / (4.0 * n) for x in s]).astype(f32) + f32(eps)).astype(f32)


def widen(raw: np.ndarray, factor: int = 64, chunk_bytes: int = CAPTURE_CHUNK) -> np.ndarray:
    """Every chunk of the capture repeated `factor` times in place: chunks of factor * chunk_bytes bytes with the SAME
    power map bit for bit (sum and count both grow by the factor; the quotient is rounded once).  The fused scan and the
    part kernels take chunk sizes that are multiples of 65536 only, so this is how a short capture's map reaches them."""
    return np.ascontiguousarray(np.repeat(raw.reshape(-1, 1, chunk_bytes), factor, axis=1)).reshape(-1)


# (n_chunks, seed): captures whose exact power map is sensitive at 5 % -- searched on the CPU like SENSITIVE_MAPS
SENSITIVE_CAPTURES = ((25, 148), (49, 223), (18, 470), (13, 520), (27, 632), (27, 758), (7, 1084), (59, 1383), (48, 1430),
                      (32, 1968))


def other_captures():
    """About a hundred captures that are not on the list: two for every other length, seeds 0 and 1."""
    return [(n, k) for n in range(2, 65) for k in range(2) if (n + k) % 5 != 0]
