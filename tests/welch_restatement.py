"""K2, the Welch waterfall (gj_welch_dev, include/gpsjam.h), restated in plain numpy, with the error measure, the
geometries, the captures and the budgets of the K2 tests.  Not a test module: tests/test_welch_host.py and
tests/welch_sizes/test_round6_gpu.py import it.

    x[t]    = ((I_t - offset) + j (Q_t - offset)) * scale
    chunk c = samples [c C, c C + C), C = chunk_samples; a trailing piece is kept when it holds nperseg samples
    segment s of a chunk of L samples starts at s N/2, s = 0 .. (L - N) / (N/2)  (50 % overlap, no padding)
    P_s[k]  = |fft(w (x_s - mean(x_s)))[k]|^2 / (fs sum(w^2)),  w[n] = 0.5 - 0.5 cos(2 pi n / N)  (periodic Hann)
    row c   = mean over s of P_s                     (unshifted: bin k is frequency k fs / N)

``single=False`` is that, in float64.  ``single=True`` is the same quantity in the form K2 computes it, in float32 and
complex64: the integers v = 2u - 2 offset are windowed, transformed, and the mean is removed BEHIND the transform (the
periodic Hann window has three non-zero DFT bins: N/2 at 0, -N/4 at 1 and N-1, so fft(w (v - m)) differs from fft(w v)
by S/2 on bin 0 and -S/4 on bins 1 and N-1, S the exact integer sum of the segment); |X|^2 is added segment by segment
and everything else -- (scale / 2)^2, 1 / (fs sum w^2), 1 / nseg -- is one factor at the end.  The float32 form is what
the budgets E32 are measured from; a GPU result never enters a tolerance.
"""
import functools

import numpy as np
from scipy import fft as sfft

from gpsjam.synth import StreamSpec, generate

FS = 2.048e6
SIZES = (16, 32, 64, 128, 256, 512, 1024, 2048, 4096)
BLOCK_POINTS = 4096                         # points a K2 workgroup transforms per step: B = 4096 / nperseg groups
CONVENTIONS = ((127.5, 1.0 / 127.5), (128.0, 1.0 / 128.0))


# ---------------------------------------------------------------------------------------------------- the definition
def hann(n):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / n)


def rows_that_fit(nbytes, chunk_samples, nperseg):
    """gj_welch_rows as the loop it abbreviates: full chunks, and a trailing piece that holds nperseg samples."""
    if chunk_samples < 1 or nperseg < 1:
        return 0
    rows, left = 0, nbytes
    while left >= 2 * chunk_samples:
        rows, left = rows + 1, left - 2 * chunk_samples
    return rows + (1 if left >= 2 * nperseg else 0)


def segments_in(length, nperseg):
    return (length - nperseg) // (nperseg // 2) + 1 if length >= nperseg else 0


def segments(v, nperseg):
    """[nseg][nperseg]: the overlapping segments of one chunk's samples (a view)."""
    return np.lib.stride_tricks.sliding_window_view(v, nperseg)[::nperseg // 2]


def unpack(raw, offset=127.5, scale=1.0 / 127.5):
    u = np.asarray(raw, np.uint8).astype(np.float64)
    return ((u[0::2] - offset) + 1j * (u[1::2] - offset)) * scale


def periodograms_of(segs, fs=FS, window=None, means=None):
    """P_s[k] in float64 of segments given as complex samples; ``window`` and ``means`` replace the definition's (the
    host test's mutants use them).  The density scale is the periodic Hann window's whatever ``window`` is."""
    n = segs.shape[1]
    w = hann(n) if window is None else window
    m = np.mean(segs, axis=1) if means is None else means
    return np.abs(np.fft.fft((segs - m[:, None]) * w[None, :], axis=1)) ** 2 / (fs * np.sum(hann(n) ** 2))


def _k2_power(raw_chunk, nperseg, offset):
    """|X_s[k]|^2 of K2's form in float32, in units of v = 2u - 2 offset: [nseg][nperseg]."""
    u = np.asarray(raw_chunk, np.uint8).astype(np.int64)
    o2 = int(round(2 * offset))
    assert o2 == 2 * offset, "offset is a multiple of 0.5 (gj_set_unpack)"
    vi, vq = segments(2 * u[0::2] - o2, nperseg), segments(2 * u[1::2] - o2, nperseg)
    w = hann(nperseg).astype(np.float32)
    x = np.empty(vi.shape, np.complex64)
    x.real, x.imag = w[None, :] * vi.astype(np.float32), w[None, :] * vq.astype(np.float32)
    spec = sfft.fft(x, axis=1)
    assert spec.dtype == np.complex64
    s = (vi.sum(axis=1).astype(np.float32) + 1j * vq.sum(axis=1).astype(np.float32)).astype(np.complex64)   # exact integers
    spec[:, 0] -= np.float32(0.5) * s
    spec[:, 1] += np.float32(0.25) * s
    spec[:, nperseg - 1] += np.float32(0.25) * s
    return spec.real * spec.real + spec.imag * spec.imag


def periodograms(raw_chunk, nperseg, offset=127.5, scale=1.0 / 127.5, fs=FS, single=False):
    """P_s[k] of every segment of one chunk's bytes, [nseg][nperseg]: float64, or K2's form in float32.  (In float32
    each segment is scaled here; ``welch`` scales once, behind the sum over the segments, as K2 does.)"""
    if single:
        f = np.float32((0.5 * scale) ** 2 / (fs * 0.375 * nperseg))
        return _k2_power(raw_chunk, nperseg, offset) * f
    return periodograms_of(segments(unpack(raw_chunk, offset, scale), nperseg), fs)


def welch(raw, nperseg, chunk_samples, offset=127.5, scale=1.0 / 127.5, fs=FS, single=False):
    """The waterfall of the bytes ``raw``: [rows_that_fit][nperseg], unshifted; float64, or float32 in K2's form."""
    raw = np.asarray(raw, np.uint8)
    rows = rows_that_fit(raw.size, chunk_samples, nperseg)
    out = np.empty((rows, nperseg), np.float32 if single else np.float64)
    for c in range(rows):
        piece = raw[2 * c * chunk_samples:2 * (c + 1) * chunk_samples]
        if single:
            p = _k2_power(piece, nperseg, offset)
            total = np.add.accumulate(p, axis=0, dtype=np.float32)[-1]          # segment by segment, in float32
            out[c] = total * np.float32((0.5 * scale) ** 2 / (fs * 0.375 * nperseg * p.shape[0]))
        else:
            out[c] = periodograms(piece, nperseg, offset, scale, fs).mean(axis=0)
    return out


# ---------------------------------------------------------------------------------------------------- the error measure
def full_scale(nperseg, fs=FS):
    """The density a full-scale tone puts into its bin (tests/test_extremes_gpu.py test_extreme_k2_welch)."""
    return 1.0 / (fs * 0.375 * nperseg) * nperseg ** 2 * 2.0


def floor(nperseg):
    """The absolute floor of test_extreme_k2_welch for spectra that are empty: 5e-8 of a full-scale line's density."""
    return 5e-8 * full_scale(nperseg)


def denominators(truth):
    """What a bin's difference is measured against: the bin, its row's mean level, or the floor, whichever is largest.
    K2 removes the mean behind the transform, so the rounding noise of the un-removed DC line lands in EVERY bin: an
    error of the size of the row's level times the float32 spacing is what a correct float32 Welch of this form has,
    however small the bin."""
    truth = np.asarray(truth, np.float64)
    return np.maximum(np.maximum(truth, truth.mean(axis=1, keepdims=True)), floor(truth.shape[1]))


def errors(got, truth):
    """e[row][k] = |got - truth| / max(truth[k], mean(truth row), FLOOR)."""
    got, truth = np.asarray(got, np.float64), np.asarray(truth, np.float64)
    assert got.shape == truth.shape and truth.ndim == 2
    return np.abs(got - truth) / denominators(truth)


def case_error(got, truth):
    """The largest e over the case's rows."""
    return float(np.max(errors(got, truth)))


# ---------------------------------------------------------------------------------------------------- geometry
SHAPES = ("one", "idle", "full", "plus1", "odd", "split2", "split5")
MIN_SPLIT = {"split2": 2, "split5": 5}      # workgroups per chunk the two last shapes must reach on the device


def groups(nperseg):
    return BLOCK_POINTS // nperseg


def shape_nseg(nperseg, shape):
    b = groups(nperseg)
    return {"one": 1, "idle": b - 1, "full": b, "plus1": b + 1, "odd": 2 * b + 1, "split2": 4 * b + 3, "split5": 12 * b + 5}[shape]


def shapes_of(nperseg):
    """The shapes of one size, without those that coincide with an earlier one (B = 1, 2) or have no segment."""
    seen, out = set(), []
    for shape in SHAPES:
        n = shape_nseg(nperseg, shape)
        if n >= 1 and n not in seen:
            seen.add(n)
            out.append(shape)
    return out


def geometry(nperseg, shape):
    """(chunk_samples, samples, rows, nseg, nseg_last).  Three full chunks and a ragged last one of about two thirds of
    the segments plus three samples that belong to no segment; with one segment per chunk no shorter chunk holds one:
    eight chunks and a tail shorter than nperseg that gives no row.  "odd": nperseg/2 - 1 samples behind a chunk's last
    segment make chunk_samples odd, so chunks 1 and 3 start on an odd sample."""
    nseg, step = shape_nseg(nperseg, shape), nperseg // 2
    chunk = nperseg + step * (nseg - 1) + (step - 1 if shape == "odd" else 0)
    if nseg == 1:
        return chunk, 8 * chunk + nperseg - 5, 8, 1, 1
    last = max(1, (2 * nseg) // 3)
    last_len = nperseg + step * (last - 1) + 3
    assert nperseg <= last_len < chunk and segments_in(last_len, nperseg) == last < nseg
    return chunk, 3 * chunk + last_len, 4, nseg, last


# ---------------------------------------------------------------------------------------------------- captures
CLASSES = ("modest", "large_dc", "extreme")
DC_Q8 = {"modest": (600, -900), "large_dc": (12000, -12000)}          # 2.3 / -3.5 LSB and +-46.9 LSB
EXTREME_NAMES = ("constant 255", "constant 0", "constant 128/127", "nyquist full scale", "uniform bytes", "saturated tone",
                 "quiet then rail to rail", "one impulse")
MAX_SAMPLES = 160000                        # no capture of these tests is longer


@functools.lru_cache(maxsize=None)
def _stream(nperseg, klass, jammed):
    """MAX_SAMPLES + 1 samples of gpsjam.synth.generate with seed = nperseg and the class's DC, the jammer on from the
    first sample to the last or never: the generator is a function of the sample index, so a capture whose jammer
    switches on at sample j is the second stream before j and the first from j on."""
    dc_i, dc_q = DC_Q8[klass]
    spec = StreamSpec(seed=nperseg, jam_start=0, jam_end=(1 << 40) if jammed else 0, jam_sigma=30.0, dc_i_q8=dc_i, dc_q_q8=dc_q)
    raw = generate(spec, MAX_SAMPLES + 1)
    raw.setflags(write=False)
    return raw


def extreme_capture(name, samples):
    """extremes_inputs.capture(name) cut to length (repeated first where 2^15 samples are too few: 4096 points)."""
    import extremes_inputs as xi
    raw = xi.capture(name)
    return np.tile(raw, -(-2 * samples // raw.size))[:2 * samples]


@functools.lru_cache(maxsize=None)
def capture(nperseg, shape, klass, name=None):
    """The bytes of one case, ONE sample longer than its geometry (so that the same geometry fits from sample 1 on:
    the 2-byte-aligned base).  Read-only uint8."""
    chunk, samples, _, _, _ = geometry(nperseg, shape)
    assert samples + 1 <= MAX_SAMPLES + 1
    if klass == "extreme":
        raw = extreme_capture(name, samples + 1)
    else:
        on = chunk + chunk // 2                                          # the jammer switches on inside the second chunk
        raw = np.concatenate([_stream(nperseg, klass, False)[:2 * on], _stream(nperseg, klass, True)[2 * on:2 * (samples + 1)]])
    raw.setflags(write=False)
    return raw


VARIANTS = ("plain", "base+2", "unpack 128")   # the last two on the "odd" shape only


def variants_of(shape):
    return VARIANTS if shape == "odd" else VARIANTS[:1]


def case_bytes(nperseg, shape, klass, name=None, variant="plain"):
    """(bytes K2 is given, offset, scale) of one case: the geometry's samples from sample 0, or from sample 1."""
    _, samples, _, _, _ = geometry(nperseg, shape)
    raw = capture(nperseg, shape, klass, name)
    offset, scale = CONVENTIONS[1] if variant == "unpack 128" else CONVENTIONS[0]
    return (raw[2:2 * (samples + 1)] if variant == "base+2" else raw[:2 * samples]), offset, scale


@functools.lru_cache(maxsize=None)
def reference(nperseg, shape, klass, name=None, variant="plain", single=False):
    """The restatement's rows of one case, computed once and shared.  Read-only."""
    raw, offset, scale = case_bytes(nperseg, shape, klass, name, variant)
    rows = welch(raw, nperseg, geometry(nperseg, shape)[0], offset, scale, FS, single)
    assert rows.shape == (geometry(nperseg, shape)[2], nperseg)
    rows.setflags(write=False)
    return rows


def cases_of(nperseg, klass):
    """(shape, name) of every case of one size and class; the extreme captures run on the "odd" shape only."""
    if klass == "extreme":
        return [("odd", name) for name in EXTREME_NAMES]
    return [(shape, None) for shape in shapes_of(nperseg)]


def measure_e32(nperseg, klass):
    """Largest case error of the float32 restatement of K2's form against the float64 one over every case of a size
    and class, variants included."""
    return max(case_error(reference(nperseg, shape, klass, name, variant, True), reference(nperseg, shape, klass, name, variant))
               for shape, name in cases_of(nperseg, klass) for variant in variants_of(shape))


# ---------------------------------------------------------------------------------------------------- budgets
# E32[nperseg][class]: measure_e32 as tests/test_welch_host.py measures it (numpy 2.2 / scipy 1.15 pocketfft), the
# measured value beside each constant.  The host test holds every constant inside [measured, 2 x measured].
E32 = {
    16: {"modest": 3.19e-06, "large_dc": 2.48e-06, "extreme": 1.06e-05},     # measured 2.278e-06, 1.774e-06, 7.607e-06
    32: {"modest": 1.81e-06, "large_dc": 2.06e-06, "extreme": 1.06e-06},     # measured 1.296e-06, 1.474e-06, 7.582e-07
    64: {"modest": 1.61e-06, "large_dc": 2.38e-06, "extreme": 8.03e-07},     # measured 1.151e-06, 1.697e-06, 5.736e-07
    128: {"modest": 1.23e-06, "large_dc": 4.09e-06, "extreme": 6.33e-07},    # measured 8.797e-07, 2.918e-06, 4.519e-07
    256: {"modest": 9.00e-07, "large_dc": 4.16e-06, "extreme": 5.53e-07},    # measured 6.427e-07, 2.973e-06, 3.951e-07
    512: {"modest": 8.32e-07, "large_dc": 1.35e-05, "extreme": 4.89e-07},    # measured 5.940e-07, 9.608e-06, 3.490e-07
    1024: {"modest": 8.72e-07, "large_dc": 1.32e-05, "extreme": 7.33e-07},   # measured 6.230e-07, 9.429e-06, 5.239e-07
    2048: {"modest": 1.22e-06, "large_dc": 1.44e-05, "extreme": 9.50e-07},   # measured 8.729e-07, 1.029e-05, 6.789e-07
    4096: {"modest": 1.57e-06, "large_dc": 1.99e-05, "extreme": 1.77e-06},   # measured 1.120e-06, 1.425e-05, 1.264e-06
}
FACTOR = 4.0                                # K2's transform is a radix-16 Stockham with table twiddles and its sums run
                                            # in another order than pocketfft's: two correct float32 transforms differ
                                            # by a small factor (the oracle and this form: within 1.5 x of each other)


def tolerance(nperseg, klass):
    """What a K2 row may be off the float64 restatement, in the measure of ``errors``."""
    return FACTOR * E32[nperseg][klass]


# The float32 oracle (oracle.gpsjam_oracle.widmo_waterfall) against the float64 restatement, in the same measure, on the
# inputs of test_gpu_parity.test_k2_all_sizes_vs_oracle (seed = nperseg, chunk 65536, three rows); and the committed
# golden rows (tests/golden/g2_welch.npz, made by that oracle) on the golden capture.  Measured beside each.
ORACLE_E32 = {16: 6.62e-06, 32: 3.85e-06, 64: 3.58e-06, 128: 2.60e-06, 256: 2.13e-06, 512: 1.31e-06, 1024: 1.22e-06, 2048: 8.21e-07,
              4096: 8.95e-07}
# measured    16: 4.727e-06, 32: 2.747e-06, 64: 2.559e-06, 128: 1.860e-06, 256: 1.522e-06, 512: 9.333e-07, 1024: 8.746e-07,
#             2048: 5.864e-07, 4096: 6.391e-07.  Per bin (|got - truth| / truth, the measure of the old tests) the oracle is
#             5.8e-06 off at 4096 points and the float32 form 9.7e-06: the un-removed DC's rounding noise in the small bins.
GOLDEN_E32 = {1024: 4.79e-06, 4096: 2.89e-06}   # measured 3.421e-06, 2.065e-06
