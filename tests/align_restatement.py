"""The pair alignment restated on integers (gj_align_dev of include/gpsjam.h), and the inputs its CPU and GPU tests
share.  ``align`` is the definition in vectorised numpy int64 -- tests/test_align_host.py holds it to a per-sample loop of
Python ints -- and the yardstick of tests/align/test_round6_gpu.py: every byte and every record is equal, bit for bit.

Nothing here reads gpsjam/align.py: the tables of the parity cases are random, and the end-to-end pair is made of tones
evaluated analytically at both receivers' sample times."""
import numpy as np

PHASES, TAPS, ROT_LEN, BLOCK = 256, 16, 1024, 4096
MAX_DRIFT, MAX_SAMPLES = 1 << 24, 1 << 28
ONE = 1 << 32
DTYPE = np.dtype([("power_out", np.uint64), ("n_clipped", np.int32), ("n_edge", np.int32)])
SIZES = (1, 15, 16, 17, 4095, 4096, 4097, 3 * 4096 + 5)


def blocks(n_out: int) -> int:
    return -(-int(n_out) // BLOCK)


def align(raw, pos0, pos_step, rot_phase, rot_step, taps, rot, n_out):
    """(uint8[2 n_out], DTYPE[blocks(n_out)]): the header's definition, every value an exact int64."""
    raw = np.asarray(raw, np.uint8)
    n_src = raw.size // 2
    u = 2 * raw[:2 * n_src].astype(np.int64).reshape(n_src, 2) - 255
    taps = np.asarray(taps, np.int64).reshape(PHASES, TAPS)
    rot = np.asarray(rot, np.int64).reshape(ROT_LEN)
    n = np.arange(int(n_out), dtype=np.int64)
    pos = int(pos0) + n * int(pos_step) + (1 << 23)
    k, p = pos >> 32, (pos & 0xFFFFFFFF) >> 24
    idx = k[:, None] - 7 + np.arange(TAPS, dtype=np.int64)[None, :]
    inside = (idx >= 0) & (idx < n_src)
    win = np.where(inside[:, :, None], u[np.clip(idx, 0, max(n_src - 1, 0))] if n_src else 0, 0)     # [n][16][2]
    y = (taps[p][:, :, None] * win).sum(axis=1)
    assert np.abs(y).max(initial=0) < 2 ** 31
    theta = (int(rot_phase) + n * int(rot_step)) & 0xFFFFFFFF
    i = ((theta + (1 << 21)) >> 22) & 1023
    c, s = rot[i], rot[(i - 256) & 1023]
    z = np.stack([y[:, 0] * c - y[:, 1] * s, y[:, 0] * s + y[:, 1] * c], axis=1)
    want = (z >> 29) + 128                                   # >> on int64 is the floor
    out = np.clip(want, 0, 255)
    rec = np.zeros(blocks(n_out), DTYPE)
    block = n // BLOCK
    np.add.at(rec["power_out"], block, ((2 * out - 255) ** 2).sum(axis=1).astype(np.uint64))
    np.add.at(rec["n_clipped"], block, (out != want).sum(axis=1).astype(np.int32))
    np.add.at(rec["n_edge"], block, (~inside.all(axis=1)).astype(np.int32))
    return out.astype(np.uint8).reshape(-1), rec


# ------------------------------------------------------------------------------------------------ parity inputs
PARITY_SAMPLES = 3 * 4096 + 300       # the source: a little longer than the largest output


def parity_capture(kind="random"):
    """uint8[2 * PARITY_SAMPLES]: random bytes with the four corners of the byte range up front; all 0; all 255."""
    if kind == "zeros":
        return np.zeros(2 * PARITY_SAMPLES, np.uint8)
    if kind == "full":
        return np.full(2 * PARITY_SAMPLES, 255, np.uint8)
    raw = np.random.default_rng(2718).integers(0, 256, 2 * PARITY_SAMPLES).astype(np.uint8)
    raw[:8] = (0, 0, 0, 255, 255, 0, 255, 255)
    return raw


def tables(kind):
    """(taps int16[256][16], rot int16[1024]).  "wide": random over all of int16, so |y| and |z| come near their bounds
    (nearly every byte clamps); "mid": random at a scale that leaves the bytes spread over 0 .. 255; "worst": every
    entry -32768, the bound itself on an all-0 or all-255 capture; "delta": row p the delta at tap 7 whatever p, and a
    true turn -- whole-sample shifts and the identity."""
    rng = np.random.default_rng({"wide": 11, "mid": 12, "worst": 13, "delta": 14}[kind])
    if kind == "wide":
        t, r = rng.integers(-32768, 32768, (PHASES, TAPS)), rng.integers(-32768, 32768, ROT_LEN)
        t[0, :4], r[:4] = (-32768, 32767, -32768, 32767), (-32768, 32767, 32767, -32768)
    elif kind == "mid":
        t, r = rng.integers(-3000, 3001, (PHASES, TAPS)), rng.integers(-16384, 16385, ROT_LEN)
    elif kind == "worst":
        t, r = np.full((PHASES, TAPS), -32768), np.full(ROT_LEN, -32768)
    else:
        t = np.zeros((PHASES, TAPS), np.int64)
        t[:, 7] = 16384
        r = np.rint(16384 * np.cos(2 * np.pi * np.arange(ROT_LEN) / ROT_LEN))
    return t.astype(np.int16), r.astype(np.int16)


# (pos0, pos_step, rot_phase, rot_step): the edges of the definition
CASES = {
    "identity time base": (0, ONE, 0, 0),
    "negative start": (-(5 << 32) - 0x4CCCCCCC, ONE, 1, 1),
    "start past the source's end": ((PARITY_SAMPLES + 9) << 32, ONE, 0, 0),
    "ends past the source's end": ((PARITY_SAMPLES - 20) << 32 | 0x80000000, ONE + 12345, 0xFFFFFFFF, 0xFFFFFFFF),
    "rounding carries into k": ((2 << 32) | 0xFF800000, ONE, 0x12345678, 0x00F00000),
    "fraction 2^23 - 1": ((9 << 32) | 0x007FFFFF, ONE, 0, 1),
    "fraction 2^23": ((9 << 32) | 0x00800000, ONE, 1, 0xFFFFFFFF),
    "slowest step": (3 << 32, ONE - MAX_DRIFT, 0xFFFFFFFF, 0x9E3779B9),
    "fastest step": (-(7 << 32), ONE + MAX_DRIFT, 0x80000000, 0x7FFFFFFF),
    "far before the source": (-(1 << 60) + 1, ONE + MAX_DRIFT, 5, 7),
    "far behind the source": ((1 << 60) - 1, ONE - MAX_DRIFT, 5, 7),
}


# ------------------------------------------------------------------------------------------------ the end-to-end pair
FS = 2.048e6
E2E_SAMPLES = 1 << 16
E2E_NFFT, E2E_FRAMES = 256, 256
E2E_LAG, E2E_DRIFT, E2E_OFFSET_HZ = 3.25, 40e-6, 300.0
E2E_TONES, E2E_BAND = 300, (0.05, 0.25)           # the jammer: tones spread over this band, cycles per sample
E2E_JAM_LSB, E2E_NOISE_LSB = 12.0, 6.25           # rms per component
# Twice what tests/test_align_host.py measures with gpsjam.align on restated integers (it prints every figure: 0.006 and
# 0.012 sample, 0.11 and 0.07 ppm, 0.12 and 0.54 Hz, without and with rf_hz); the GPU test holds the device to the same
# bounds.  The median MSC of the aligned pair is measured 0.005 under the one-clock pair's.
E2E_TOL_LAG, E2E_TOL_DRIFT, E2E_TOL_OFFSET_HZ = 0.025, 0.25e-6, 1.1
E2E_TOL_MSC = 0.02


def _tones(t, freqs, phases, amp):
    """Sum of complex tones at the (fractional) sample times t, evaluated in chunks."""
    out = np.zeros(t.size, np.complex128)
    for lo in range(0, freqs.size, 50):
        out += np.exp(2j * np.pi * (np.outer(t, freqs[lo:lo + 50]) + phases[lo:lo + 50][None, :])).sum(axis=1)
    return amp * out


def _bytes(z):
    iq = np.empty(2 * z.size)
    iq[0::2], iq[1::2] = z.real, z.imag
    return np.clip(np.floor(iq + 127.5 + 0.5), 0, 255).astype(np.uint8)       # u = 2 byte - 255 = 2 * round(x)


_pair = {}


def e2e_pair():
    """(raw_a, raw_b, raw_b_one_clock): a band of 300 tones, 12 LSB rms per component, over 6.25 LSB of noise of each
    receiver's own.  Receiver b samples the source at the instants (m - lag) / (1 + drift) of a's clock and sees it 300
    Hz higher; ``raw_b_one_clock`` is b on a's clock and tuner, with the same noise.  Every tone is evaluated at the
    sample times themselves: nothing is interpolated."""
    if not _pair:
        rng = np.random.default_rng(1618)
        n = E2E_SAMPLES
        freqs = rng.uniform(E2E_BAND[0], E2E_BAND[1], E2E_TONES)
        phases = rng.uniform(0, 1, E2E_TONES)
        amp = E2E_JAM_LSB * np.sqrt(2.0 / E2E_TONES)
        noise = [E2E_NOISE_LSB * (rng.normal(size=n) + 1j * rng.normal(size=n)) for _ in range(2)]
        m = np.arange(n, dtype=np.float64)
        t_b = (m - E2E_LAG) / (1.0 + E2E_DRIFT)
        gain_b = np.exp(1j * 0.7)                              # another cable, another phase
        a = _tones(m, freqs, phases, amp) + noise[0]
        b = gain_b * _tones(t_b, freqs, phases, amp) * np.exp(2j * np.pi * E2E_OFFSET_HZ * m / FS) + noise[1]
        same = gain_b * _tones(m, freqs, phases, amp) + noise[1]
        _pair["v"] = tuple(_bytes(z) for z in (a, b, same))
        for raw in _pair["v"]:
            raw.flags.writeable = False
    return _pair["v"]


def band_bins(nfft=E2E_NFFT):
    """FFT-order bins that lie wholly inside the jammer's band."""
    k = np.arange(nfft)
    return k[(k >= np.ceil(E2E_BAND[0] * nfft) + 1) & (k <= np.floor(E2E_BAND[1] * nfft) - 1)]
