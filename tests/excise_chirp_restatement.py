"""The chirp-domain excisor (gj_excise_chirp_dev, include/gpsjam.h) and the rate picker (gj_chirp_rates_dev) restated in
numpy, and the inputs and constants of their tests.  Not a test module: tests/test_excise_chirp_host.py and
tests/excise_chirp/test_round6_gpu.py import it.  Built on tests/excise_restatement.py (the excisor) and
tests/chirp_restatement.py (the de-chirp, its complex64 factoring, the saw-tooth).

    c_f[n] = exp(-i pi ((q_f n^2) mod 2 N^2) / N^2)
    X_f    = fft(w * x[s_f : s_f + N] * c_f),  s_f = first_sample + f N/2
    P_f[k] = |X_f[k]|^2 * scale^2
    y_f    = conj(c_f) * ifft(X_f where P_f <= thr else 0)
    y[t]   = y_{f-1}[t - s_{f-1}] + y_f[t - s_f];  u = clip(rint(float32(y + offset)), 0, 255) on samples [N/2, F N/2)

    rate[f] = rate_first + rate_index_f * rate_step  if total_f > 0 and peak_f >= float32(min_concentration * total_f) else 0
"""
import functools

import numpy as np
import scipy.fft

import chirp_restatement as cr
import excise_restatement as er
import ridge_restatement as rr

FS = er.FS
NFFT = (16, 32, 64, 256, 1024, 2048, 4096)
CONVENTIONS = er.CONVENTIONS
NEAR_TIE = er.NEAR_TIE                      # 1e-4 relative: P against its threshold, peak / total against MIN_CONCENTRATION
RTOL = 1e-5                                 # the project's figure for a K2 value summed in another order
PARITY_SAMPLES = er.PARITY_SAMPLES          # 2^15
PARITY_FIRST = 1                            # odd on purpose
PARITY_SIGMA = er.PARITY_SIGMA              # 6.25 LSB
PARITY_TONE_HZ, PARITY_TONE_AMP = er.PARITY_TONE_HZ, er.PARITY_TONE_AMP
PARITY_SWEEP_AMP = 40.0
PARITY_SWEEP_BW_HZ = 1.0e6
# the saw-tooth's rate in units of (fs / nfft)^2 AT THAT nfft: an integer, so that the matching de-chirp makes a line
PARITY_Q = {16: 2, 32: 2, 64: 3, 256: 5, 1024: 40, 2048: 60, 4096: 100}
# one seed per size, chosen so that the restatement alone keeps every P_f[k] NEAR_TIE away from its threshold and every
# frame's peak / total NEAR_TIE away from MIN_CONCENTRATION (tests/test_excise_chirp_host.py asserts both)
PARITY_SEED = {16: 8, 32: 14, 64: 1, 256: 1, 1024: 1, 2048: 1, 4096: 1}
MIN_CONCENTRATION = 0.1
RATE_SPAN = 8

# Largest |y_complex64 - y_float64| over the parity inputs, every size and both unpack conventions, measured on the CPU
# with scipy.fft on complex64 input and the de-chirp factors built as the kernel builds them (cr.dechirp_factors32, the
# two parts multiplied in complex64): a product of up to ten unit-modulus floats at BOTH ends of the frame, which the
# plain excisor's E32 does not contain.  A transform with other radices and twiddles than pocketfft errs against float64
# by a like amount; the factor 8 covers the sum of both and the final + offset (the argument of excise_restatement.py).
E32_CHIRP_MEASURED = 3.4406242278350874e-05     # 1.4e-5 at 16 points .. 3.4e-5 at 2048 points
E32_CHIRP = 3.45e-5
TIE_BAND = 8 * E32_CHIRP
# The share of excised components whose float64 value lies inside TIE_BAND of a rounding tie, at most, over the parity
# inputs: the values are spread evenly over a unit interval, so the share is 2 TIE_BAND, and twice that is the cap
TIE_SHARE_CAP = 4 * TIE_BAND


def effective_rate(q, nfft):
    """q modulo 2 N^2, the period of the phase."""
    return int(q) % (2 * nfft * nfft)


@functools.lru_cache(maxsize=None)
def factors(q, nfft, single=False):
    """c_q[n]: float64 from the integer phase; single: complex64 as the kernel builds it, (e8 d^(s-8)) * k_s."""
    if not single:
        c = cr.dechirp(effective_rate(q, nfft), nfft)
    else:
        e, k = cr.dechirp_factors32(int(q), nfft)
        c = e * k
        assert c.dtype == np.complex64
    c.setflags(write=False)
    return c


def excise_chirp(raw, thr, rates, nfft, first_sample=0, n_samples=None, offset=127.5, scale=1.0 / 127.5, single=False):
    """The definition on the bytes `raw`; `rates`: one integer per frame.  single=True: window, de-chirp, transforms and
    re-chirp in complex64, everything else alike.  Returns an er.Excised."""
    raw = np.asarray(raw, np.uint8)
    if n_samples is None:
        n_samples = raw.size // 2 - first_sample
    h = nfft // 2
    nf = er.frames_loop(n_samples, nfft)
    rates = [int(q) for q in np.asarray(rates).reshape(-1)]
    assert nf >= 1 and first_sample + n_samples <= raw.size // 2 and len(rates) == nf
    src = raw[2 * first_sample:2 * (first_sample + n_samples)]
    x = er.unpack_lsb(src, offset)
    idx = (h * np.arange(nf))[:, None] + np.arange(nfft)[None, :]
    seg = x[idx] * er.hann(nfft)[None, :]
    c = np.stack([factors(q, nfft, single) for q in rates])
    if single:
        seg = seg.astype(np.complex64)
    X = scipy.fft.fft(seg * c, axis=1)
    assert X.dtype == (np.complex64 if single else np.complex128)
    P, _, sums, value, out = er.finish(X, src, thr, nfft, offset, scale, rechirp=np.conj(c))
    rec = np.zeros(nf, er.RECORD64)
    rec["total"], rec["removed"], rec["n_excised"] = sums
    return er.Excised(out, rec, value, P, nfft)


def chirp_rates(records, rate_first, rate_step, min_concentration):
    """gj_chirp_rates_dev on records with `total`, `peak` and `rate_index`: the product in float32, the sum modulo 2^32."""
    total, peak = records["total"].astype(np.float32), records["peak"].astype(np.float32)
    need = np.float32(min_concentration) * total                 # float32 * float32: one rounding
    assert need.dtype == np.float32
    with np.errstate(invalid="ignore"):
        on = (total > 0) & (peak >= need)
    q = (int(rate_first) + records["rate_index"].astype(np.int64) * int(rate_step)) & 0xFFFFFFFF
    return np.where(on, q, 0).astype(np.uint32).view(np.int32)


def concentration_margin(records, min_concentration=MIN_CONCENTRATION):
    """Smallest |peak / (min_concentration total) - 1| over the frames with power (inf without one)."""
    total, peak = records["total"].astype(np.float64), records["peak"].astype(np.float64)
    ok = total > 0
    return float(np.min(np.abs(peak[ok] / (min_concentration * total[ok]) - 1.0))) if ok.any() else np.inf


# ---------------------------------------------------------------------------------------------------- inputs
def parity_sweep_hz_per_s(nfft):
    return PARITY_Q[nfft] * (FS / nfft) ** 2


@functools.lru_cache(maxsize=None)
def parity_capture(nfft):
    """2^15 samples: noise of sigma 6.25 LSB, the parity tone and a saw-tooth of PARITY_Q[nfft] rate units over 1 MHz
    (at 16 and 32 points a period is shorter than a frame or two, so few frames hold a clean sweep).  Read-only uint8."""
    rng = np.random.default_rng(PARITY_SEED[nfft])
    n = PARITY_SAMPLES
    z = rr._noise(rng, n, PARITY_SIGMA).astype(np.complex128) + rr.tone(n, PARITY_TONE_HZ, PARITY_TONE_AMP)
    z = z + cr.sawtooth(n, PARITY_SWEEP_AMP, parity_sweep_hz_per_s(nfft), PARITY_SWEEP_BW_HZ)
    raw = rr.quantise(z)
    raw.setflags(write=False)
    return raw


def rate_cycle(nfft):
    """0, the matching rate, its negative, +-1, +-N^2/2 and 2 N^2 + 3 (which is the rate 3): consecutive frames differ."""
    q, n2 = PARITY_Q[nfft], nfft * nfft
    return (0, q, -q, 1, -1, n2 // 2, -(n2 // 2), 2 * n2 + 3)


def parity_rates(nfft, n_frames=None):
    """The cycling rate vector of the parity input (int32), one rate per frame."""
    if n_frames is None:
        n_frames = er.frames_loop(PARITY_SAMPLES - PARITY_FIRST, nfft)
    cyc = rate_cycle(nfft)
    return np.array([cyc[f % len(cyc)] for f in range(n_frames)], np.int32)


def parity_threshold(nfft, scale=1.0 / 127.5):
    return er.parity_threshold(nfft, scale)


@functools.lru_cache(maxsize=None)
def parity_reference(nfft, offset=127.5, scale=1.0 / 127.5, single=False):
    """The restatement of parity_capture(nfft) from PARITY_FIRST to the end at parity_rates(nfft), computed once."""
    return excise_chirp(parity_capture(nfft), parity_threshold(nfft, scale), parity_rates(nfft), nfft, PARITY_FIRST, None,
                        offset, scale, single)


def parity_scan_rates(nfft):
    """The grid the rate picker's tests scan the parity input with: five rates around the matching one."""
    return (PARITY_Q[nfft] - 2, 1, 5)


@functools.lru_cache(maxsize=None)
def parity_scan(nfft):
    """The restated chirp-rate search of parity_capture(nfft) on the excisor's frames (hop N/2 from PARITY_FIRST)."""
    return cr.chirp_scan(parity_capture(nfft), nfft, nfft // 2, parity_scan_rates(nfft), PARITY_FIRST,
                         er.frames_loop(PARITY_SAMPLES - PARITY_FIRST, nfft))


# complete removal: a noiseless chirp of an even integer rate from sample 0, whose band-edge wrap is seamless in discrete
# time, so EVERY frame holds the rate REMOVAL_Q and starts on a bin centre (bin q f / 2 of frame f)
REMOVAL_NFFT = (64, 1024)
REMOVAL_Q = {64: 6, 1024: 200}
REMOVAL_AMP = 50.0
REMOVAL_FRAMES = 12


@functools.lru_cache(maxsize=None)
def removal_capture(nfft):
    n = (REMOVAL_FRAMES + 1) * (nfft // 2)
    t = np.arange(n, dtype=np.float64)
    z = REMOVAL_AMP * np.exp(1j * np.pi * REMOVAL_Q[nfft] * (t / nfft) ** 2)
    # rounded to the nearest level of the 127.5 convention (rr.quantise truncates toward zero, and the error of that
    # follows the signal's sign: harmonics of the chirp, which no single de-chirp collects)
    raw = np.empty(2 * n, np.uint8)
    raw[0::2], raw[1::2] = np.floor(z.real + 128.0), np.floor(z.imag + 128.0)
    raw.setflags(write=False)
    return raw


def removal_threshold(nfft, scale=1.0 / 127.5):
    """Between the de-chirped line and zero: a Hann-windowed tone of amplitude A on a bin centre is A N / 2 there and
    A N / 4 on each neighbour, nothing elsewhere; (A N / 16)^2 lies 12 dB under the neighbours and far above what the
    quantiser leaves (0.3 LSB rms)."""
    return np.full(nfft, (REMOVAL_AMP * nfft / 16.0 * scale) ** 2, np.float32)


# end to end: er.E2E_SATS in sigma = 10 noise, quiet lead-in, then a 60-LSB saw-tooth of about 4 GHz/s over 1.6 MHz
E2E_NFFT = er.E2E_NFFT                       # 1024: one rate unit is 4 MHz/s
E2E_Q = 1002                                 # rate units at 1024 points
E2E_SWEEP = E2E_Q * (FS / E2E_NFFT) ** 2     # 4.008 GHz/s = 62.625 units at 256 points: an eighth off a half-integer
E2E_BW_HZ = 1.6e6
E2E_AMP = er.E2E_TONE_AMP                    # 60 LSB
E2E_MAX_SWEEP = 4.2e9                        # characterise_swept then searches +-66 units at 256 points
E2E_CHARACTERISE_NFFT = 256
# C/N0 of the oracle's acquisition (orc.acq_search) on the CPU restatement of the whole chain, dB per satellite of
# er.E2E_SATS (tests/test_excise_chirp_host.py re-measures and prints them):
E2E_CPU_FREE = (49.58, 48.86, 47.35)         # jammer-free, acquired at the first step
E2E_CPU_SWEPT = (48.90, 47.86, 46.69)        # chirp domain (rates 1000 .. 1004 from the grid 1000 .. 1016), acquired at the first step
E2E_CPU_PLAIN = (35.52, 34.75, 34.71)        # er.excise, same capture and threshold: none acquired (the jammed capture: 35.7 36.9 36.8)
E2E_CPU_LOSS_DB = 1.01                       # largest loss of the chirp-domain result against jammer-free (0.68 1.01 0.66)
E2E_CPU_GAP_DB = 11.97                       # smallest advantage of the chirp-domain result over er.excise (13.38 13.10 11.97)
E2E_CN0_TOL_DB = 2.0 * E2E_CPU_LOSS_DB       # the rule: twice the loss the CPU restatement measured
E2E_MIN_GAP_DB = 0.5 * E2E_CPU_GAP_DB        # mitigate.clean must be worse by at least half the gap the CPU measured


@functools.lru_cache(maxsize=None)
def e2e_capture(jammed=True):
    """er.e2e_capture's signals and noise (same seed), with the saw-tooth from sample E2E_LEAD on."""
    from gpsjam import gnss
    n = er.E2E_LEAD + er.E2E_AFTER
    rng = np.random.default_rng(4)
    k = np.arange(n)
    z = rng.normal(0, er.E2E_SIGMA, n) + 1j * rng.normal(0, er.E2E_SIGMA, n)
    for prn, dop, delay, amp in er.E2E_SATS:
        chip = ((k - delay) * 1.023e6 / FS) % 1023
        z += amp * gnss.ca_code(prn)[chip.astype(np.int64)] * np.exp(-2j * np.pi * dop * (k / FS))
    if jammed:
        z[er.E2E_LEAD:] += cr.sawtooth(er.E2E_AFTER, E2E_AMP, E2E_SWEEP, E2E_BW_HZ)
    iq = np.empty(2 * n, np.float64)
    iq[0::2], iq[1::2] = z.real, z.imag
    raw = (np.clip(np.round(iq), -128, 127) + 128).astype(np.uint8)
    raw.setflags(write=False)
    return raw


def e2e_flat_threshold(nfft=E2E_NFFT, scale=1.0 / 127.5):
    """What clean_swept applies: flat, the nominal floor of sigma = 10 noise times 12 dB (the measured median of the
    quiet part's floor is within a few percent of it)."""
    return np.full(nfft, er.noise_floor(nfft, er.E2E_SIGMA, scale) * 10.0 ** (er.E2E_RISE_DB / 10.0), np.float32)


def compare(got, rec, want, what):
    """GPU bytes and records against an er.Excised."""
    assert rec.size == want.records.size and got.size == want.out.size, what
    np.testing.assert_array_equal(rec["n_excised"], want.records["n_excised"], err_msg=str(what))
    assert not rec["reserved"].any()
    tot = want.records["total"]
    for key in ("total", "removed"):
        err = float(np.max(np.abs(rec[key] - want.records[key]) / tot))
        print(f"{what}: {key} within {err:.2e}")
        assert err <= RTOL, (what, key, err)
    assert np.array_equal(got[:want.lo], want.out[:want.lo]) and np.array_equal(got[want.hi:], want.out[want.hi:]), (what, "edges")
    body, ref = got[want.lo:want.hi].astype(np.int16), want.out[want.lo:want.hi].astype(np.int16)
    clear = er.tie_distance(want.value) > TIE_BAND
    diff = np.abs(body - ref)
    share = float(np.mean(~clear))
    print(f"{what}: {int(np.sum(diff != 0))} of {diff.size} bytes differ, {int(np.sum(~clear))} lie in the tie band ({share:.2e})")
    assert share <= TIE_SHARE_CAP, (what, share)
    assert not diff[clear].any(), (what, int(np.sum(diff[clear] != 0)), "bytes differ outside the tie band")
    assert diff.max(initial=0) <= 1, (what, int(diff.max()))
