"""CPU side of the counterfeit-signal subtraction and what is built on it (gj_subtract_dev, gj_subtract_blocks,
Device.subtract, postcorr.amplitudes, spoof.remove, mitigate.clean_spoofed and its command line): the interface, the
integer restatement the GPU tests compare with (tests/subtract_restatement.py) checked against a per-sample Python-int
loop and against the definition's own consequences, the Python layers on a host double of the library, and the end-to-end
figures on restated integers, which set the tolerances of the GPU test.  No GPU call is made.

The float chain is not restated anywhere: gpsjam.postcorr, gpsjam.spoof and gpsjam.mitigate themselves run here, on
restated integers."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import corr_restatement as cr
import gpsjam
import host_lib
import peaks_restatement as pr
import subtract_restatement as sr
from gpsjam import _ffi, gnss, mitigate, postcorr, spoof
from oracle import gpsjam_oracle as orc

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gpsjam.h")
NSAMP, NSAMPCHIP = 2048, 2


# ------------------------------------------------------------------------------------------------ interface
def test_symbols_bindings_and_python_interface():
    lib = _ffi.load()
    assert len(_ffi.SIGNATURES["gj_subtract_dev"][1]) == 15 and len(_ffi.SIGNATURES["gj_subtract_blocks"][1]) == 1
    for name in ("gj_subtract_dev", "gj_subtract_blocks"):
        assert callable(getattr(lib, name))
    assert _ffi.GJ_VERSION == 150 == lib.gj_version()
    assert (_ffi.GJ_SUB_BLOCK, _ffi.GJ_SUB_FRAC, _ffi.GJ_SUB_MAX_AMP, _ffi.GJ_SUB_DITHER) == (sr.SUB_BLOCK, sr.FRAC, sr.MAX_AMP, sr.DITHER) == (4096, 16, 2 ** 19, 1)
    assert (gpsjam.SUB_BLOCK, gpsjam.SUB_FRAC, gpsjam.SUB_MAX_AMP) == (4096, 16, 2 ** 19) and postcorr.SUB_FRAC == 16
    assert C.sizeof(_ffi.SubtractBlock) == 24 == gpsjam.SUB_DTYPE.itemsize == sr.DTYPE.itemsize
    assert [f[0] for f in _ffi.SubtractBlock._fields_] == list(gpsjam.SUB_DTYPE.names) == list(sr.DTYPE.names) == ["total", "removed", "n_clipped", "reserved"]
    for name in ("subtract", "subtract_dev"):
        assert callable(getattr(gpsjam.Device, name))
    for name in ("SUB_BLOCK", "SUB_DTYPE", "subtract_blocks"):
        assert name in gpsjam.__all__
    for n in (0, 1, 4095, 4096, 4097, 3 * 4096 + 5, 2 ** 40 + 1):
        assert gpsjam.subtract_blocks(n) == -(-n // 4096) == sr.blocks(n), n
    assert gpsjam.subtract_blocks(-1) == 0
    assert callable(postcorr.amplitudes) and callable(spoof.remove) and callable(mitigate.clean_spoofed)
    assert spoof.Removal._fields == ("prn", "code_index", "doppler_hz", "cn0_before", "cn0_after", "suppression_db")


def test_the_headers_constants_and_the_bound():
    text = open(HEADER).read()
    assert int(re.search(r"#define GJ_SUB_BLOCK (\d+)", text).group(1)) == 4096
    assert int(re.search(r"#define GJ_SUB_FRAC (\d+)", text).group(1)) == 16
    assert re.search(r"#define GJ_SUB_MAX_AMP \(1 << 19\)", text) and re.search(r"#define GJ_SUB_DITHER 1\b", text)
    assert sr.R_BOUND == 64 * 2 ** 19 * 46 == 1543503872 and sr.R_BOUND + 65535 < 2 ** 31
    gains = [c * c + s * s for c, s in zip(cr.COS, cr.SIN)]
    assert sum(gains) / 16 == postcorr.MIXER_GAIN == 1042.5 and min(gains) == 1024 and max(gains) == 1058
    assert max(abs(g / 1042.5 - 1.0) for g in gains) < 0.018


# ------------------------------------------------------------------------------------------------ the restatement
def small_input(seed, n_samples=700):
    rng = np.random.default_rng(seed)
    raw = rng.integers(0, 256, 2 * n_samples).astype(np.uint8)
    raw[:8] = (0, 0, 255, 255, 0, 255, 255, 0)
    return raw


@pytest.mark.parametrize("B", [16, 48])
def test_restatement_equals_the_python_int_loop(B):
    raw, codes, channels = small_input(B), cr.parity_codes(), cr.parity_channels(8)
    for first, n in ((0, 1), (3, 15), (1, B - 1), (0, B), (5, B + 1), (2, 6 * B + 5)):
        for bound, flags, seed in ((2 ** 14, 0, 0), (2 ** 14, 1, 0), (2 ** 19, 1, 0xDEADBEEF), (2 ** 22, 0, 5)):
            amps = sr.random_amps(8, cr.blocks(n, B), bound, seed=n)
            got, rec = sr.subtract(raw, first, n, B, codes, channels, amps, flags, seed)
            want, wrec = sr.brute(raw, first, n, B, codes, channels, amps, flags, seed)
            assert got.tolist() == want and [tuple(int(v) for v in r)[:3] for r in rec] == wrec, (first, n, bound, flags)
            assert not rec["reserved"].any()


def test_the_dither_is_the_hash_of_the_absolute_index_and_its_key_is_64_bits_wide():
    """k = 2 sample + comp passes 2^32 at sample 2^31: the upper word enters the key from there on."""
    for first in (0, 7, 2 ** 31 - 3, 2 ** 32 - 2, 2 ** 33 + 5, 2 ** 62):
        for seed in (0, 1, 0xFFFFFFFF):
            got = sr.dither(first, 6, seed)
            want = [[sr.dither_one(first + t, comp, seed) for comp in (0, 1)] for t in range(6)]
            assert got.tolist() == want and 0 <= got.min() and got.max() < 65536, (first, seed)
    lo, hi = sr.dither(5, 4, 9), sr.dither(2 ** 31 + 5, 4, 9)
    assert not np.array_equal(lo, hi), "the same low word, another upper word: other values"
    text = open(HEADER).read()
    for const in ("0x9e3779b9", "0x7feb352d", "0x846ca68b"):
        assert const in text


def test_zero_amplitudes_are_the_identity_with_and_without_dither():
    raw, codes, channels = cr.parity_capture(), cr.parity_codes(), cr.parity_channels(5)
    n = 2 * 4096 + 77
    for flags, seed in ((0, 0), (1, 0), (1, 12345)):
        got, rec = sr.subtract(raw, 3, n, 256, codes, channels, np.zeros((5, cr.blocks(n, 256), 2), np.int32), flags, seed)
        assert got.tobytes() == raw[6:6 + 2 * n].tobytes() and not rec["removed"].any() and not rec["n_clipped"].any()
        assert int(rec["total"].sum()) == int(((raw[6:6 + 2 * n].astype(np.int64) - 128) ** 2).sum())


def constant_replica_input(aI):
    """One channel that gives R = (32 aI, 0) at every sample: an all-ones code row, a still carrier at table index 0."""
    return np.ones((1, 1023), np.int16), [(0, 0, 0, 0, 0, 0)], aI


@pytest.mark.parametrize("R", [-32736, -9984, -32, 32, 7008, 32736])
def test_the_dither_is_unbiased_where_rounding_subtracts_nothing(R):
    """A constant |R| < 32768 on a constant capture over 2^16 samples: without the dither q is 0 everywhere (the case
    it exists for); with it the mean of q is R / 65536 within 4 standard errors of a uniform d, 4 / sqrt(12 * 2^16).
    The hash is fixed, so the result is too."""
    n = 2 ** 16
    ones, channels, aI = constant_replica_input(R // 32)
    assert aI * 32 == R
    raw = np.full(2 * n, 128, np.uint8)
    amps = np.tile(np.array([aI, 0], np.int32), (1, cr.blocks(n, 4096), 1))
    plain, _ = sr.subtract(raw, 0, n, 4096, ones, channels, amps, 0, 0)
    assert np.all(plain == 128), "rounding to nearest subtracts nothing"
    for seed in (0, 77):
        got, rec = sr.subtract(raw, 0, n, 4096, ones, channels, amps, sr.DITHER, seed)
        q_i, q_q = 128 - got[0::2].astype(np.int64), 128 - got[1::2].astype(np.int64)
        assert set(np.unique(q_i)) <= {0, 1 if R > 0 else -1}
        bound = 4.0 / math.sqrt(12.0 * n)
        print(f"R {R} seed {seed}: mean q {q_i.mean():+.6f}, R / 65536 {R / 65536.0:+.6f}, bound {bound:.6f}")
        assert abs(q_i.mean() - R / 65536.0) <= bound
        assert abs(q_q.mean()) <= bound and not rec["n_clipped"].any(), "R_Q = 0: the Q bytes move by the dither of 0 alone, which is none"


def test_a_block_aligned_sub_range_reproduces_the_larger_calls_bytes():
    raw, codes = cr.parity_capture(), cr.parity_codes()
    channels = [postcorr.Channel(*c) for c in cr.parity_channels(6)]
    B, first, n = 48, 5, 4096 + 48 * 20 + 7
    amps = sr.random_amps(6, cr.blocks(n, B), 2 ** 15)
    whole, _ = sr.subtract(raw, first, n, B, codes, channels, amps, sr.DITHER, 31)
    for m0 in (1, 7, 86):
        sub_first, sub_n = first + m0 * B, n - m0 * B - 11
        moved = [tuple(postcorr.advance(c, m0 * B)) for c in channels]
        part, _ = sr.subtract(raw, sub_first, sub_n, B, codes, moved, amps[:, m0:m0 + cr.blocks(sub_n, B)], sr.DITHER, 31)
        assert part.tobytes() == whole[2 * m0 * B:2 * (m0 * B + sub_n)].tobytes(), m0
    off, _ = sr.subtract(raw, first + 1, n - 1, B, codes, [tuple(postcorr.advance(c, 1)) for c in channels],
                         amps, sr.DITHER, 31)
    assert off.tobytes() != whole[2:].tobytes(), "a start inside a block is another blocking of the amplitudes"


def test_negative_replicas_are_floored_not_truncated():
    ones, channels, _ = constant_replica_input(0)
    raw = np.full(2 * 64, 100, np.uint8)
    # R = 32 aI; q = floor((R + 32768) / 65536): -32800 + 32768 = -32 goes to -1 where truncation gives 0
    for aI, q in ((-1, 0), (-1024, 0), (-1025, -1), (-3072, -1), (-3073, -2), (1023, 0), (1024, 1)):
        got, _ = sr.subtract(raw, 0, 64, 64, ones, channels, np.array([[[aI, 0]]], np.int32), 0, 0)
        assert (32 * aI + 32768) // 65536 == q and np.all(got[0::2] == 100 - q) and np.all(got[1::2] == 100), (aI, q)


# ------------------------------------------------------------------------------------------------ the Python layers
class HostLib(host_lib.HostLib):
    """gj_corr_bank_dev and gj_subtract_dev computed by the restatements on host memory (tests/host_lib.py)."""

    def gj_corr_bank_dev(self, ctx, d_iq, nbytes, first, n, B, d_codes, n_rows, d_channels, n_channels, taps, n_taps, d_out):
        taps = [int(taps[j]) for j in range(n_taps)]
        self.calls.append(("corr", first, n, B, n_rows, n_channels, tuple(taps)))
        codes = self.view(d_codes, n_rows * 1023, np.int16).reshape(n_rows, 1023)
        channels = [tuple(int(v) for v in c) for c in self.view(d_channels, n_channels, gpsjam.CORR_CHANNEL_DTYPE)]
        out = cr.bank(self.view(d_iq, nbytes), first, n, B, codes, channels, taps)
        self.view(d_out, out.size, np.int32)[:] = out.reshape(-1)
        return 0

    def gj_subtract_dev(self, ctx, d_iq, nbytes, first, n, B, d_codes, n_rows, d_channels, n_channels, d_amp, flags, seed, d_out, d_blocks):
        self.calls.append(("subtract", first, n, B, n_rows, n_channels, flags, seed))
        codes = self.view(d_codes, n_rows * 1023, np.int16).reshape(n_rows, 1023)
        channels = [tuple(int(v) for v in c) for c in self.view(d_channels, n_channels, gpsjam.CORR_CHANNEL_DTYPE)]
        amps = self.view(d_amp, 2 * n_channels * cr.blocks(n, B), np.int32).reshape(n_channels, -1, 2)
        out, rec = sr.subtract(self.view(d_iq, nbytes), first, n, B, codes, channels, amps, flags, seed)
        self.view(d_out, 2 * n)[:] = out
        if d_blocks:
            self.view(d_blocks, rec.size, sr.DTYPE)[:] = rec
        return 0


@pytest.fixture
def host_dev():
    dev = host_lib.host_device(HostLib())
    yield dev
    dev._ctx = None            # a Capture that outlives the test frees nothing


def test_device_subtract_on_the_host_double(host_dev):
    raw, codes, channels, lib = cr.parity_capture(), cr.parity_codes(), cr.parity_channels(3), host_dev._lib
    n = 2 * 4096 + 5
    amps = sr.random_amps(3, cr.blocks(n, 256), 2 ** 14)
    want, wrec = sr.subtract(raw, 3, n, 256, codes, channels, amps, sr.DITHER, 0)
    uploads = gpsjam.Capture.uploads
    cleaned, rec = host_dev.subtract(raw, channels, codes, amps, first_sample=3, n_samples=n)
    assert gpsjam.Capture.uploads == uploads + 1, "host bytes are uploaded once; the result is no upload"
    assert isinstance(cleaned, gpsjam.Capture) and cleaned.nbytes == 2 * n and cleaned.download().tobytes() == want.tobytes()
    assert rec.dtype == gpsjam.SUB_DTYPE and rec.tobytes() == wrec.tobytes() and rec.size == 3
    assert host_lib.mallocs(lib) == [codes.nbytes, amps.nbytes, 3 * 32, 2 * n, 3 * 24]
    assert lib.calls[-1] == ("subtract", 3, n, 256, 4, 3, 1, 0)
    assert set(lib.mem) == {cleaned.ptr}, "everything but the result is freed"
    cleaned.free()
    assert not lib.mem and host_dev.kernel_calls == {"subtract": 1}
    # a resident capture, records as a structured array, the range to the end, no dither, a seed, another block size
    rec_ch = np.array(channels, gpsjam.CORR_CHANNEL_DTYPE)
    with gpsjam.Capture(host_dev, raw) as cap:
        uploads = gpsjam.Capture.uploads
        rest = cr.PARITY_SAMPLES - 5
        amps = sr.random_amps(3, cr.blocks(rest, 4096), 2 ** 16)
        out, rec = host_dev.subtract(cap, rec_ch, codes, amps, first_sample=5, block_samples=4096, dither=False, seed=2 ** 32 + 9)
        assert gpsjam.Capture.uploads == uploads and out.nsamples == rest and lib.calls[-1][-2:] == (0, 9)
        assert out.download().tobytes() == sr.subtract(raw, 5, rest, 4096, codes, channels, amps, 0, 9)[0].tobytes()
        assert set(lib.mem) == {cap.ptr, out.ptr}
        out.free()
        with pytest.raises(ValueError):
            host_dev.subtract(cap, rec_ch, codes, amps[:, :-1], first_sample=5, block_samples=4096)
        assert set(lib.mem) == {cap.ptr}


def test_device_subtract_checks_the_channels_on_the_host_and_frees_everything(host_dev):
    raw, codes, lib = cr.parity_capture(), cr.parity_codes(), host_dev._lib
    good = cr.parity_channels(2)
    n_blocks = cr.blocks(cr.PARITY_SAMPLES, 256)
    host_lib.check_freed(host_dev, raw, lambda cap: host_dev.subtract(cap, good, codes, np.zeros((2, n_blocks, 2), np.int32)))
    bad = {"reserved must be 0": (0, 1, 0, 0, 0, 1),
           "code_row 4 outside the 4 rows": (0, 1, 0, 0, 4, 0),
           "code_phase is not below 1023 * 2^32": (cr.PERIOD, 1, 0, 0, 0, 0),
           "code_step is not below 2^34": (0, 2 ** 34, 0, 0, 0, 0)}
    for what, ch in bad.items():
        lib.calls.clear()
        host_lib.check_refused(host_dev, raw, lambda s: host_dev.subtract(s, good + [ch], codes, np.zeros((3, n_blocks, 2), np.int32)),
                               gpsjam.GpsJamError, f"gpsjam: invalid argument: channel 2: {what} (status -1)")
        assert not [c for c in lib.calls if c[0] == "subtract"], "the library is not reached"
    lib.refuse("gj_subtract_dev")
    host_lib.check_refused(host_dev, raw, lambda s: host_dev.subtract(s, good, codes, np.zeros((2, cr.blocks(cr.PARITY_SAMPLES, 32), 2), np.int32),
                                                                      block_samples=32),
                           gpsjam.GpsJamError, host_lib.REFUSED_TEXT, counted="subtract")


class FakeBank:
    """What postcorr.amplitudes reads of a CorrBank."""

    def __init__(self, z, B, n):
        self.z, self.block_samples, self.n_samples = np.asarray(z, np.complex128), B, n

    def tap(self, offset=0):
        return self.z


def test_amplitudes_groups_periods_from_first_block_with_a_head_group_and_a_ragged_block():
    B, n = 256, 21 * 256 + 100                                   # 22 blocks, the last one of 100 samples
    rng = np.random.default_rng(8)
    z = rng.normal(0, 1e5, (3, 22)) + 1j * rng.normal(0, 1e5, (3, 22))
    got = postcorr.amplitudes(FakeBank(z, B, n), [3, 0, 8 + 5])
    assert got.shape == (3, 22, 2) and got.dtype == np.int32
    groups = {0: [(0, 3), (3, 11), (11, 19), (19, 22)], 1: [(0, 8), (8, 16), (16, 22)], 2: [(0, 5), (5, 13), (13, 21), (21, 22)]}
    for k, spans in groups.items():
        for lo, hi in spans:
            samples = (hi - lo) * B - (B - 100 if hi == 22 else 0)
            alpha = z[k, lo:hi].sum() / (samples * 1042.5) * 65536.0
            assert np.all(got[k, lo:hi] == [int(round(alpha.real)), int(round(alpha.imag))]), (k, lo, hi)
    # the amplitude takes out what the bank saw: a replica made with it gives the bank's own sum back within the table's 1.8 %
    codes = postcorr.codes([11])
    ch = postcorr.channel(0, 100.25, 1234.0, cr.FS, 0.3)
    amps = np.tile(np.array([3000, -1500], np.int32), (1, 8, 1))
    R = sr.replica(0, 2048, 256, codes, [tuple(ch)], amps)
    raw = cr.quantise((R[:, 0] + 1j * R[:, 1]) / 65536.0 * 32.0)          # 32 times the replica, so that the bytes resolve it
    iq = cr.bank(raw, 0, 2048, 256, codes, [tuple(ch)], (0,))
    back = postcorr.amplitudes(FakeBank(iq[:, :, 0, 0] + 1j * iq[:, :, 0, 1], 256, 2048), [0])
    assert np.all(np.abs(back[0] / 32.0 - [3000, -1500]) < 0.03 * 3000), back[0, 0]


# ------------------------------------------------------------------------------------------------ end to end
def oracle_surface(raw, prn, steps=10):
    """P[n_freq][nsamp] of the oracle's pcorrelator over ``steps`` steps, with no early stop (as tests/test_peaks_host.py)."""
    freqs = list(gnss.doppler_bins())
    codex = orc.acq_code_fft(prn, NSAMP)
    P = np.zeros(len(freqs) * NSAMP, np.float64)
    for i in range(steps):
        loc = i * NSAMP
        data = (np.asarray(raw[2 * loc:2 * (loc + 2 * NSAMP)]).astype(np.int16) - 128).astype(np.int8)
        orc.acq_pcorrelator(data, 1.0 / cr.FS, NSAMP, freqs, 2 * NSAMP, codex, P)
    return P.reshape(len(freqs), NSAMP)


@pytest.fixture(scope="module")
def cleaned_overpowered():
    dev = host_lib.host_device(HostLib())
    a, b = pr.overpowered_pair()
    res = mitigate.clean_spoofed(dev, a, b, k=2, search=pr.TruthSearch("overpowered"), tol=cr.E2E_TOL)
    out = res, res.capture_a.download(), res.capture_b.download()
    res.capture_a.free()
    res.capture_b.free()
    assert not dev._lib.mem, "everything is freed"
    dev._ctx = None
    return out


def test_end_to_end_the_cleaned_capture_holds_the_authentic_signals_alone(cleaned_overpowered):
    """The condition: on cleaned a the oracle's surface of each PRN has its largest cell at the authentic truth and no
    second peak above the threshold of 10 steps and 71 x 2048 cells."""
    res, clean_a, _ = cleaned_overpowered
    prns = [cr.E2E_PRNS[k] for k in pr.E2E_IDX]
    assert res.report.spoofed is True and [r.prn for r in res.removals_a] == prns == [r.prn for r in res.removals_b]
    assert clean_a.size == 2 * cr.E2E_SAMPLES and res.records_a.size == sr.blocks(cr.E2E_SAMPLES)
    print(f"bytes clipped: {int(res.records_a['n_clipped'].sum())} and {int(res.records_b['n_clipped'].sum())}; removed share "
          f"{res.records_a['removed'].sum() / res.records_a['total'].sum():.4f}")
    gamma = gnss.peak_threshold(10, 71 * NSAMP, 1e-3)
    freqs = gnss.doppler_bins()
    for k in pr.E2E_IDX:
        prn = cr.E2E_PRNS[k]
        peaks, (mean, kept) = pr.top_k(oracle_surface(clean_a, prn), 2, 2 * NSAMPCHIP)
        (p0, code, freq), (p1, code1, freq1) = peaks
        print(f"PRN {prn}: first peak {p0 / mean:.2f} at code {code} / {freqs[freq]:+.0f} Hz (truth {cr.E2E_CODE_INDEX[k]} / {cr.E2E_DOPPLER[k]:+.0f}), "
              f"second peak {p1 / mean:.2f} at code {code1} / {freqs[freq1]:+.0f} Hz (gamma {gamma:.3f})")
        assert abs(code - cr.E2E_CODE_INDEX[k]) <= 1.0 and abs(freqs[freq] - cr.E2E_DOPPLER[k]) <= 200.0, (prn, code, freqs[freq])
        assert p0 / mean > gamma > p1 / mean, (prn, p0 / mean, p1 / mean)


def one_step_peak(raw, prn, steps=1):
    """(code index, Doppler of the bin, surface): the largest cell of the oracle's surface after ``steps`` steps, which
    is what the plain search decides on when it stops there."""
    P = oracle_surface(raw, prn, steps)
    f, c = divmod(int(np.argmax(P)), NSAMP)
    return c, float(gnss.doppler_bins()[f]), P


def test_one_step_of_the_plain_search_resolves_the_doppler_to_a_bin_either_side(cleaned_overpowered):
    """Why tests/subtract/test_round6_gpu.py lets PRN 14 of the cleaned capture land one Doppler bin from the nearest.
    The plain search stops at the first step that passes its threshold: one millisecond, a main lobe 1 kHz wide, where
    200 Hz off the centre cost 0.6 dB.  On the oracle's ONE-step surface of the cleaned capture PRN 14 (+356 Hz,
    nearest bin +400) has its largest cell at the authentic code index in the +600 bin, 3 % above the +400 cell of the
    same column; at two steps it is in +400.  That is the yardstick and not the cleaning: on the NEVER-spoofed pair,
    with nothing of the subtraction in the path, PRN 4 (-2431) lands in -2200 and PRN 30 (-788) in -600 at one step,
    and PRN 14 in +200 at two.  The code index, which tells the authentic signal from the copy, is right every time."""
    _, clean_a, _ = cleaned_overpowered
    freqs = list(gnss.doppler_bins())
    code, dop, P = one_step_peak(clean_a, 14)
    win, near = P[freqs.index(600.0), code], P[freqs.index(400.0), code]
    print(f"cleaned PRN 14, one step: code {code}, bin {dop:+.0f}, power {win:.4f} against {near:.4f} in the +400 bin")
    assert abs(code - cr.E2E_CODE_INDEX[2]) <= 1.0 and dop == 600.0 and near < win < 1.05 * near
    code, dop, _ = one_step_peak(clean_a, 14, steps=2)
    assert abs(code - cr.E2E_CODE_INDEX[2]) <= 1.0 and dop == 400.0
    for k in (1, 3, 4):                                    # PRNs 9, 21 and 30 of the cleaned capture: the nearest bin at one step
        code, dop, _ = one_step_peak(clean_a, cr.E2E_PRNS[k])
        assert abs(code - cr.E2E_CODE_INDEX[k]) <= 1.0 and abs(dop - cr.E2E_DOPPLER[k]) <= 100.0, (k, code, dop)
    auth, _ = cr.e2e_pair("authentic")
    for k, steps, lands in ((0, 1, -2200.0), (4, 1, -600.0), (2, 2, 200.0), (2, 1, 400.0)):
        code, dop, _ = one_step_peak(auth, cr.E2E_PRNS[k], steps)
        print(f"never-spoofed PRN {cr.E2E_PRNS[k]}, {steps} step(s): code {code}, bin {dop:+.0f} (truth {cr.E2E_DOPPLER[k]:+.0f})")
        assert abs(code - cr.E2E_CODE_INDEX[k]) <= 1.0 and dop == lands, (k, steps, code, dop)


def test_end_to_end_figures_set_the_gpu_tests_tolerances(cleaned_overpowered, host_dev):
    """Re-measures sr.E2E_CPU_*: the smallest suppression of the ten removals, and the largest phase and C/N0 errors of
    the authentic signals on the cleaned pair, which spoof.scan does not flag."""
    res, clean_a, clean_b = cleaned_overpowered
    for name, rows in (("a", res.removals_a), ("b", res.removals_b)):
        for r in rows:
            print(f"antenna {name} PRN {r.prn}: code {r.code_index}, Doppler {r.doppler_hz:+.1f} Hz, C/N0 {r.cn0_before:.1f} -> {r.cn0_after:.1f} dB-Hz, "
                  f"suppression {r.suppression_db:.1f} dB")
    smallest = min(r.suppression_db for r in res.removals_a + res.removals_b)
    report = spoof.scan(host_dev, clean_a, clean_b, cr.GridSearch("authentic"), tol=cr.E2E_TOL)
    assert report.spoofed is False and report.prns == [cr.E2E_PRNS[k] for k in pr.E2E_IDX]
    worst = {"phase": 0.0, "cn0": 0.0}
    for prn, ph, c in zip(report.prns, report.phase, report.cn0):
        k = cr.E2E_PRNS.index(prn)
        e_ph, e_cn0 = abs(float(cr.wrap(ph - cr.E2E_AUTHENTIC[k]))), abs(c - cr.E2E_CN0[k])
        print(f"cleaned PRN {prn}: phase {ph:+.4f} (error {e_ph:.4f}), C/N0 {c:.2f} (error {e_cn0:.2f} dB)")
        worst = {"phase": max(worst["phase"], e_ph), "cn0": max(worst["cn0"], e_cn0)}
    print(f"smallest suppression {smallest:.2f} dB, worst of the cleaned authentic signals: {worst}")
    for got, recorded in ((smallest, sr.E2E_CPU_MIN_SUPPRESSION_DB), (worst["phase"], sr.E2E_CPU_ERROR_PHASE), (worst["cn0"], sr.E2E_CPU_ERROR_CN0)):
        assert abs(got - recorded) <= 0.1 * recorded, (got, recorded)
    assert (sr.E2E_TOL_PHASE, sr.E2E_TOL_CN0) == (2 * sr.E2E_CPU_ERROR_PHASE, 2 * sr.E2E_CPU_ERROR_CN0)
    assert sr.E2E_GPU_MIN_SUPPRESSION_DB == sr.E2E_CPU_MIN_SUPPRESSION_DB - 6.0
    assert worst["cn0"] < pr.E2E_CPU_ERROR_CN0, "the authentic signals read nearer their C/N0 than under the copies"


def test_the_authentic_pair_comes_back_byte_for_byte(host_dev):
    a, b = cr.e2e_pair("authentic")
    res = mitigate.clean_spoofed(host_dev, a, b, k=2, search=pr.TruthSearch("authentic"), tol=cr.E2E_TOL)
    assert res.report.spoofed is False and res.removals_a == [] == res.removals_b
    assert res.capture_a.download().tobytes() == a.tobytes() and res.capture_b.download().tobytes() == b.tobytes()
    assert not res.records_a["removed"].any() and not res.records_b["n_clipped"].any()
    res.capture_a.free()
    res.capture_b.free()
    assert not host_dev._lib.mem


def test_more_candidates_than_a_bank_go_out_in_slices_and_the_records_add_up(host_dev, monkeypatch, cleaned_overpowered):
    """Five candidates at two per pass: three subtractions, each from the range the one before left; ``total`` is the
    input's, ``removed`` and ``n_clipped`` the sums over the passes; the signals go out as in one pass."""
    res, _, _ = cleaned_overpowered
    a, _ = pr.overpowered_pair()
    monkeypatch.setattr(spoof, "BANK_CHANNELS", 2)
    lib = host_dev._lib
    out = spoof.remove(host_dev, a, res.report.counterfeit, pr.TruthSearch("overpowered"))
    passes = [c for c in lib.calls if c[0] == "subtract"]
    assert [c[5] for c in passes] == [2, 2, 1] and [c[1] for c in passes] == [0, 0, 0]
    assert [r.prn for r in out.removals] == [r.prn for r in res.removals_a] and len(out.observations) == 5
    for got, one in zip(out.removals, res.removals_a):
        print(f"PRN {got.prn}: suppression {got.suppression_db:.1f} dB in slices, {one.suppression_db:.1f} dB in one pass")
        assert got.suppression_db >= sr.E2E_GPU_MIN_SUPPRESSION_DB, (got, one)      # the factor of two the GPU test allows
    assert np.array_equal(out.records["total"], res.records_a["total"]), "the input's power, read by the first pass"
    # each pass alone, from the bytes it was given: the records are their sums
    removed, clipped, src = np.zeros(out.records.size, np.uint64), np.zeros(out.records.size, np.int32), np.asarray(a)
    for at in (0, 2, 4):
        part = spoof.remove(host_dev, src, res.report.counterfeit[at:at + 2], pr.TruthSearch("overpowered"))
        removed, clipped, src = removed + part.records["removed"], clipped + part.records["n_clipped"], part.capture.download()
        part.capture.free()
    assert np.array_equal(out.records["removed"], removed) and np.array_equal(out.records["n_clipped"], clipped)
    assert out.capture.download().tobytes() == src.tobytes()
    out.capture.free()
    assert not lib.mem


def test_the_spoofed_command_line_through_the_double(tmp_path, monkeypatch, capsys):
    a, b = pr.overpowered_pair()
    pa, pb, oa, ob = (str(tmp_path / name) for name in ("a.bin", "b.bin", "out_a.bin", "out_b.bin"))
    a.tofile(pa)
    b.tofile(pb)
    lib = HostLib()
    dev = host_lib.host_device(lib)                         # gpsjam.Device on the double, with ``capture`` reading the file on the host
    dev.capture = lambda path: gpsjam.Capture(dev, np.fromfile(path, np.uint8))
    dev.close = lambda: None
    monkeypatch.setattr(gpsjam, "Device", lambda index=0: dev)
    monkeypatch.setattr(gnss, "AcqSearch", lambda dev, fs=cr.FS: type("S", (pr.TruthSearch,), {"close": lambda self: None})("overpowered", fs))
    assert mitigate.main([pa, oa, "--spoofed", pb, "--peaks", "2", "--out-b", ob]) == 0
    text = capsys.readouterr().out
    assert "SPOOFED" in text and text.count("suppression") == 10 and "counterfeit (in the arc): 5" in text and "bytes clipped" in text
    got_a, got_b = np.fromfile(oa, np.uint8), np.fromfile(ob, np.uint8)
    assert got_a.size == a.size == got_b.size and not np.array_equal(got_a, a) and not np.array_equal(got_b, b)
    assert not lib.mem
    for other in ("--pulsed", "--swept", "--spatial"):
        with pytest.raises(SystemExit):
            mitigate.main([pa, oa, "--spoofed", pb] + ([other, pb] if other == "--spatial" else [other]))
