"""CPU side of the correlator bank and what is built on it (gj_corr_bank_dev, gj_corr_blocks, Device.corr_bank,
gpsjam.postcorr, gpsjam.spoof): the interface, the integer restatement the GPU tests compare with
(tests/corr_restatement.py) checked against a per-sample Python-int loop and against the definition's own consequences,
the Python layers on a host double of the library, the chance bound against a Monte-Carlo, and the accuracy of the float
chain on restated integers, which sets the tolerances of the GPU test.  No GPU call is made.

The tests under "the restatement" exercise tests/corr_restatement.py alone: they check the yardstick.  The float chain
is not restated anywhere: gpsjam.postcorr and gpsjam.spoof themselves run here, on restated integers."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import corr_restatement as cr
import gpsjam
import host_lib
from gpsjam import _ffi, gnss, postcorr, spoof

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gpsjam.h")


# ------------------------------------------------------------------------------------------------ interface
def test_symbols_bindings_and_python_interface():
    lib = _ffi.load()
    assert len(_ffi.SIGNATURES["gj_corr_bank_dev"][1]) == 13 and len(_ffi.SIGNATURES["gj_corr_blocks"][1]) == 2
    for name in ("gj_corr_bank_dev", "gj_corr_blocks"):
        assert callable(getattr(lib, name))
    assert _ffi.GJ_VERSION == 150 == lib.gj_version()
    assert _ffi.GJ_CORR_MAX_BLOCK == gpsjam.CORR_MAX_BLOCK == cr.MAX_BLOCK == 4096
    assert (_ffi.GJ_CORR_MAX_TAPS, _ffi.GJ_CORR_MAX_TAP_OFFSET, _ffi.GJ_CORR_MAX_CHANNELS) == (cr.MAX_TAPS, cr.MAX_TAP_OFFSET, cr.MAX_CHANNELS) == (9, 64, 64)
    assert (_ffi.GJ_CORR_MAX_SAMPLES, _ffi.GJ_CORR_MAX_CODE_STEP, _ffi.GJ_CORR_CODE_LEN) == (2 ** 28, 2 ** 34, 1023)
    assert C.sizeof(_ffi.CorrChannel) == 32 == gpsjam.CORR_CHANNEL_DTYPE.itemsize
    assert [f[0] for f in _ffi.CorrChannel._fields_] == list(gpsjam.CORR_CHANNEL_DTYPE.names) == list(postcorr.Channel._fields)
    for name in ("corr_bank", "corr_bank_dev"):
        assert callable(getattr(gpsjam.Device, name))
    for name in ("corr_blocks", "CORR_MAX_BLOCK", "CorrBank"):
        assert name in gpsjam.__all__
    assert gpsjam.CorrBank._fields == ("iq", "taps", "block_samples", "n_samples")
    for n, B in ((0, 16), (1, 16), (15, 16), (16, 16), (17, 16), (4095, 4096), (3 * 2048 + 5, 2048), (2 ** 40 + 1, 4096)):
        assert gpsjam.corr_blocks(n, B) == -(-n // B) == cr.blocks(n, B), (n, B)
    assert gpsjam.corr_blocks(100, 0) == 0 and gpsjam.corr_blocks(-1, 16) == 0 and lib.gj_corr_blocks(100, -16) == 0


def test_the_headers_tables_and_constants_are_the_formulas():
    text = open(HEADER).read()
    table = re.search(r"#define GJ_CORR_COS_TABLE \{([^}]*)\}", text).group(1)
    header = tuple(int(v) for v in table.split(","))
    assert header == cr.COS == _ffi.GJ_CORR_COS_TABLE == (32, 30, 23, 12, 0, -12, -23, -30, -32, -30, -23, -12, 0, 12, 23, 30)
    assert cr.SIN == tuple(int(math.floor(math.sin(2.0 * math.pi * i / 16.0) * 32.0 + 0.5)) if i not in (0, 8) else 0 for i in range(16))
    assert max(abs(c) + abs(s) for c, s in zip(cr.COS, cr.SIN)) == 46 and cr.RECORD_BOUND == 24117248 < 2.5e7 < 2 ** 31
    for name, value in (("MAX_BLOCK", 4096), ("MAX_TAPS", 9), ("MAX_TAP_OFFSET", 64), ("MAX_CHANNELS", 64), ("CODE_LEN", 1023)):
        assert int(re.search(rf"#define GJ_CORR_{name} (\d+)", text).group(1)) == value
    assert "#define GJ_VERSION 150" in text or re.search(r"GJ_VERSION\s+150", text)


# ------------------------------------------------------------------------------------------------ the restatement
def small_input(seed, n_samples=120):
    rng = np.random.default_rng(seed)
    raw = rng.integers(0, 256, 2 * n_samples).astype(np.uint8)
    raw[:8] = (0, 0, 255, 255, 0, 255, 255, 0)
    return raw


@pytest.mark.parametrize("B", [16, 48])
def test_restatement_equals_the_python_int_loop(B):
    raw, codes = small_input(B), cr.parity_codes()
    channels = cr.parity_channels(8)
    for first, n in ((0, 1), (3, 15), (1, B - 1), (0, B), (5, B + 1), (2, 2 * B + 5)):
        for taps in ((0,), (0, -1, 1), (64, -64, 0, 1, -1, 2, -2, 33, -17)):
            got = cr.bank(raw, first, n, B, codes, channels, taps)
            want = np.array(cr.brute(raw, first, n, B, codes, channels, taps), np.int64)
            assert got.shape == (8, cr.blocks(n, B), len(taps), 2)
            assert np.array_equal(got, want), (first, n, taps)


def test_block_records_add_up_to_the_one_block_call():
    raw, codes, channels = cr.parity_capture(), cr.parity_codes(), cr.parity_channels(6)
    n = 4096 - 11
    whole = cr.bank(raw, 7, n, 4096, codes, channels, (0, -1, 1))
    assert whole.shape == (6, 1, 3, 2)
    for B in (16, 2048, 1920):
        parts = cr.bank(raw, 7, n, B, codes, channels, (0, -1, 1))
        assert parts.shape[1] == -(-n // B) and np.array_equal(parts.sum(axis=1), whole[:, 0]), B


def test_a_tap_is_the_prompt_of_the_channel_advanced_by_it():
    raw, codes, channels = cr.parity_capture(), cr.parity_codes(), cr.parity_channels(8)
    for d in (1, -1, 64, -64, 7):
        moved = [(ch[0] + d * ch[1]) % cr.PERIOD for ch in channels]
        shifted = [(m,) + tuple(ch[1:]) for m, ch in zip(moved, channels)]
        a = cr.bank(raw, 3, 5000, 2048, codes, channels, (d,))
        b = cr.bank(raw, 3, 5000, 2048, codes, shifted, (0,))
        assert np.array_equal(a, b), d


def test_saturated_captures_reach_the_bound_without_wrapping():
    """All bytes 0 is I = Q = -128: with the all-ones row and a still carrier at table index i the record is
    -128 (C - S) B and -128 (S + C) B; index 2 (23, 23) and index 14 (23, -23) give the 46 of the bound."""
    ones = np.ones((1, 1023), np.int16)
    n = 4096
    for value, sign in ((0, -128), (255, 127)):
        raw = np.full(2 * n, value, np.uint8)
        for i in range(16):
            got = cr.bank(raw, 0, n, 4096, ones, [(0, 0, i << 28, 0, 0, 0)], (0,))[0, 0, 0]
            assert got.tolist() == [sign * (cr.COS[i] - cr.SIN[i]) * n, sign * (cr.SIN[i] + cr.COS[i]) * n], (value, i)
    raw = np.full(2 * n, 0, np.uint8)
    assert cr.bank(raw, 0, n, 4096, ones, [(0, 0, 14 << 28, 0, 0, 0)], (0,))[0, 0, 0, 0] == -cr.RECORD_BOUND
    alt = np.tile(np.array([0, 255], np.uint8), n)                     # I = -128, Q = 127 throughout
    assert cr.bank(alt, 0, n, 4096, ones, [(0, 0, 2 << 28, 0, 0, 0)], (0,))[0, 0, 0].tolist() == [23 * -255 * n, 23 * -1 * n]


def test_parity_channels_exercise_what_they_claim():
    ch = cr.parity_channels(64)
    steps = cr.code_steps()
    assert len(ch) == 64 and ch[1][4] == ch[2][4], "two channels share a code row"
    assert {0, cr.PERIOD - 1} <= {c[0] for c in ch} and set(steps) <= {c[1] for c in ch}
    assert {0, 1, 0xFFFFFFFF, 0x80000000} <= {c[3] for c in ch}
    assert abs(steps[0] / 2 ** 32 - 0.4995) < 1e-4 and 4096 * steps[0] >= 2 * cr.PERIOD, "two wraps inside a 4096 block"
    assert abs(steps[1] / 2 ** 32 - 1.998) < 1e-3 and steps[2] == 2 ** 34 - 1 and steps[3] == 0
    assert all(0 <= c[0] < cr.PERIOD and 0 <= c[1] < cr.MAX_CODE_STEP and 0 <= c[4] < 4 and c[5] == 0 for c in ch)
    # carr_phase = k 2^28 - 1 with step 1: the table index changes at sample 1
    assert ((ch[1][2] + 0) >> 28, (ch[1][2] + 1) >> 28) == (4, 5)
    raw = cr.parity_capture()
    pairs = set(zip(raw[0::2].tolist(), raw[1::2].tolist()))
    assert {(0, 0), (0, 255), (255, 0), (255, 255)} <= pairs and raw.size == 2 * cr.PARITY_SAMPLES


# ------------------------------------------------------------------------------------------------ the Python layers
class HostLib(host_lib.HostLib):
    """gj_corr_bank_dev computed by the restatement on host memory (tests/host_lib.py)."""

    def gj_corr_bank_dev(self, ctx, d_iq, nbytes, first, n, B, d_codes, n_rows, d_channels, n_channels, taps, n_taps, d_out):
        taps = [int(taps[j]) for j in range(n_taps)]
        self.calls.append(("corr", first, n, B, n_rows, n_channels, tuple(taps)))
        codes = self.view(d_codes, n_rows * 1023, np.int16).reshape(n_rows, 1023)
        channels = [tuple(int(v) for v in c) for c in self.view(d_channels, n_channels, gpsjam.CORR_CHANNEL_DTYPE)]
        out = cr.bank(self.view(d_iq, nbytes), first, n, B, codes, channels, taps)
        self.view(d_out, out.size, np.int32)[:] = out.reshape(-1)
        return 0


@pytest.fixture
def host_dev():
    dev = host_lib.host_device(HostLib())
    yield dev
    dev._ctx = None            # a Capture that outlives the test frees nothing


def test_device_corr_bank_on_the_host_double(host_dev):
    raw, codes, channels, lib = cr.parity_capture(), cr.parity_codes(), cr.parity_channels(3), host_dev._lib
    n = 2 * 2048 + 5
    want = cr.bank(raw, 3, n, 2048, codes, channels, (0, -1, 1))
    uploads = gpsjam.Capture.uploads
    got = host_dev.corr_bank(raw, channels, codes, first_sample=3, n_samples=n)
    assert gpsjam.Capture.uploads == uploads + 1, "host bytes are uploaded once"
    assert isinstance(got, gpsjam.CorrBank) and got.taps == (0, -1, 1) and got.block_samples == 2048 and got.n_samples == n
    assert got.iq.dtype == np.int32 and got.iq.shape == (3, 3, 3, 2) and np.array_equal(got.iq, want)
    assert np.array_equal(got.tap(-1), want[:, :, 1, 0] + 1j * want[:, :, 1, 1])
    assert host_lib.mallocs(lib) == [codes.nbytes, 3 * 32, 8 * 3 * 3 * 3] and lib.calls[-1] == ("corr", 3, n, 2048, 4, 3, (0, -1, 1))
    assert not lib.mem, "everything is freed"
    assert host_dev.kernel_calls == {"corr_bank": 1}
    # a resident capture, records as a structured array, the range to the end, one tap, another block size
    rec = np.array(channels, gpsjam.CORR_CHANNEL_DTYPE)
    with gpsjam.Capture(host_dev, raw) as cap:
        uploads = gpsjam.Capture.uploads
        rest = host_dev.corr_bank(cap, rec, codes, first_sample=5, block_samples=4096, taps=(7,))
        assert gpsjam.Capture.uploads == uploads and rest.n_samples == cr.PARITY_SAMPLES - 5
        assert np.array_equal(rest.iq, cr.bank(raw, 5, rest.n_samples, 4096, codes, channels, (7,)))
        assert set(lib.mem) == {cap.ptr}, "everything but the input is freed"


def test_device_corr_bank_checks_the_channels_on_the_host_and_frees_everything(host_dev):
    raw, codes, lib = cr.parity_capture(), cr.parity_codes(), host_dev._lib
    good = cr.parity_channels(2)
    host_lib.check_freed(host_dev, raw, lambda cap: host_dev.corr_bank(cap, good, codes))
    bad = {"reserved must be 0": (0, 1, 0, 0, 0, 1),
           "code_row 4 outside the 4 rows": (0, 1, 0, 0, 4, 0),
           "code_row -1 outside the 4 rows": (0, 1, 0, 0, -1, 0),
           "code_phase is not below 1023 * 2^32": (cr.PERIOD, 1, 0, 0, 0, 0),
           "code_step is not below 2^34": (0, 2 ** 34, 0, 0, 0, 0)}
    for what, ch in bad.items():
        lib.calls.clear()
        host_lib.check_refused(host_dev, raw, lambda s: host_dev.corr_bank(s, good + [ch], codes), gpsjam.GpsJamError,
                               f"gpsjam: invalid argument: channel 2: {what} (status -1)")
        assert not [c for c in lib.calls if c[0] == "corr"], "the library is not reached"
    with pytest.raises(gpsjam.GpsJamError) as e:
        host_dev.corr_bank(raw, [(0, 1, 2 ** 32, 0, 0, 0)], codes)
    assert e.value.status == -1 and not lib.mem
    with pytest.raises(ValueError):
        host_dev.corr_bank(raw, good, np.ones((2, 1000), np.int16))
    assert not lib.mem
    lib.refuse("gj_corr_bank_dev")
    host_lib.check_refused(host_dev, raw, lambda s: host_dev.corr_bank(s, good, codes, block_samples=24), gpsjam.GpsJamError,
                           host_lib.REFUSED_TEXT, counted="corr_bank")


# ------------------------------------------------------------------------------------------------ postcorr
def test_channel_fields_and_the_mixers_sign():
    ch = postcorr.channel(3, 1022.75, 2200.0, cr.FS, 0.25)
    assert ch.code_phase == int(round(1022.75 * 2 ** 32)) and ch.carr_phase == 2 ** 30 and ch.code_row == 3 and ch.reserved == 0
    assert ch.code_step == int(round(gnss.CA_RATE * (1 + 2200.0 / 1575.42e6) / cr.FS * 2 ** 32))
    assert ch.carr_step == int(round(2200.0 / cr.FS * 2 ** 32))
    neg = postcorr.channel(0, -0.5, -2200.0, cr.FS, -0.25)
    assert neg.carr_step == 2 ** 32 - ch.carr_step and neg.carr_phase == 3 * 2 ** 30 and neg.code_phase == int(1022.5 * 2 ** 32)
    assert postcorr.channel(0, 1023.0, 0.0, cr.FS).code_phase == 0 and postcorr.channel(0, 1023 - 2.0 ** -34, 0.0, cr.FS).code_phase == 0
    moved = postcorr.advance(ch, -700)
    assert moved.code_phase == (ch.code_phase - 700 * ch.code_step) % cr.PERIOD and moved.carr_phase == (ch.carr_phase - 700 * ch.carr_step) % 2 ** 32
    # a capture holding code exp(-2j pi dop t), as every generator here writes it, peaks at doppler = +dop
    n, dop = 8 * 2048, 2200.0
    t = np.arange(n)
    chips = ((t - 700) * gnss.CA_RATE / cr.FS) % 1023
    raw = cr.quantise(60.0 * gnss.ca_code(11)[chips.astype(np.int64)] * np.exp(-2j * np.pi * dop * t / cr.FS))
    power = {}
    for d in (dop, -dop, 0.0):
        c = postcorr.advance(postcorr.channel(0, 0.0, d, cr.FS), -700)
        power[d] = float(np.abs(cr.bank(raw, 0, n, 2048, postcorr.codes([11]), [c], (0,))[0, :, 0, :].astype(float)).sum())
    assert power[dop] > 10 * power[-dop] and power[dop] > 10 * power[0.0], power
    assert postcorr.codes([11, 5]).shape == (2, 1023) and np.array_equal(postcorr.codes([11, 5])[0], gnss.ca_code(11))


def test_channels_from_acq_takes_the_code_phase_from_code_index():
    s = cr.GridSearch("authentic")
    res = s.search(None, 0)
    res[1].acquired = False
    prns, chans = postcorr.channels_from_acq(s, res, 0)
    assert prns == [4, 14, 21, 30] and [c.code_row for c in chans] == [0, 1, 2, 3]
    for c, r in zip(chans, [res[0]] + res[2:]):
        assert c.code_step == postcorr.channel(0, 0.0, r.doppler_hz, s.fs).code_step
        assert (c.code_phase + r.code_index * c.code_step) % cr.PERIOD == 0, "the code starts code_index samples on"
        assert c.carr_step == postcorr.channel(0, 0.0, r.doppler_hz, s.fs).carr_step
    later = postcorr.channels_from_acq(s, res, 100, at_sample=2148, doppler_hz=[1.0, 2.0, 3.0, 4.0])[1]
    assert (later[0].code_phase + (res[0].code_index - 2048) * later[0].code_step) % cr.PERIOD == 0
    assert later[2].carr_step == postcorr.channel(0, 0.0, 3.0, s.fs).carr_step


def test_estimators_on_synthetic_prompts():
    rng = np.random.default_rng(5)
    m, T = 100, 1e-3
    bits = rng.choice((-1.0, 1.0), m)
    for residual in (0.0, 37.5, -91.0, 100.0):
        p = 50.0 * bits * np.exp(-2j * np.pi * residual * T * np.arange(m) + 0.4j)
        assert abs(postcorr.residual_doppler(p, T) - residual) < 0.05, residual
    assert postcorr.residual_doppler(np.zeros(10), T) == 0.0 and postcorr.residual_doppler([1.0], T) == 0.0
    # C/N0: amplitude A over complex noise of variance 2 s^2 per prompt: C/N0 = A^2 / (2 s^2 T)
    for cn0 in (38.0, 45.0, 50.0):
        a = math.sqrt(10 ** (cn0 / 10) * 2.0 * T)
        p = a * rng.choice((-1.0, 1.0), 20000) + rng.normal(0, 1, 20000) + 1j * rng.normal(0, 1, 20000)
        assert abs(postcorr.cn0(p, T) - cn0) < 0.3, cn0
    assert postcorr.cn0([], T) == float("-inf") and postcorr.cn0(rng.normal(0, 1, 2000) + 1j * rng.normal(0, 1, 2000), T) < 30.0
    assert postcorr.code_error([3.0, 3.0j], [9.0, 9.0], [1.0, -1.0]) == 0.5 and postcorr.code_error([0], [0], [0]) == 0.0
    assert postcorr.code_shift(0.5, postcorr.Channel(0, 2 ** 31, 0, 0, 0)) == 0.25 and postcorr.code_shift(0.5, postcorr.Channel(0, 2 ** 33, 0, 0, 0)) == 0.0
    assert postcorr.first_block(700, 256) == 3 and postcorr.first_block(1999, 256) == 0 and postcorr.first_block(100, 256) == 0
    assert postcorr.periods(np.arange(20), 3).tolist() == [sum(range(3, 11)), sum(range(11, 19))] and postcorr.periods(np.arange(5), 3).size == 0


# ------------------------------------------------------------------------------------------------ spoof
def test_common_direction_and_its_chance_against_a_monte_carlo():
    c = spoof.common_direction([0.3, 2.4, -1.9, -0.6, 1.5])
    assert len(c.members) == 1 and c.p_chance == 1.0
    c = spoof.common_direction([1.0, 1.1, 3.0, 1.25, 0.96, -2.0], 0.15)
    assert c.members == [0, 1, 3, 4] and abs(c.centre - 1.105) < 1e-9
    assert c.p_chance == spoof.chance(4, 6, 0.15)
    wrapped = spoof.common_direction([3.1, -3.1, 3.0, 0.0], 0.15)               # an arc across +-pi
    assert wrapped.members == [0, 1, 2] and abs(abs(wrapped.centre) - math.pi) < 0.06
    assert spoof.common_direction([]).members == [] and spoof.common_direction([0.5]).members == [0]
    assert spoof.chance(5, 5, 0.15) == pytest.approx(5 * (0.15 / math.pi) ** 4) and spoof.chance(1, 5, 0.15) == 1.0
    # seeded Monte-Carlo under uniform phases, at a wide arc so that the events are frequent enough to count
    rng = np.random.default_rng(11)
    trials, tol = 8000, 0.6
    for n in (4, 6):
        sizes = np.array([len(spoof.common_direction(rng.uniform(-math.pi, math.pi, n), tol).members) for _ in range(trials)])
        for k in range(2, n + 1):
            seen, bound = float(np.mean(sizes >= k)), spoof.chance(k, n, tol)
            sigma = math.sqrt(max(bound * (1 - bound), 1e-12) / trials)
            print(f"n {n} k {k}: seen {seen:.5f}, bound {bound:.5f}")
            assert seen <= bound + 4 * sigma, (n, k, seen, bound)
            if k == n:
                assert abs(seen - bound) <= 4 * sigma, "exact for the full set"


def run_pair(host_dev, kind):
    a, b = cr.e2e_pair(kind)
    search = cr.GridSearch(kind)
    report = spoof.scan(host_dev, a, b, search, tol=cr.E2E_TOL)
    obs = postcorr.observe(host_dev, a, search)
    return report, obs


def test_end_to_end_accuracy_sets_the_tolerances_and_the_verdicts_hold(host_dev):
    """Re-measures cr.E2E_CPU_ERROR_*, which the GPU test's tolerances are twice of, and checks the three verdicts."""
    worst = {"phase": 0.0, "doppler": 0.0, "cn0": 0.0}
    for kind, (idx, phases) in cr.E2E_KINDS.items():
        report, obs = run_pair(host_dev, kind)
        assert report.prns == [cr.E2E_PRNS[k] for k in idx] == [o.prn for o in obs]
        for o, got, co, k, psi in zip(obs, report.phase, report.coherence, idx, phases):
            e_ph, e_dop, e_cn0 = abs(float(cr.wrap(got - psi))), abs(o.doppler_hz - cr.E2E_DOPPLER[k]), abs(o.cn0_dbhz - cr.E2E_CN0[k])
            print(f"{kind} PRN {o.prn}: phase {got:+.4f} (error {e_ph:.4f}), Doppler error {e_dop:.3f} Hz, C/N0 {o.cn0_dbhz:.2f} "
                  f"(error {e_cn0:.2f} dB), code shift {o.code_shift_chips:+.3f} chip, code error left {o.code_error:+.3f}, coherence {co:.3f}")
            assert e_ph <= cr.E2E_TOL_PHASE and e_dop <= cr.E2E_TOL_DOPPLER and e_cn0 <= cr.E2E_TOL_CN0
            assert co > 0.9 and abs(o.code_error) < 0.1 and o.prompts.size in (99, 100)
            worst = {"phase": max(worst["phase"], e_ph), "doppler": max(worst["doppler"], e_dop), "cn0": max(worst["cn0"], e_cn0)}
        if kind == "authentic":
            assert report.spoofed is False and len(report.common_prns) < 4
            # the condition the generator's phases were chosen for: no four within one arc, with margin
            assert len(spoof.common_direction(cr.E2E_AUTHENTIC, cr.E2E_TOL + 2 * cr.E2E_TOL_PHASE).members) < 4
        elif kind == "spoofed":
            assert report.spoofed is True and report.common_prns == report.prns and report.p_chance == pytest.approx(5 * (0.15 / math.pi) ** 4)
            assert float(np.ptp(report.phase)) < 2 * cr.E2E_TOL - 2 * cr.E2E_TOL_PHASE, "inside one arc with margin"
        else:
            assert report.spoofed is True and tuple(report.common_prns) == cr.E2E_MIXED_COMMON
    print("worst:", worst)
    for key, recorded in (("phase", cr.E2E_CPU_ERROR_PHASE), ("doppler", cr.E2E_CPU_ERROR_DOPPLER), ("cn0", cr.E2E_CPU_ERROR_CN0)):
        assert abs(worst[key] - recorded) <= 0.1 * recorded, (key, worst[key], recorded)
    assert (cr.E2E_TOL_PHASE, cr.E2E_TOL_DOPPLER, cr.E2E_TOL_CN0) == (2 * cr.E2E_CPU_ERROR_PHASE, 2 * cr.E2E_CPU_ERROR_DOPPLER, 2 * cr.E2E_CPU_ERROR_CN0)


def test_too_few_prns_give_no_verdict(host_dev):
    a, b = cr.e2e_pair("spoofed")

    class Three(cr.GridSearch):
        def search(self, capture, first_sample=0):
            out = super().search(capture, first_sample)
            for r in out[3:]:
                r.acquired = False
            return out

    report = spoof.scan(host_dev, a, b, Three("spoofed"))
    assert report.prns == [4, 9, 14] and report.spoofed is None and len(report.common_prns) == 3

    class Nothing(cr.GridSearch):
        def search(self, capture, first_sample=0):
            return []

    empty = spoof.scan(host_dev, a, b, Nothing("spoofed"))
    assert empty.prns == [] and empty.spoofed is None and empty.p_chance == 1.0 and postcorr.observe(host_dev, a, Nothing("spoofed")) == []
    assert not host_dev._lib.mem
