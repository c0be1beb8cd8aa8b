"""The correlator bank on the GPU (gj_corr_bank_dev, Device.corr_bank) and what is built on it: post-correlation
observables (gpsjam.postcorr) and the two-antenna spoofing test (gpsjam.spoof).

This file sits in a package of its own on purpose, as tests/fine/ does: the suite orders GPU files by basename
(tests/conftest.py SUITE_ORDER, which tests/test_suite_order.py holds every GPU file to), and under the name
test_round6_gpu.py it runs in stage 2.

Yardstick: the integer restatement of the definition in include/gpsjam.h (tests/corr_restatement.py, which
tests/test_corr_host.py holds to a per-sample Python-int loop).  Everything the kernel makes is integer arithmetic, so
EVERY record is equal, bit for bit.  Every call writes into a sentinel-filled buffer whose 256 bytes behind the call's
records must stay untouched.  The float observables are held to twice the error that tests/test_corr_host.py measures
on the CPU with the same host code on restated integers."""
import math

import numpy as np
import pytest

import corr_restatement as cr
import gpsjam
from gpsjam import gnss, postcorr, spoof
from gpu_lib import GJ_ERR_INVALID, GJ_ERR_UNSUPPORTED, Guarded, freed, refused
from gpu_lib import run_corr as run

pytestmark = pytest.mark.gpu

TAPS9 = (1, -64, 0, 64, -1, 33, -17, 2, -2)     # 0, +-1, +-64 among them, in scrambled order


@pytest.fixture(scope="module")
def cap(dev):
    c = dev.capture(cr.parity_capture())
    yield c
    c.free()


@pytest.fixture(scope="module")
def d_codes(dev):
    b = dev.alloc(cr.parity_codes().nbytes).upload(cr.parity_codes())
    yield b
    b.free()


def compare(dev, capture, raw, first, n, B, d_rows, codes, channels, taps):
    got = run(dev, capture, first, n, B, d_rows, len(codes), channels, taps)
    want = cr.bank(raw, first, n, B, codes, channels, taps)
    np.testing.assert_array_equal(got.astype(np.int64), want, err_msg=f"first {first} n {n} B {B} channels {len(channels)} taps {taps}")
    return got


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("B", [16, 2048, 4096])
def test_parity_with_the_restatement(dev, cap, d_codes, B):
    raw, codes, channels = cr.parity_capture(), cr.parity_codes(), cr.parity_channels(6)
    for n in (1, 15, B - 1, B, B + 1, 3 * B + 5):
        for first in (0, 7, cap.nsamples - n):                   # even, odd, and ending on the capture's last sample
            compare(dev, cap, raw, first, n, B, d_codes, codes, channels, (0, -1, 1))


@pytest.mark.parametrize("n_channels", [1, 3, 64])
def test_channel_counts_and_nine_taps(dev, cap, d_codes, n_channels):
    raw, codes, channels = cr.parity_capture(), cr.parity_codes(), cr.parity_channels(n_channels, seed=n_channels)
    n = 3 * 2048 + 5
    nine = compare(dev, cap, raw, 7, n, 2048, d_codes, codes, channels, TAPS9)
    again = run(dev, cap, 7, n, 2048, d_codes, 4, channels, TAPS9)
    assert nine.tobytes() == again.tobytes(), "two calls, identical bits"
    one = compare(dev, cap, raw, 7, n, 2048, d_codes, codes, channels, (0,))
    assert np.array_equal(one[:, :, 0], nine[:, :, 2]), "the prompt does not depend on the other taps"


@pytest.mark.parametrize("B", [32, 48, 64, 128, 256, 512, 1024, 1920, 4080])
def test_every_reduction_width_and_two_tiles(dev, cap, d_codes, B):
    """A block's B / 16 threads add up in groups of the largest power of two that divides them: 2, 1 (48), 4, 8, 16,
    32, 64, 8 (1920) and 1 (4080: 255 threads, one group each); the range reaches into a second tile."""
    raw, codes, channels = cr.parity_capture(), cr.parity_codes(), cr.parity_channels(4, seed=B)
    n = (4096 // B) * B + B + 5
    compare(dev, cap, raw, 1, n, B, d_codes, codes, channels, (0, -1, 1))


# ------------------------------------------------------------------------------------------------ 2. extremes
def test_saturated_captures_do_not_wrap(dev):
    """All-ones code row, a still carrier at every table index: bytes 0 are I = Q = -128 and reach -24 117 248, the
    header's bound, at index 14; bytes 255 and bytes alternating 0 / 255 against the closed forms and the restatement."""
    ones = np.ones((1, 1023), np.int16)
    channels = [(0, 0, i << 28, 0, 0, 0) for i in range(16)]
    n = 4096
    with dev.alloc(ones.nbytes) as d_ones:
        d_ones.upload(ones)
        for name, raw, (I, Q) in (("0", np.zeros(2 * n, np.uint8), (-128, -128)), ("255", np.full(2 * n, 255, np.uint8), (127, 127)),
                                  ("0/255", np.tile(np.array([0, 255], np.uint8), n), (-128, 127))):
            with dev.capture(raw) as c:
                got = compare(dev, c, raw, 0, n, 4096, d_ones, ones, channels, (0, 64, -64))
            want = [[(cr.COS[i] * I - cr.SIN[i] * Q) * n, (cr.SIN[i] * I + cr.COS[i] * Q) * n] for i in range(16)]
            for j in range(3):
                assert got[:, 0, j].tolist() == want, name
        raw = np.zeros(2 * n, np.uint8)
        with dev.capture(raw) as c:
            assert run(dev, c, 0, n, 4096, d_ones, 1, [channels[14]], (0,))[0, 0, 0, 0] == -cr.RECORD_BOUND


def test_one_long_range(dev):
    """2^24 + 4099 samples, one channel, one tap: the 64-bit code phase and the wrapping carrier far from t = 0."""
    n = 2 ** 24 + 4099
    raw = np.random.default_rng(99).integers(0, 256, 2 * (n + 1), dtype=np.uint8)
    codes = cr.parity_codes()
    ch = postcorr.channel(1, 1022.9999, -3400.0, cr.FS, 0.77)
    channels = [(cr.PERIOD - 1, ch.code_step - 3, ch.carr_phase, ch.carr_step, 1, 0)]
    want = cr.bank(raw, 1, n, 4096, codes, channels, (-1,))
    with dev.capture(raw) as c, dev.alloc(codes.nbytes) as d_rows:
        d_rows.upload(codes)
        got = run(dev, c, 1, n, 4096, d_rows, 4, channels, (-1,))
    np.testing.assert_array_equal(got.astype(np.int64), want)
    assert got.shape == (1, 4098, 1, 2) and got[0, -1].any()


# ------------------------------------------------------------------------------------------------ 3. refusals
def test_refusals_enqueue_nothing(dev, cap, d_codes):
    raw, codes, channels = cr.parity_capture(), cr.parity_codes(), cr.parity_channels(3)
    rec = np.array(channels, gpsjam.CORR_CHANNEL_DTYPE)
    n, B, T = 3 * 2048, 2048, (0, -1, 1)
    size = 8 * 3 * 3 * 3
    out, d_ch = Guarded(dev, size), dev.alloc(rec.nbytes + 8)
    try:
        d_ch.upload(rec)
        I, U = GJ_ERR_INVALID, GJ_ERR_UNSUPPORTED
        cases = [  # d_iq, nbytes, first, n, B, d_codes, rows, d_channels, n_channels, taps, d_out, status
            (0, cap.nbytes, 0, n, B, d_codes, 4, d_ch, 3, T, out, I),                              # null d_iq
            (cap, cap.nbytes, 0, n, B, 0, 4, d_ch, 3, T, out, I),                                  # null d_codes
            (cap, cap.nbytes, 0, n, B, d_codes, 4, 0, 3, T, out, I),                               # null d_channels
            (cap, cap.nbytes, 0, n, B, d_codes, 4, d_ch, 3, T, 0, I),                              # null d_out
            (cap.ptr + 1, cap.nbytes - 2, 0, n, B, d_codes, 4, d_ch, 3, T, out, I),                # odd d_iq
            (cap, cap.nbytes, 0, n, B, d_codes.ptr + 1, 3, d_ch, 3, T, out, I),                    # odd d_codes
            (cap, cap.nbytes, 0, n, B, d_codes, 4, d_ch.ptr + 4, 3, T, out, I),                    # d_channels not 8-byte aligned
            (cap, cap.nbytes, 0, n, B, d_codes, 4, d_ch, 3, T, out.ptr + 2, I),                    # d_out not 4-byte aligned
            (cap, cap.nbytes, 0, n, B, d_codes, 0, d_ch, 3, T, out, I),                            # no code rows
            (cap, cap.nbytes, cap.nsamples - n + 1, n, B, d_codes, 4, d_ch, 3, T, out, I),         # a range past the capture
            (cap, cap.nbytes, cap.nsamples + 1, 1, B, d_codes, 4, d_ch, 3, T, out, I),
            (cap, cap.nbytes, 2 ** 64 - 16, 32, B, d_codes, 4, d_ch, 3, T, out, I),                # first + n wraps
            (cap, cap.nbytes, 0, n, 0, d_codes, 4, d_ch, 3, T, out, U),                            # block_samples
            (cap, cap.nbytes, 0, n, 24, d_codes, 4, d_ch, 3, T, out, U),
            (cap, cap.nbytes, 0, n, 4112, d_codes, 4, d_ch, 3, T, out, U),
            (cap, cap.nbytes, 0, n, -2048, d_codes, 4, d_ch, 3, T, out, U),
            (cap, cap.nbytes, 0, n, B, d_codes, 4, d_ch, 3, (), out, U),                           # n_taps
            (cap, cap.nbytes, 0, n, B, d_codes, 4, d_ch, 3, tuple(range(10)), out, U),
            (cap, cap.nbytes, 0, n, B, d_codes, 4, d_ch, 3, (0, 65), out, U),                      # a tap offset
            (cap, cap.nbytes, 0, n, B, d_codes, 4, d_ch, 3, (-65,), out, U),
            (cap, cap.nbytes, 0, n, B, d_codes, 4, d_ch, 0, T, out, U),                            # n_channels
            (cap, cap.nbytes, 0, n, B, d_codes, 4, d_ch, 65, T, out, U),
            (cap, cap.nbytes, 0, 0, B, d_codes, 4, d_ch, 3, T, out, U),                            # n_samples
            (cap, 2 ** 40, 0, 2 ** 28 + 1, B, d_codes, 4, d_ch, 3, T, out, U),
        ]
        for c in cases:                                      # nothing written behind each one of them
            refused(dev, dev.corr_bank_dev, [(c[:-1], c[-1])], out)
        # channel fields live in device memory: the library cannot refuse them with a status, so the launch writes nothing
        bad = [(0, 1, 0, 0, 0, 1), (0, 1, 0, 0, 4, 0), (0, 1, 0, 0, -1, 0), (cr.PERIOD, 1, 0, 0, 0, 0), (0, 2 ** 34, 0, 0, 0, 0)]
        for ch in bad:
            for at in (0, 2):
                table = list(channels)
                table[at] = ch
                d_ch.upload(np.array(table, gpsjam.CORR_CHANNEL_DTYPE))
                dev.corr_bank_dev(cap, cap.nbytes, 0, n, B, d_codes, 4, d_ch, 3, T, out)
                dev.synchronize()
                out.check_untouched(f"channel {ch} at {at}")
            # ... and the wrapper checks them on the host, before anything is uploaded
            with pytest.raises(gpsjam.GpsJamError) as e:
                dev.corr_bank(cap, channels[:2] + [ch], codes)
            assert e.value.status == GJ_ERR_INVALID and cap.ptr
        # accepted: the limits themselves
        d_ch.upload(rec)
        dev.corr_bank_dev(cap, cap.nbytes, cap.nsamples - 1, 1, 4096, d_codes, 4, d_ch, 1, (64,), out)
        dev.corr_bank_dev(cap, cap.nbytes, 0, 16, 16, d_codes, 4, d_ch, 1, (-64,), out)
        dev.synchronize()
        out.check_pads("records")
    finally:
        freed(out, d_ch)
    # the next valid call gives the parity bits, and a library refusal through the wrapper raises and leaves the capture alone
    compare(dev, cap, raw, 7, n + 5, B, d_codes, codes, channels, T)
    with pytest.raises(gpsjam.GpsJamError) as e:
        dev.corr_bank(cap, channels, codes, block_samples=24)
    assert e.value.status == GJ_ERR_UNSUPPORTED and cap.ptr


def test_device_corr_bank_is_the_restatement(dev, cap):
    raw, codes, channels = cr.parity_capture(), cr.parity_codes(), cr.parity_channels(5)
    uploads, calls = gpsjam.Capture.uploads, dev.kernel_calls.get("corr_bank", 0)
    got = dev.corr_bank(cap, channels, codes, first_sample=3, n_samples=5000)
    assert gpsjam.Capture.uploads == uploads and dev.kernel_calls["corr_bank"] == calls + 1
    assert got.taps == (0, -1, 1) and got.block_samples == 2048 and got.n_samples == 5000
    assert np.array_equal(got.iq, cr.bank(raw, 3, 5000, 2048, codes, channels, (0, -1, 1)))
    host = dev.corr_bank(raw, channels, codes, first_sample=3, n_samples=5000)
    assert host.iq.tobytes() == got.iq.tobytes()


# ------------------------------------------------------------------------------------------------ 4. end to end
@pytest.fixture(scope="module")
def search(dev):
    s = gnss.AcqSearch(dev, prns=sorted(cr.E2E_PRNS + (1,)))         # PRN 1 is in no pair
    yield s
    s.close()


@pytest.mark.parametrize("kind", list(cr.E2E_KINDS))
def test_end_to_end_pairs(dev, search, kind):
    """100 ms pairs of the restatement's generator through the real acquisition, the bank and the host chain: every
    PRN's phase, Doppler and C/N0 within twice the CPU chain's error of the truth, and the verdict of its kind."""
    idx, phases = cr.E2E_KINDS[kind]
    raw_a, raw_b = cr.e2e_pair(kind)
    with dev.capture(raw_a) as a, dev.capture(raw_b) as b:
        uploads = gpsjam.Capture.uploads
        report = spoof.scan(dev, a, b, search, tol=cr.E2E_TOL)
        obs = postcorr.observe(dev, a, search)
        assert gpsjam.Capture.uploads == uploads
    assert report.prns == sorted(cr.E2E_PRNS[k] for k in idx) == [o.prn for o in obs]
    truth = {cr.E2E_PRNS[k]: (k, psi) for k, psi in zip(idx, phases)}
    for o, got, co in zip(obs, report.phase, report.coherence):
        k, psi = truth[o.prn]
        e_ph, e_dop, e_cn0 = abs(float(cr.wrap(got - psi))), abs(o.doppler_hz - cr.E2E_DOPPLER[k]), abs(o.cn0_dbhz - cr.E2E_CN0[k])
        print(f"{kind} PRN {o.prn}: phase {got:+.4f} (error {e_ph:.4f}, tolerance {cr.E2E_TOL_PHASE}), Doppler error {e_dop:.3f} Hz "
              f"({cr.E2E_TOL_DOPPLER}), C/N0 {o.cn0_dbhz:.2f} (error {e_cn0:.2f} dB, {cr.E2E_TOL_CN0}), code shift "
              f"{o.code_shift_chips:+.3f} chip, coherence {co:.3f}")
        assert e_ph <= cr.E2E_TOL_PHASE, (o.prn, got, psi)
        assert e_dop <= cr.E2E_TOL_DOPPLER, (o.prn, o.doppler_hz)
        assert e_cn0 <= cr.E2E_TOL_CN0, (o.prn, o.cn0_dbhz)
    if kind == "authentic":
        assert report.spoofed is False and len(report.common_prns) < 4
    elif kind == "spoofed":
        assert report.spoofed is True and report.common_prns == report.prns
        assert report.p_chance == pytest.approx(5 * (cr.E2E_TOL / math.pi) ** 4)
    else:
        assert report.spoofed is True and report.common_prns == sorted(cr.E2E_MIXED_COMMON)
