"""The tracking loops on the GPU (gj_track_dev, Device.track) and what is built on them (gpsjam.track).

This file sits in a package of its own on purpose, as tests/corr/ does: the suite orders GPU files by basename
(tests/conftest.py SUITE_ORDER, which tests/test_suite_order.py holds every GPU file to), and under the name
test_round6_gpu.py it runs in stage 2.

Yardstick: the integer restatement of the definition in include/gpsjam.h (tests/track_restatement.py, which
tests/test_track_host.py holds to a per-sample Python-int loop).  Everything the kernel makes is integer arithmetic, so
EVERY record and EVERY state is equal, bit for bit.  Every call writes into sentinel-filled buffers whose 256 bytes
behind the call's records and states must stay untouched.  The float figures of the end-to-end test are held to twice the
error that tests/test_track_host.py measures on the CPU with the same host code on restated integers."""
import numpy as np
import pytest

import corr_restatement as cr
import gpsjam
import track_restatement as tr
from gpsjam import gnss, postcorr, track
from gpu_lib import GJ_ERR_INVALID, GJ_ERR_UNSUPPORTED, SENTINEL, Guarded, freed, refused
from gpu_lib import run_track as run
from gpu_lib import track_state_records as to_records

pytestmark = pytest.mark.gpu

EPOCH, STATE = gpsjam.TRACK_EPOCH_DTYPE, gpsjam.TRACK_STATE_DTYPE
G = tr.MAX_GAIN
WIDE = tr.gains(*tr.WIDE, 2048, cr.FS)          # (1, 1540, ...)
ZERO = (1, 0, 0, 0, 0, 0, 0)


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


def compare(dev, capture, raw, first, n, B, n_epochs, d_rows, codes, states, params):
    got, after = run(dev, capture, first, n, B, n_epochs, d_rows, len(codes), states, params)
    want, want_after = tr.track(raw, first, n, B, n_epochs, codes, states, params)
    what = f"first {first} n {n} B {B} epochs {n_epochs} channels {len(states)} params {params}"
    for k, rows in enumerate(want):
        if rows is None:
            assert np.all(got[k] == SENTINEL), f"a bad channel's records were written: channel {k}, {what}"
        else:
            np.testing.assert_array_equal(tr.epochs_as_array(got[k].view(EPOCH)), np.array(rows, np.int64), err_msg=f"channel {k}, {what}")
    assert after == want_after, what
    return got, after


def spread_states(n_channels, n, n_epochs, B, seed=0):
    """The parity channels at start 0, 1 and the start that ends on the range's last sample, in turn."""
    starts = (0, 1, n - n_epochs * B)
    return [tr.state(ch, starts[k % 3]) for k, ch in enumerate(cr.parity_channels(n_channels, seed))]


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("B", [16, 272, 1040, 2048, 4096])
def test_parity_with_the_restatement(dev, cap, d_codes, B):
    """One data thread, 17, 65 (one past a wave), half the workgroup and all of it; an odd first sample; the six edge
    channels: code phase 1023 2^32 - 1, code steps that wrap inside an epoch, carrier steps 0, 1, 0x80000000, 0xFFFFFFFF."""
    raw, codes = cr.parity_capture(), cr.parity_codes()
    n = cap.nsamples - 7
    for n_epochs in (1, 2, 3):
        compare(dev, cap, raw, 7, n, B, n_epochs, d_codes, codes, spread_states(6, n, n_epochs, B), WIDE)


def test_many_epochs_of_one_thread(dev, cap, d_codes):
    raw, codes = cr.parity_capture(), cr.parity_codes()
    n = 97 * 16 + 1
    compare(dev, cap, raw, 1, n, 16, 97, d_codes, codes, spread_states(6, n, 97, 16), WIDE)
    compare(dev, cap, raw, cap.nsamples - n, n, 16, 97, d_codes, codes, spread_states(6, n, 97, 16), (2, 1, G, -G, G, -G, G))


@pytest.mark.parametrize("spacing", [1, 8, 9, 64])
def test_spacings_aiding_and_gains(dev, cap, d_codes, spacing):
    """Both chip paths at their edges (one window up to 8, three from 9), every aid_div and every set of gains, at start 0."""
    raw, codes = cr.parity_capture(), cr.parity_codes()
    states = [tr.state(ch) for ch in cr.parity_channels(6, seed=spacing)]
    for aid_div in (0, 1, 1540):
        for gains in ((0, 0, 0, 0, 0), WIDE[2:], (G, G, G, G, G), (-G, -G, -G, -G, -G)):
            compare(dev, cap, raw, 3, 4 * 272, 272, 4, d_codes, codes, states, (spacing, aid_div) + tuple(gains))


@pytest.mark.parametrize("n_channels", [1, 3, 300])
def test_channel_counts(dev, cap, d_codes, n_channels):
    """300: more workgroups than compute units; channels 1 and 2 share a code row."""
    raw, codes = cr.parity_capture(), cr.parity_codes()
    n = cap.nsamples - 1
    states = spread_states(n_channels, n, 3, 2048, seed=n_channels)
    got, after = compare(dev, cap, raw, 1, n, 2048, 3, d_codes, codes, states, WIDE)
    again, after2 = run(dev, cap, 1, n, 2048, 3, d_codes, 4, states, WIDE)
    assert got.tobytes() == again.tobytes() and after == after2, "two calls, identical bits"


# ------------------------------------------------------------------------------------------------ 2. extremes
def test_extreme_captures(dev):
    """All 128: every sum is 0 and the degenerate rules hold (angle 0, c = 0, nothing moves).  Bytes 0 with a row of ones
    and a still carrier at table index 14: the record bound; bytes 0 / 255 in turn."""
    ones = np.ones((1, 1023), np.int16)
    n = 2 * 4096
    states = [tr.state((0, 0, i << 28, 0, 0, 0)) for i in range(16)]
    with dev.alloc(ones.nbytes) as d_ones:
        d_ones.upload(ones)
        for name, raw in (("128", np.full(2 * n, 128, np.uint8)), ("0", np.zeros(2 * n, np.uint8)),
                          ("0/255", np.tile(np.array([0, 255], np.uint8), n))):
            with dev.capture(raw) as c:
                for params in (WIDE, (64, 1, G, G, G, G, G)):
                    got, after = compare(dev, c, raw, 0, n, 4096, 2, d_ones, ones, states, params)
                    rec = tr.epochs_as_array(got.view(EPOCH))
                    if name == "128":
                        assert not rec[..., :6].any() and not rec[..., 10:].any() and [s[:6] for s in after] == [s[:6] for s in states], name
                    if name == "0":
                        assert rec[14, 0, 0] == rec[14, 0, 2] == rec[14, 0, 4] == -cr.RECORD_BOUND


# ------------------------------------------------------------------------------------------------ 3. the header's consequences
@pytest.mark.parametrize("d", [1, 64])
def test_zero_gains_are_the_bank(dev, cap, d_codes, d):
    raw, codes, channels = cr.parity_capture(), cr.parity_codes(), cr.parity_channels(6)
    B, n_epochs = 2048, 6
    got, _ = compare(dev, cap, raw, 7, n_epochs * B, B, n_epochs, d_codes, codes, [tr.state(ch) for ch in channels], (d, 0, 0, 0, 0, 0, 0))
    bank = dev.corr_bank(cap, channels, codes, 7, n_epochs * B, B, (d, 0, -d))
    rec = got.view(EPOCH)
    mine = np.stack([rec["early"], rec["prompt"], rec["late"]], axis=2)
    assert mine.tobytes() == bank.iq.tobytes()


def test_n_plus_m_epochs_are_n_then_m(dev, cap, d_codes):
    raw, codes = cr.parity_capture(), cr.parity_codes()
    B, N, M, n = 1040, 4, 7, cap.nsamples - 5
    states = spread_states(6, n, N + M, B)
    whole, after = compare(dev, cap, raw, 5, n, B, N + M, d_codes, codes, states, WIDE)
    first, mid = run(dev, cap, 5, n, B, N, d_codes, 4, states, WIDE)
    second, end = run(dev, cap, 5, n, B, M, d_codes, 4, mid, WIDE)
    assert np.concatenate([first, second], axis=1).tobytes() == whole.tobytes() and end == after


# ------------------------------------------------------------------------------------------------ 4. bad channels, refusals
def test_bad_channels_write_nothing(dev, cap, d_codes):
    raw, codes = cr.parity_capture(), cr.parity_codes()
    n, B, n_epochs = 3 * 2048 + 9, 2048, 3
    good = spread_states(5, n, n_epochs, B)
    for bad in tr.bad_states(good[2], 4, n_epochs, B, n):
        for at in (0, 2, 4):
            states = list(good)
            states[at] = bad
            got, after = compare(dev, cap, raw, 3, n, B, n_epochs, d_codes, codes, states, WIDE)
            assert np.all(got[at] == SENTINEL) and after[at] == bad
        # ... and the wrapper checks them on the host, before anything is uploaded or launched
        calls = dev.kernel_calls.get("track", 0)
        with pytest.raises(gpsjam.GpsJamError) as e:
            dev.track(cap, good[:2] + [bad], codes, WIDE, 3, n, B, n_epochs)
        assert e.value.status == GJ_ERR_INVALID and cap.ptr and dev.kernel_calls.get("track", 0) == calls, bad


def test_refusals_enqueue_nothing(dev, cap, d_codes):
    raw, codes = cr.parity_capture(), cr.parity_codes()
    n, B, E = 3 * 2048, 2048, 3
    states = spread_states(3, n, E, B)
    rec = to_records(states)
    size = EPOCH.itemsize * 3 * E
    out, d_st = Guarded(dev, size), dev.alloc(rec.nbytes + 8)
    P = WIDE

    def with_(at, v):
        return P[:at] + (v,) + P[at + 1:]

    try:
        d_st.upload(np.concatenate([rec.view(np.uint8), np.zeros(8, np.uint8)]))
        I, U = GJ_ERR_INVALID, GJ_ERR_UNSUPPORTED
        reserved = gpsjam.TrackParams(*P, 1)
        cases = [  # d_iq, nbytes, first, n, B, n_epochs, d_codes, rows, d_states, n_channels, params, d_out, status
            (0, cap.nbytes, 0, n, B, E, d_codes, 4, d_st, 3, P, out, I),                           # null d_iq
            (cap, cap.nbytes, 0, n, B, E, 0, 4, d_st, 3, P, out, I),                               # null d_codes
            (cap, cap.nbytes, 0, n, B, E, d_codes, 4, 0, 3, P, out, I),                            # null d_states
            (cap, cap.nbytes, 0, n, B, E, d_codes, 4, d_st, 3, P, 0, I),                           # null d_out
            (cap.ptr + 1, cap.nbytes - 2, 0, n, B, E, d_codes, 4, d_st, 3, P, out, I),             # odd d_iq
            (cap, cap.nbytes, 0, n, B, E, d_codes.ptr + 1, 3, d_st, 3, P, out, I),                 # odd d_codes
            (cap, cap.nbytes, 0, n, B, E, d_codes, 4, d_st.ptr + 4, 3, P, out, I),                 # d_states not 8-byte aligned
            (cap, cap.nbytes, 0, n, B, E, d_codes, 4, d_st, 3, P, out.ptr + 4, I),                 # d_out not 8-byte aligned
            (cap, cap.nbytes, 0, n, B, E, d_codes, 0, d_st, 3, P, out, I),                         # no code rows
            (cap, cap.nbytes, 0, n, B, E, d_codes, 4, d_st, 3, reserved, out, I),                  # params.reserved
            (cap, cap.nbytes, 0, n - 1, B, E, d_codes, 4, d_st, 3, P, out, I),                     # n_epochs B > n_samples
            (cap, cap.nbytes, 0, 4095, 4096, 1, d_codes, 4, d_st, 3, P, out, I),
            (cap, cap.nbytes, cap.nsamples - n + 1, n, B, E, d_codes, 4, d_st, 3, P, out, I),      # a range past the capture
            (cap, cap.nbytes, cap.nsamples + 1, 16, 16, 1, d_codes, 4, d_st, 3, P, out, I),
            (cap, cap.nbytes, 2 ** 64 - 16, 32, 16, 1, d_codes, 4, d_st, 3, P, out, I),            # first + n wraps
            (cap, cap.nbytes, 0, n, 0, E, d_codes, 4, d_st, 3, P, out, U),                         # block_samples
            (cap, cap.nbytes, 0, n, 24, E, d_codes, 4, d_st, 3, P, out, U),
            (cap, cap.nbytes, 0, n, 4112, 1, d_codes, 4, d_st, 3, P, out, U),
            (cap, cap.nbytes, 0, n, -2048, E, d_codes, 4, d_st, 3, P, out, U),
            (cap, cap.nbytes, 0, n, B, 0, d_codes, 4, d_st, 3, P, out, U),                         # n_epochs
            (cap, cap.nbytes, 0, n, B, -1, d_codes, 4, d_st, 3, P, out, U),
            (cap, cap.nbytes, 0, n, 16, tr.MAX_EPOCHS + 1, d_codes, 4, d_st, 3, P, out, U),
            (cap, cap.nbytes, 0, n, B, E, d_codes, 4, d_st, 0, P, out, U),                         # n_channels
            (cap, cap.nbytes, 0, n, B, E, d_codes, 4, d_st, tr.MAX_CHANNELS + 1, P, out, U),
            (cap, cap.nbytes, 0, 0, B, E, d_codes, 4, d_st, 3, P, out, U),                         # n_samples
            (cap, 2 ** 40, 0, 2 ** 28 + 1, B, E, d_codes, 4, d_st, 3, P, out, U),
            (cap, cap.nbytes, 0, n, B, E, d_codes, 4, d_st, 3, with_(0, 0), out, U),               # spacing
            (cap, cap.nbytes, 0, n, B, E, d_codes, 4, d_st, 3, with_(0, 65), out, U),
            (cap, cap.nbytes, 0, n, B, E, d_codes, 4, d_st, 3, with_(0, -1), out, U),
            (cap, cap.nbytes, 0, n, B, E, d_codes, 4, d_st, 3, with_(1, -1), out, U),              # aid_div
        ]
        for at in range(2, 7):                                                                     # a gain beyond +-2^30
            cases.append((cap, cap.nbytes, 0, n, B, E, d_codes, 4, d_st, 3, with_(at, G + 1), out, U))
            cases.append((cap, cap.nbytes, 0, n, B, E, d_codes, 4, d_st, 3, with_(at, -G - 1), out, U))
        for c in cases:                                      # nothing written behind each one of them, the states as they were
            refused(dev, dev.track_dev, [(c[:-1], c[-1])], out)
            assert d_st.download(np.uint8, rec.nbytes).tobytes() == rec.tobytes(), c[2:8]
        # accepted: the limits themselves
        dev.track_dev(cap, cap.nbytes, cap.nsamples - 16, 16, 16, 1, d_codes, 4, d_st, 1, (64, 0, G, -G, G, -G, G), out)
        d_st.upload(rec)
        dev.track_dev(cap, cap.nbytes, 0, 4096, 4096, 1, d_codes, 4, d_st, 1, (1, 2 ** 31 - 1, -G, G, -G, G, -G), out)
        dev.synchronize()
        out.check_pads("records")
    finally:
        freed(out, d_st)
    # the next valid call gives the parity bits, and a library refusal through the wrapper raises and leaves the capture alone
    compare(dev, cap, raw, 7, n + 5, B, E, d_codes, codes, states, P)
    with pytest.raises(gpsjam.GpsJamError) as e:
        dev.track(cap, states, codes, P, block_samples=24, n_epochs=1)
    assert e.value.status == GJ_ERR_UNSUPPORTED and cap.ptr


def test_device_track_is_the_restatement(dev, cap):
    raw, codes = cr.parity_capture(), cr.parity_codes()
    states = spread_states(5, 5000, 2, 2048)
    uploads, calls = gpsjam.Capture.uploads, dev.kernel_calls.get("track", 0)
    rec, after = dev.track(cap, states, codes, WIDE, first_sample=3, n_samples=5000)
    assert gpsjam.Capture.uploads == uploads and dev.kernel_calls["track"] == calls + 1
    want, want_after = tr.track(raw, 3, 5000, 2048, 2, codes, states, WIDE)
    assert rec.shape == (5, 2) and rec.dtype == EPOCH and after.dtype == STATE
    np.testing.assert_array_equal(tr.epochs_as_array(rec), tr.as_array(want))
    assert tr.states_as_tuples(after) == want_after
    host, host_after = dev.track(raw, to_records(states), codes, track.gains(*track.WIDE, 2048, cr.FS), first_sample=3, n_samples=5000,
                                 n_epochs=2)
    assert host.tobytes() == rec.tobytes() and host_after.tobytes() == after.tobytes()


# ------------------------------------------------------------------------------------------------ 5. end to end
def test_the_loop_capture_bit_for_bit(dev):
    """The host test's capture, states and schedule through Device.track: every record and the last state."""
    want, want_after = tr.loop_track()
    states, pieces = [tr.state(tr.loop_channel(), tr.LOOP_START)], []
    with dev.capture(tr.loop_capture()) as c:
        for n_epochs, params in tr.loop_schedule():
            rec, states = dev.track(c, states, tr.loop_codes(), params, 0, tr.LOOP_SAMPLES, tr.LOOP_B, n_epochs)
            pieces.append(rec)
    np.testing.assert_array_equal(tr.epochs_as_array(np.concatenate(pieces, axis=1)[0]), want)
    assert tr.states_as_tuples(states) == [want_after]


def test_command_line_prints_a_line_per_prn_and_second(tmp_path, capsys):
    path = tmp_path / "loop.bin"
    tr.loop_capture().tofile(path)
    assert track.main([str(path), "--pull-in", str(tr.LOOP_PULL_IN)]) == 0
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith(f"PRN {tr.LOOP_PRN:2d} ")]
    assert len(lines) == 1 and "Doppler" in lines[0] and "C/N0" in lines[0], lines       # 0.6 s: one window
    assert float(lines[0].split("lock")[1]) > 0.9, lines


def test_follow_with_the_real_acquisition(dev):
    """gpsjam.track.follow on the same bytes: the chain differs from the CPU's only in the acquisition's cell, so it is
    allowed twice the recorded CPU errors, and it must beat the open loop at the acquisition's own channel."""
    search = gnss.AcqSearch(dev, prns=[1, tr.LOOP_PRN])
    try:
        with dev.capture(tr.loop_capture()) as c:
            uploads = gpsjam.Capture.uploads
            tracks = track.follow(dev, c, search, pull_in=tr.LOOP_PULL_IN)
            assert gpsjam.Capture.uploads == uploads
            assert [t.prn for t in tracks] == [tr.LOOP_PRN]
            t = tracks[0]
            first = t.records[0]
            channel = (int(first["code_phase"]), int(first["code_step"]), int(first["carr_phase"]), int(first["carr_step"]), 0, 0)
            bank = dev.corr_bank(c, [channel], tr.loop_codes(), t.start, t.prompts.size * tr.LOOP_B, tr.LOOP_B, (0,))
    finally:
        search.close()
    assert t.prompts.size >= tr.LOOP_EPOCHS and abs(t.start - tr.LOOP_START) <= 1 and abs(t.doppler_hz[0] - tr.LOOP_GRID_DOPPLER) <= 200.0
    rms, lock, cn0 = tr.loop_figures(tr.epochs_as_array(t.records))
    open_cn0 = postcorr.cn0(bank.tap(0)[0][-tr.LOOP_WINDOW:], tr.LOOP_B / cr.FS)
    print(f"follow: start {t.start}, first Doppler {t.doppler_hz[0]:.1f} Hz, Doppler rms error {rms:.3f} Hz (allowed {2 * tr.LOOP_CPU_DOPPLER_RMS}), "
          f"lock {lock:.4f} (at least {1 - 2 * (1 - tr.LOOP_CPU_LOCK):.3f}), tracked C/N0 {cn0:.2f} dB-Hz (within "
          f"{2 * (tr.LOOP_CN0 - tr.LOOP_CPU_CN0_TRACKED):.2f} dB of {tr.LOOP_CN0}), open-loop C/N0 {open_cn0:.2f} dB-Hz")
    assert rms <= 2.0 * tr.LOOP_CPU_DOPPLER_RMS
    assert 1.0 - lock <= 2.0 * (1.0 - tr.LOOP_CPU_LOCK)
    assert abs(cn0 - tr.LOOP_CN0) <= 2.0 * abs(tr.LOOP_CN0 - tr.LOOP_CPU_CN0_TRACKED)
    assert cn0 > open_cn0
    assert t.lock.size == t.cn0_dbhz.size == 1 and t.bits.size == t.prompts.size and set(np.unique(t.bits)) <= {-1, 1}
