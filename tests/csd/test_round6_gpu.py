"""Cross-spectral density and coherence of a capture pair (gj_csd_dev, Device.cross_spectrum, gpsjam.coherence) on the GPU.

This file sits in a package of its own on purpose, as tests/skurt/ does: the suite orders GPU files by basename
(tests/conftest.py SUITE_ORDER, which tests/test_suite_order.py holds every GPU file to), and under the name
test_round6_gpu.py it runs in stage 2, behind the parity tests of K2 whose transform it shares.

Yardstick: the float64 restatement of the definition in include/gpsjam.h (tests/csd_restatement.py).
  Saa, Sbb: within 1e-5 (sr.S1_TOL, the project's tolerance for these very sums in gj_sk_dev) of the row's largest
            reference value;
  Sab:      re and im within 1e-5 * sqrt(max_k Saa * max_k Sbb) of the row: every term is bounded by |A| |B| and carries
            the same rounding as a term of Saa or Sbb;
  d_msc:    within 2 float32 ulps of the formula in float64 on the downloaded Saa, Sbb and Sab, NaN exactly where
            Saa * Sbb == 0.
Translation, fewer rows, d_msc = NULL, repetition and another partner capture are bit-exact.  Every call writes into
sentinel-filled buffers whose bytes behind the asked-for output must stay untouched."""
import os
import sys

import numpy as np
import pytest

SKRYPTY = os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "gps-jamming_amd", "skrypty")
if SKRYPTY not in sys.path:
    sys.path.append(SKRYPTY)

import csd_restatement as cs
import gpsjam
import skurt_restatement as sr
from gpsjam import coherence
from gpu_lib import GJ_ERR_INVALID, GJ_ERR_UNSUPPORTED, PAD, SENTINEL, Guarded, freed, refused, run_sk
from gpu_lib import run_csd as run

pytestmark = pytest.mark.gpu

FA, FB = cs.PARITY_FIRST_A, cs.PARITY_FIRST_B   # 1 and 4


@pytest.fixture(scope="module")
def pair(dev):
    a, b = (dev.capture(r) for r in cs.parity_pair())
    yield a, b
    a.free()
    b.free()


def run_pair(dev, pair, nfft, hop, m, n_rows, first_a=FA, first_b=FB, want_msc=True):
    a, b = pair
    return run(dev, a, a.nbytes, first_a, b, b.nbytes, first_b, nfft, hop, m, n_rows, want_msc)


def same(x, y):
    return all((p is None and q is None) or p.tobytes() == q.tobytes() for p, q in zip(x, y))


def report(head):
    print(f"{head}: largest errors so far Saa {cs.worst['saa']:.2e}, Sbb {cs.worst['sbb']:.2e}, Sab {cs.worst['sab']:.2e} (tolerance {cs.S1_TOL:.0e}), "
          f"MSC {cs.worst['msc_ulp']:.2f} ulp (tolerance 2)")


@pytest.mark.parametrize("nfft", cs.NFFT)
def test_parity_with_the_restatement(dev, pair, nfft):
    try:
        for offset, scale in ((127.5, 1.0 / 127.5), (128.0, 1.0 / 128.0)):
            dev.set_unpack(offset, scale)
            for hop in cs.parity_hops(nfft):
                sa, sb = cs.parity_spectra(nfft, hop, FA, FB, offset)
                for m in cs.PARITY_M:
                    n_rows = gpsjam.csd_rows(pair[0].nbytes, FA, pair[1].nbytes, FB, nfft, hop, m)
                    assert n_rows == sa.shape[0] // m >= 1
                    cs.compare(run_pair(dev, pair, nfft, hop, m, n_rows), cs.sums_of(sa, sb, m, n_rows, scale), (nfft, hop, m, offset))
    finally:
        dev.set_unpack()
    assert dev.get_unpack() == (127.5, 1.0 / 127.5)
    report(f"nfft {nfft}")


@pytest.mark.parametrize("nfft", cs.BOUNDARY_NFFT)      # a group inside a wave, a whole wave, the whole workgroup
def test_block_boundaries(dev, pair, nfft):
    """Rows of 1, 2, 3, ... blocks, with a full and with a short last block (blocks hold at most MAX_RUN = 16 pairs)."""
    hop = cs.BOUNDARY_HOP
    sa, sb = cs.parity_spectra(nfft, hop)
    for m in cs.BOUNDARY_M:
        for n_rows in (1, 3):
            assert n_rows <= gpsjam.csd_rows(pair[0].nbytes, FA, pair[1].nbytes, FB, nfft, hop, m)
            cs.compare(run_pair(dev, pair, nfft, hop, m, n_rows), cs.sums_of(sa, sb, m, n_rows), (nfft, m, n_rows))
    report(f"nfft {nfft}")


def test_workgroups_that_take_more_than_one_step(dev):
    """nfft 16, hop 1, M 2 on 2^19 samples: one block per row, 256 blocks per workgroup step, 1024 steps -- more than one
    round of workgroups (two per CU at 16 points)."""
    a, b = (r[:2 << 19] for r in cs.detect_pair("two"))
    n_rows = gpsjam.csd_rows(a.size, FA, b.size, FB, 16, 1, 2)
    assert n_rows == ((1 << 19) - FB - 16 + 1) // 2
    nsteps, cus = -(-n_rows // 256), dev.info()["compute_units"]
    assert nsteps > 2 * cus, f"{nsteps} steps are sized for 256 CUs with two workgroups each, this device has {cus}"
    with dev.capture(a) as ca, dev.capture(b) as cb:
        got = run(dev, ca, ca.nbytes, FA, cb, cb.nbytes, FB, 16, 1, 2, n_rows)
    cs.compare(got, cs.csd(a, b, 16, 1, 2, FA, FB, n_rows), "M 2 on 2^19 samples")
    report(f"{nsteps} steps")


@pytest.mark.parametrize("nfft", cs.BOUNDARY_NFFT)
def test_bit_exact_behaviour(dev, pair, nfft):
    hop, m = 101, 18                                      # two blocks of 9 pairs
    n = gpsjam.csd_rows(pair[0].nbytes, 3, pair[1].nbytes, 6, nfft, hop, m)
    assert n >= 12
    base = run_pair(dev, pair, nfft, hop, m, n, 3, 6)
    assert same(run_pair(dev, pair, nfft, hop, m, n, 3, 6), base), "two identical calls"
    for k in (1, 2, 7):                                   # started k rows later in both: the same rows, bit for bit
        later = run_pair(dev, pair, nfft, hop, m, n - k, 3 + k * m * hop, 6 + k * m * hop)
        assert all(x.tobytes() == y[k:].tobytes() for x, y in zip(later, base)), (nfft, k)
    third = run_pair(dev, pair, nfft, hop, m, n // 3, 3, 6)              # fewer rows: another grid, the same bits
    assert all(x.tobytes() == y[:n // 3].tobytes() for x, y in zip(third, base))
    no_msc = run_pair(dev, pair, nfft, hop, m, n, 3, 6, want_msc=False)
    assert no_msc[3] is None and same(no_msc[:3], base[:3]), "d_msc = NULL changes no other bit"
    # another partner: Saa depends on a's bytes alone, Sbb on b's
    a, b = pair
    aa = run(dev, a, a.nbytes, 3, a, a.nbytes, 6, nfft, hop, m, n)       # b := a at another start (d_a == d_b, overlapping)
    assert aa[0].tobytes() == base[0].tobytes(), "Saa is unchanged under a different b"
    bb = run(dev, b, b.nbytes, 3, b, b.nbytes, 6, nfft, hop, m, n)
    assert bb[1].tobytes() == base[1].tobytes(), "Sbb is unchanged under a different a"
    assert aa[2].tobytes() != base[2].tobytes()
    # one capture against itself at the same start: Sab = Saa exactly, no imaginary part, MSC = 1
    one = run(dev, a, a.nbytes, 3, a, a.nbytes, 3, nfft, hop, m, n)
    assert one[0].tobytes() == base[0].tobytes() == one[1].tobytes() and not one[2].imag.any()
    assert np.array_equal(one[2].real, one[0]) and np.all(one[3] == 1.0)
    # the pair swapped: the auto-spectra exchanged, Sab conjugated, MSC the same, all bit for bit
    swapped = run(dev, b, b.nbytes, 6, a, a.nbytes, 3, nfft, hop, m, n)
    assert swapped[0].tobytes() == base[1].tobytes() and swapped[1].tobytes() == base[0].tobytes()
    assert np.array_equal(swapped[2], np.conj(base[2])) and swapped[3].tobytes() == base[3].tobytes()


@pytest.mark.parametrize("nfft", cs.NFFT)
def test_saa_against_the_kurtosis_s1(dev, pair, nfft):
    a, _ = pair
    identical = True
    for hop in cs.parity_hops(nfft):
        for m in cs.PARITY_M:
            n_rows = gpsjam.csd_rows(pair[0].nbytes, FA, pair[1].nbytes, FB, nfft, hop, m)
            saa = run_pair(dev, pair, nfft, hop, m, n_rows)[0]
            s1 = run_sk(dev, a, a.nbytes, nfft, hop, FA, m, n_rows, want_sk=False)[0]
            err = float(np.max(np.abs(saa.astype(np.float64) - s1) / s1.max(axis=1, keepdims=True)))
            assert err <= cs.S1_TOL, (nfft, hop, m, err)
            identical &= saa.tobytes() == s1.tobytes()
    print(f"nfft {nfft}: Saa and gj_sk_dev's S1 of capture a are {'bit-identical' if identical else 'NOT bit-identical'} at every geometry tried")


def test_refusals_enqueue_nothing(dev, pair):
    a, b = pair
    fit = gpsjam.csd_rows(a.nbytes, 0, b.nbytes, 0, 256, 128, 16)
    cells = (fit + 1) * 256
    saa, sbb, sab, msc = Guarded(dev, 4 * cells), Guarded(dev, 4 * cells), Guarded(dev, 8 * cells), Guarded(dev, 4 * cells)
    outs = (saa, sbb, sab, msc)
    ok = (a, a.nbytes, 0, b, b.nbytes, 0, 256, 128, 16, 4)

    def geom(nfft=256, hop=128, m=16, n_rows=4, first_a=0, first_b=0):
        return (a, a.nbytes, first_a, b, b.nbytes, first_b, nfft, hop, m, n_rows)
    cases = [
        (*geom(nfft=8, hop=4), *outs, GJ_ERR_UNSUPPORTED),
        (*geom(nfft=8192, hop=4096, m=2, n_rows=1), *outs, GJ_ERR_UNSUPPORTED),
        (*geom(nfft=48, hop=24), *outs, GJ_ERR_UNSUPPORTED),
        (*geom(hop=0), *outs, GJ_ERR_INVALID),
        (*geom(m=1), *outs, GJ_ERR_INVALID),                                     # M below 2
        (*geom(m=0), *outs, GJ_ERR_INVALID),
        (*geom(m=-5), *outs, GJ_ERR_INVALID),
        (*geom(nfft=16, hop=1, m=65537, n_rows=1), *outs, GJ_ERR_UNSUPPORTED),   # M above 65536 (one such row fits)
        (*geom(n_rows=0), *outs, GJ_ERR_INVALID),                                # no row
        (*geom(n_rows=fit + 1), *outs, GJ_ERR_INVALID),                          # more than fit
        (*geom(n_rows=fit, first_b=2048), *outs, GJ_ERR_INVALID),                # ... b alone: the shorter of two decides
        (*geom(n_rows=fit, first_a=2048), *outs, GJ_ERR_INVALID),
        (*geom(n_rows=1, first_a=a.nsamples), *outs, GJ_ERR_INVALID),
        (*geom(n_rows=1, first_b=2 ** 64 - 8), *outs, GJ_ERR_INVALID),           # first_b + nfft wraps
        (a, a.nbytes, 0, b, 2 * 255, 0, 256, 128, 16, 1, *outs, GJ_ERR_INVALID), # b too short for one frame
        (0, *ok[1:], *outs, GJ_ERR_INVALID),                                     # null d_a, d_b
        (*ok[:3], 0, *ok[4:], *outs, GJ_ERR_INVALID),
        (a.ptr + 1, a.nbytes - 2, *ok[2:], *outs, GJ_ERR_INVALID),               # odd d_a, d_b
        (*ok[:3], b.ptr + 1, b.nbytes - 2, *ok[5:], *outs, GJ_ERR_INVALID),
        (*ok, 0, sbb, sab, msc, GJ_ERR_INVALID),                                 # null d_saa, d_sbb, d_sab
        (*ok, saa, 0, sab, msc, GJ_ERR_INVALID),
        (*ok, saa, sbb, 0, msc, GJ_ERR_INVALID),
        (*ok, saa.ptr + 2, sbb, sab, msc, GJ_ERR_INVALID),                       # misaligned outputs
        (*ok, saa, sbb.ptr + 1, sab, msc, GJ_ERR_INVALID),
        (*ok, saa, sbb, sab, msc.ptr + 2, GJ_ERR_INVALID),
        (*ok, saa, sbb, sab.ptr + 4, msc, GJ_ERR_INVALID),                       # d_sab: 8 bytes
        (*ok, saa, sbb, sab.ptr + 2, msc, GJ_ERR_INVALID),
    ]
    try:
        refused(dev, dev.cross_spectrum_dev, [(c[:-1], c[-1]) for c in cases], *outs)
        # accepted: M at its smallest, a call that just fits, no d_msc, d_saa only 4-byte aligned
        need = dev.csd_workspace(256, 16, fit)
        assert need == fit * 4 * 256 * 4
        dev.reserve(need)
        dev.cross_spectrum_dev(*geom(nfft=16, hop=8, m=2), saa.ptr + 4, sbb, sab, msc)
        dev.cross_spectrum_dev(*geom(n_rows=fit), saa, sbb, sab, None)
        dev.synchronize()
        size = 4 * fit * 256
        for buf, s in ((saa, size), (sbb, size), (sab, 2 * size)):
            assert np.all(buf.download(np.uint8, PAD, s) == SENTINEL)
            buf.check_pads("output")
    finally:
        freed(*outs)


def test_extremes(dev):
    """Saturated pairs: finite sums everywhere, MSC finite wherever both auto-spectra hold power (the definition's NaN
    is for Saa * Sbb == 0 alone) and 1 in the bins a constant fills, 0 and +-1 under the Hann window.  Silence: NaN."""
    n = 2 * 12000
    lo, hi = np.zeros(n, np.uint8), np.full(n, 255, np.uint8)
    for nfft in (16, 256, 4096):
        for ra, rb in ((lo, lo), (hi, hi), (lo, hi)):
            with dev.capture(ra) as ca, dev.capture(rb) as cb:
                rows = gpsjam.csd_rows(n, 1, n, 2, nfft, nfft // 4, 3)
                assert rows >= 1
                saa, sbb, sab, msc = run(dev, ca, n, 1, cb, n, 2, nfft, nfft // 4, 3, rows)
            assert np.isfinite(saa).all() and np.isfinite(sbb).all() and np.isfinite(sab.real).all() and np.isfinite(sab.imag).all()
            cs.check_msc(saa, sbb, sab, msc, (nfft, "saturated"))
            live = saa.astype(np.float64) * sbb.astype(np.float64) > 0
            assert np.isfinite(msc[live]).all() and live[:, [0, 1, -1]].all()
            np.testing.assert_allclose(msc[:, [0, 1, -1]], 1.0, rtol=1e-5)
            print(f"nfft {nfft}: {int(np.sum(~live))} of {live.size} cells without power in one of the two")
    try:
        dev.set_unpack(128.0, 1.0 / 128.0)
        flat = np.full(n, 128, np.uint8)
        with dev.capture(flat) as c:
            for nfft in (16, 256, 2048):
                rows = gpsjam.csd_rows(n, 1, n, 0, nfft, nfft // 2, 2)
                saa, sbb, sab, msc = run(dev, c, n, 1, c, n, 0, nfft, nfft // 2, 2, rows)
                assert rows >= 1 and not saa.any() and not sbb.any() and not sab.any() and np.isnan(msc).all()
    finally:
        dev.set_unpack()


BIG = 2 ** 32 + 2 ** 20
S0 = 2 ** 31                                    # the window's first sample: byte 2^32


@pytest.mark.parametrize("nfft", (64, 4096))
def test_past_byte_2_32(dev, nfft):
    """a and b are the windows at samples 2^31 + 1 and 2^31 + 4 of one allocation of 4 GiB + 1 MiB (never filled: only the
    window is ever read): the bits of the same bytes uploaded as a small capture."""
    raw = cs.parity_pair()[0]
    hop, m = nfft // 2 + 37, 5
    rows = gpsjam.csd_rows(raw.size, FA, raw.size, FB, nfft, hop, m)
    assert rows >= 1 and 2 * S0 + raw.size <= BIG and 2 * (S0 + FA) > 2 ** 32
    with dev.capture(raw) as small:
        near = run(dev, small, small.nbytes, FA, small, small.nbytes, FB, nfft, hop, m, rows)
    sa, sb = cs.frame_spectra(raw, nfft, hop, FA, 0, rows * m), cs.frame_spectra(raw, nfft, hop, FB, 0, rows * m)
    cs.compare(near, cs.sums_of(sa, sb, m, rows), (nfft, "the window as a capture of its own"))
    big = dev.alloc(BIG)
    try:
        assert big.ptr and big.nbytes == BIG
        big.upload(raw, offset=2 * S0)
        assert big.download(np.uint8, 64, offset=2 * S0).tobytes() == raw[:64].tobytes()
        assert gpsjam.csd_rows(BIG, S0 + FA, BIG, S0 + FB, nfft, hop, m) >= rows
        far = run(dev, big, BIG, S0 + FA, big, BIG, S0 + FB, nfft, hop, m, rows)
    finally:
        big.free()
    assert same(far, near), nfft


def test_device_cross_spectrum_takes_host_bytes_and_captures(dev, pair):
    ra, rb = cs.parity_pair()
    x = dev.cross_spectrum(pair[0], pair[1], frames_per_row=64)
    y = dev.cross_spectrum(ra, rb, nfft=256, hop=256, frames_per_row=64)
    assert (x.nfft, x.hop, x.frames_per_row, x.first_a, x.first_b, len(x)) == (256, 256, 64, 0, 0, 8)
    assert same((x.saa, x.sbb, x.sab, x.msc), (y.saa, y.sbb, y.sab, y.msc)) and dev.last_kernel_ms > 0
    cs.compare((x.saa, x.sbb, x.sab, x.msc), cs.csd(ra, rb, 256, 256, 64), "Device.cross_spectrum")
    part = dev.cross_spectrum(pair[0], pair[1], nfft=64, hop=100, frames_per_row=5, first_a=5, first_b=2, n_rows=3)
    assert len(part) == 3 and part.sab.shape == (3, 64) and part.sab.dtype == np.complex64
    assert len(dev.cross_spectrum(np.zeros(100, np.uint8), rb)) == 0


@pytest.mark.parametrize("case", cs.CASES)
def test_detection_on_the_device(dev, case):
    """The flagged bins of the restatement (tests/test_csd_host.py: no off-DC cell lies within 1e-3 of the threshold)."""
    ref, _ = cs.detect_reference(case)
    want = coherence.detect(ref, cs.P_FA)
    a, b = cs.detect_pair(case)
    with dev.capture(a) as ca, dev.capture(b) as cb:
        got = coherence.scan(dev, ca, cb, fs=cs.FS, nfft=cs.DETECT_NFFT, frames_per_row=cs.DETECT_M[case], p_fa=cs.P_FA)
    assert len(got.result) == len(ref) and got.result.hop == cs.DETECT_NFFT and got.lag == 0
    np.testing.assert_array_equal(got.detection.flagged, want.flagged)
    assert [bd[:5] for bd in got.bands] == [bd[:5] for bd in coherence.bands(ref, want, cs.FS)]
    hit = np.flatnonzero(got.detection.flagged)
    if case == "noise":
        assert hit.size == 0
    elif case == "subnoise":
        assert set(range(cs.SUB_BINS_INSIDE[0], cs.SUB_BINS_INSIDE[1] + 1)) <= set(hit.tolist())
        assert hit.min() >= cs.SUB_BINS_OUTSIDE[0] and hit.max() <= cs.SUB_BINS_OUTSIDE[1]
    else:
        lower, upper = got.bands
        print(f"two: {upper.delay:.4f} and {lower.delay:.4f} against {cs.TWO_DELAY}")
        for have, truth in zip((upper.delay, lower.delay), cs.TWO_DELAY):
            assert abs(have - truth) <= 0.01, (have, truth)
        # the drop-in's form of the same, and the pair aligned by K5's integer lag first (tests/test_csd_host.py restates it)
        import triangulateTDOA as tt
        rows = tt.correlation_lag_bands(tt.IQCapture(b), tt.IQCapture(a), lag=0, frames_per_row=cs.DETECT_M[case])
        assert rows == [(bd.freq_lo_hz, bd.freq_hi_hz, bd.delay) for bd in got.bands]
        k5 = coherence.scan(dev, a, b, lag="k5", fs=cs.FS, nfft=cs.DETECT_NFFT, frames_per_row=cs.DETECT_M[case], p_fa=cs.P_FA)
        assert k5.lag == 3 and (k5.result.first_a, k5.result.first_b, len(k5.result)) == (0, 3, 3) and len(k5.bands) == 2
        print(f"two, aligned by K5's lag {k5.lag}: {k5.bands[1].delay:.4f} and {k5.bands[0].delay:.4f}")
        for have, truth in zip((k5.bands[1].delay, k5.bands[0].delay), cs.TWO_DELAY):
            assert abs(have - truth) <= 0.01, (have, truth)
