"""Spectral kurtosis (gj_sk_dev, Device.spectral_kurtosis, gpsjam.kurtosis) on the GPU.

This file sits in a package of its own on purpose, as tests/ridge/ does: the suite orders GPU files by basename
(tests/conftest.py SUITE_ORDER, which tests/test_suite_order.py holds every GPU file to), and under the name
test_round6_gpu.py it runs in stage 2, behind the parity tests of K2 whose transform it shares.

Yardstick: the float64 restatement of the definition in include/gpsjam.h (tests/skurt_restatement.py).
  S1: |S1 - ref| <= 1e-5 of the row's largest reference S1 -- the project's figure for a K2 value summed in another
      order (tests/test_gpu_parity.py), taken relative to the row's maximum as the ridge does for `second`;
  S2: 2e-5 of the row's largest reference S2, since P^2 carries twice P's relative error.
With M <= 64 the float32 summation adds at most 64 * 2^-24 = 4e-6; the one case with M = 130 (two rounding steps per
frame and 9 block sums: 139 * 2^-24 = 8e-6 at the very worst, a random walk in practice) is held to the same bound.
d_sk: within 2 float32 ulps of the formula in float64 on the downloaded S1 and S2, NaN exactly where S1 == 0.
Translation, fewer rows, d_sk = NULL and repetition are bit-exact.  Every call writes into sentinel-filled buffers whose
bytes behind [n_rows][nfft] must stay untouched."""
import numpy as np
import pytest

import gpsjam
import ridge_restatement as rr
import skurt_restatement as sr
from gpsjam import kurtosis, mitigate
from gpu_lib import GJ_ERR_INVALID, GJ_ERR_UNSUPPORTED, Guarded, freed, refused
from gpu_lib import run_sk as run

pytestmark = pytest.mark.gpu



@pytest.fixture(scope="module")
def cap(dev):
    c = dev.capture(rr.parity_capture())
    yield c
    c.free()


@pytest.mark.parametrize("nfft", sr.NFFT)
def test_parity_with_the_restatement(dev, cap, nfft):
    for hop in sr.parity_hops(nfft):
        for first in (0, 1):
            p = sr.parity_powers(nfft, hop, first)
            for m in sr.PARITY_M:
                n_rows = gpsjam.sk_rows(cap.nbytes, first, nfft, hop, m)
                assert n_rows == p.shape[0] // m >= 1
                sr.compare(run(dev, cap, cap.nbytes, nfft, hop, first, m, n_rows), p, m, n_rows, (nfft, hop, first, m))
    print(f"nfft {nfft}: largest errors so far S1 {sr.worst['s1']:.2e} (tolerance {sr.S1_TOL:.0e}), S2 {sr.worst['s2']:.2e} "
          f"(tolerance {sr.S2_TOL:.0e}), SK {sr.worst['sk_ulp']:.2f} ulp")


@pytest.mark.parametrize("nfft", sr.BOUNDARY_NFFT)      # a group inside a wave, a whole wave, the whole workgroup
def test_block_boundaries(dev, cap, nfft):
    """Rows of 1, 2, 3, ... blocks, with a full and with a short last block (blocks hold at most MAX_RUN = 16 frames)."""
    hop, first = sr.BOUNDARY_HOP, 1
    p = sr.parity_powers(nfft, hop, first)
    for m in sr.BOUNDARY_M:
        for n_rows in (1, 3):
            assert n_rows <= gpsjam.sk_rows(cap.nbytes, first, nfft, hop, m)
            sr.compare(run(dev, cap, cap.nbytes, nfft, hop, first, m, n_rows), p, m, n_rows, (nfft, m, n_rows))
    print(f"nfft {nfft}: largest errors so far S1 {sr.worst['s1']:.2e}, S2 {sr.worst['s2']:.2e}, SK {sr.worst['sk_ulp']:.2f} ulp")


def test_exactly_all_rows_that_fit(dev):
    """The last frame of the last row ends on the capture's last byte."""
    raw = rr.parity_capture()
    for nfft, hop, first, m, n_rows in ((16, 16, 0, 2, 300), (256, 165, 1, 5, 7), (4096, 4096, 1, 17, 1)):
        nbytes = 2 * (first + (n_rows * m - 1) * hop + nfft)
        assert gpsjam.sk_rows(nbytes, first, nfft, hop, m) == n_rows and gpsjam.sk_rows(nbytes - 2, first, nfft, hop, m) == n_rows - 1
        with dev.capture(raw[:nbytes]) as exact:
            got = run(dev, exact, nbytes, nfft, hop, first, m, n_rows)
        sr.compare(got, sr.parity_powers(nfft, hop, first), m, n_rows, (nfft, "exact"))


def test_workgroups_that_take_more_than_one_step(dev):
    """nfft 16, hop 1, M 4 on 2^18 samples, compared in full: 65 532 rows of one block each, 256 blocks per workgroup
    step.  Then M 2 on 2^19 samples: 1024 steps, more than the 512 workgroups of one round (two per CU at 16 points) on
    256 CUs, and more than 768 should the kernel ever keep three."""
    raw = rr.classifier_capture("cw")
    assert raw.size == 2 << 18
    n_rows = gpsjam.sk_rows(raw.size, 0, 16, 1, 4)
    assert n_rows == ((1 << 18) - 16 + 1) // 4
    with dev.capture(raw) as c:
        got = run(dev, c, c.nbytes, 16, 1, 0, 4, n_rows)
    sr.compare(got, sr.frame_powers(raw, 16, 1, 0, 4 * n_rows), 4, n_rows, "M 4 on 2^18 samples")
    raw = sr.detect_capture("tone")
    n_rows = gpsjam.sk_rows(raw.size, 0, 16, 1, 2)
    assert n_rows * 1 >= 768 * 256 + 1
    with dev.capture(raw) as c:
        got = run(dev, c, c.nbytes, 16, 1, 0, 2, n_rows, want_sk=False)
    sr.compare(got, sr.frame_powers(raw, 16, 1, 0, 2 * n_rows), 2, n_rows, "M 2 on 2^19 samples")


@pytest.mark.parametrize("nfft", sr.BOUNDARY_NFFT)
def test_bit_exact_behaviour(dev, cap, nfft):
    hop, first, m = 101, 3, 18                            # two blocks of 9 frames
    n = gpsjam.sk_rows(cap.nbytes, first, nfft, hop, m)
    assert n >= 12
    a = run(dev, cap, cap.nbytes, nfft, hop, first, m, n)
    again = run(dev, cap, cap.nbytes, nfft, hop, first, m, n)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, again))
    for k in (1, 2, 7):                                   # started k rows later: the same rows, bit for bit
        b = run(dev, cap, cap.nbytes, nfft, hop, first + k * m * hop, m, n - k)
        assert all(x.tobytes() == y[k:].tobytes() for x, y in zip(b, a)), (nfft, k)
    third = run(dev, cap, cap.nbytes, nfft, hop, first, m, n // 3)      # fewer rows: another grid, the same bits
    assert all(x.tobytes() == y[:n // 3].tobytes() for x, y in zip(third, a))
    s1, s2, none = run(dev, cap, cap.nbytes, nfft, hop, first, m, n, want_sk=False)
    assert none is None and s1.tobytes() == a[0].tobytes() and s2.tobytes() == a[1].tobytes()


def test_unpack_convention(dev, cap):
    try:
        dev.set_unpack(128.0, 1.0 / 128.0)
        with dev.capture(np.full(2 * 5000, 128, np.uint8)) as flat:
            for nfft in (16, 256, 2048):
                n = gpsjam.sk_rows(flat.nbytes, 1, nfft, nfft // 2, 2)
                s1, s2, skv = run(dev, flat, flat.nbytes, nfft, nfft // 2, 1, 2, n)
                assert n >= 1 and not s1.any() and not s2.any() and np.isnan(skv).all()
        for nfft in sr.NFFT:
            hop = nfft // 2 + 37
            p = sr.parity_powers(nfft, hop, 1, 128.0, 1.0 / 128.0)
            n_rows = p.shape[0] // 5
            sr.compare(run(dev, cap, cap.nbytes, nfft, hop, 1, 5, n_rows), p, 5, n_rows, (nfft, "gnssdec convention"))
    finally:
        dev.set_unpack()
    assert dev.get_unpack() == (127.5, 1.0 / 127.5)
    p = sr.parity_powers(256, 256, 0)
    sr.compare(run(dev, cap, cap.nbytes, 256, 256, 0, 17, p.shape[0] // 17), p, 17, p.shape[0] // 17, "default convention restored")


def test_refusals_enqueue_nothing(dev, cap):
    fit = gpsjam.sk_rows(cap.nbytes, 0, 256, 128, 16)
    size = 4 * (fit + 1) * 256
    s1, s2, skb = (Guarded(dev, size) for _ in range(3))
    ok = (cap, cap.nbytes, 0, 256, 128, 16, 4)
    cases = [  # d_iq, nbytes, first, nfft, hop, M, n_rows, d_s1, d_s2, d_sk, status
        (cap, cap.nbytes, 0, 8, 4, 16, 4, s1, s2, skb, GJ_ERR_UNSUPPORTED),
        (cap, cap.nbytes, 0, 8192, 4096, 2, 1, s1, s2, skb, GJ_ERR_UNSUPPORTED),
        (cap, cap.nbytes, 0, 48, 24, 16, 4, s1, s2, skb, GJ_ERR_UNSUPPORTED),
        (cap, cap.nbytes, 0, 256, 0, 16, 4, s1, s2, skb, GJ_ERR_INVALID),                    # hop 0
        (cap, cap.nbytes, 0, 256, 128, 1, 4, s1, s2, skb, GJ_ERR_INVALID),                   # M below 2
        (cap, cap.nbytes, 0, 256, 128, 0, 4, s1, s2, skb, GJ_ERR_INVALID),
        (cap, cap.nbytes, 0, 256, 128, -5, 4, s1, s2, skb, GJ_ERR_INVALID),
        (cap, cap.nbytes, 0, 16, 1, 65537, 1, s1, s2, skb, GJ_ERR_UNSUPPORTED),              # M above 65536 (one such row fits)
        (cap, cap.nbytes, 0, 256, 128, 16, 0, s1, s2, skb, GJ_ERR_INVALID),                  # no row
        (cap, cap.nbytes, 0, 256, 128, 16, fit + 1, s1, s2, skb, GJ_ERR_INVALID),            # more than fit
        (cap, cap.nbytes, cap.nsamples, 256, 128, 16, 1, s1, s2, skb, GJ_ERR_INVALID),
        (cap, cap.nbytes, 2 ** 64 - 8, 256, 128, 16, 1, s1, s2, skb, GJ_ERR_INVALID),        # first_sample + nfft wraps
        (0, *ok[1:], s1, s2, skb, GJ_ERR_INVALID),                                           # null d_iq
        (cap.ptr + 1, cap.nbytes - 2, *ok[2:], s1, s2, skb, GJ_ERR_INVALID),                 # odd d_iq
        (*ok, 0, s2, skb, GJ_ERR_INVALID),                                                   # null d_s1
        (*ok, s1, 0, skb, GJ_ERR_INVALID),                                                   # null d_s2
        (*ok, s1.ptr + 2, s2, skb, GJ_ERR_INVALID),                                          # misaligned outputs
        (*ok, s1, s2.ptr + 1, skb, GJ_ERR_INVALID),
        (*ok, s1, s2, skb.ptr + 2, GJ_ERR_INVALID),
    ]
    try:
        refused(dev, dev.spectral_kurtosis_dev, [(c[:-1], c[-1]) for c in cases], s1, s2, skb)
        # accepted: M at its smallest, a call that just fits, no d_sk
        dev.spectral_kurtosis_dev(cap, cap.nbytes, 0, 16, 8, 2, 4, s1, s2, skb)
        dev.spectral_kurtosis_dev(cap, cap.nbytes, 0, 256, 128, 16, fit, s1, s2, None)
        dev.synchronize()
        for b, what in ((s1, "S1"), (s2, "S2"), (skb, "SK")):
            b.check_pads(what)
    finally:
        freed(s1, s2, skb)


def test_device_spectral_kurtosis_takes_host_bytes_and_captures(dev, cap):
    p = sr.parity_powers(256, 256, 0)
    a = dev.spectral_kurtosis(cap, frames_per_row=64)
    b = dev.spectral_kurtosis(rr.parity_capture(), nfft=256, hop=256, frames_per_row=64)
    assert (a.nfft, a.hop, a.frames_per_row, a.first_sample, len(a)) == (256, 256, 64, 0, 8)
    assert a.s1.tobytes() == b.s1.tobytes() and a.s2.tobytes() == b.s2.tobytes() and a.sk.tobytes() == b.sk.tobytes()
    sr.compare((a.s1, a.s2, a.sk), p, 64, 8, "Device.spectral_kurtosis")
    part = dev.spectral_kurtosis(cap, nfft=64, hop=100, frames_per_row=5, first_sample=5, n_rows=3)
    assert len(part) == 3 and part.s1.shape == (3, 64)
    np.testing.assert_allclose(a.merged(), sr.sums_of(p, 512, 1)[2][0], rtol=1e-4)
    assert len(dev.spectral_kurtosis(np.zeros(100, np.uint8))) == 0
    need = dev.sk_workspace(256, 64, 8)
    assert need == 8 * 4 * 2 * 256 * 4
    dev.reserve(need)


@pytest.mark.parametrize("case", sr.CASES)
def test_detection_on_the_device(dev, case):
    """The flagged bins of the restatement (tests/test_skurt_host.py: no cell lies within 1e-3 of a band edge)."""
    ref, _ = sr.detect_reference(case)
    want = kurtosis.detect(ref, sr.SIGMAS)
    with dev.capture(sr.detect_capture(case)) as c:
        got = kurtosis.scan(dev, c, fs=sr.FS, nfft=sr.DETECT_NFFT, frames_per_row=sr.DETECT_M, sigmas=sr.SIGMAS)
    assert len(got.result) == 8 and got.result.hop == sr.DETECT_NFFT
    np.testing.assert_array_equal(got.detection.steady, want.steady)
    np.testing.assert_array_equal(got.detection.intermittent, want.intermittent)
    assert [b[:4] for b in got.bands] == [b[:4] for b in kurtosis.bands(ref, want, sr.FS)]
    if case == "tone":
        assert np.flatnonzero(got.detection.steady).tolist() == [sr.TONE_BIN]


@pytest.mark.parametrize("amp", sr.EXCISE_AMPS)
def test_a_tone_from_the_first_sample_is_found_excised_and_gone(dev, amp):
    with dev.capture(sr.excise_capture(amp)) as c:
        first = kurtosis.scan(dev, c, fs=sr.FS, nfft=sr.DETECT_NFFT, frames_per_row=sr.DETECT_M, sigmas=sr.SIGMAS)
        assert first.detection.steady[sr.TONE_BIN] and not first.detection.intermittent.any()
        thr = kurtosis.excision_threshold(first.result, first.detection, rise_db=12.0)
        res = mitigate.clean(dev, c, nfft=sr.DETECT_NFFT, threshold=thr)
    try:
        assert res.floor_from == "given" and res.capture.nbytes == c.nbytes and 0.0 < res.removed_share < 1.0
        again = kurtosis.scan(dev, res.capture, fs=sr.FS, nfft=sr.DETECT_NFFT, frames_per_row=sr.DETECT_M, sigmas=sr.SIGMAS)
    finally:
        res.capture.free()
    assert not again.detection.flagged.any() and again.bands == [], (amp, again.bands)
