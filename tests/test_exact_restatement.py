"""The integer-exact restatements of K1 / K3 / K4 (tests/exact_restatement.py) against the vectors captured from the
reference and against the oracle: they are what the GPU tests compare the kernels with bit for bit, so they are pinned
here, on the CPU, first."""
import os

import numpy as np
import pytest

import exact_restatement as ex
import golden_inputs as gi
from gpsjam.synth import StreamSpec, generate
from oracle import gpsjam_oracle as orc


def test_chunk_power_is_the_references_map(golden_dir, g1_raw):
    g = np.load(os.path.join(golden_dir, "g1_power.npz"))
    np.testing.assert_allclose(ex.chunk_power(g1_raw, 65536), g["power_map"], rtol=1e-6)
    cij = ex.chunk_power(g1_raw, orc.CIJ_CHUNK_BYTES, eps=0.0, odd_chunk_zero=True)
    assert cij[-1] == 0.0                                        # ragged odd tail: checkIfJamming.py:52-55
    np.testing.assert_allclose(cij, g["cij_power"], rtol=1e-6)
    assert np.isnan(ex.chunk_power(np.zeros(65537, np.uint8), 65536)[-1])


def test_onset_is_the_references_index(golden_meta, g4_raws):
    g4 = golden_meta["g4"]
    got = [ex.onset(r) for r in g4_raws]
    assert [o["start"] for o in got] == g4["onset"]
    assert all(o["guard"] == o["start"] and o["hit"] >= 1e-6 for o in got)       # "the reference's by construction"
    assert ex.onset(g4_raws[0][:2 * 200500])["start"] == g4["onset_short"] == -1
    assert ex.onset(g4_raws[0][:2 * 250000])["start"] == g4["onset_none"] == -1
    assert ex.onset(g4_raws[1], 50000, 256, 20.0)["start"] == g4["onset_alt"]
    for o, r in zip(got, g4_raws):                               # noise and threshold: the reference's to float32 rounding
        p = np.abs(orc.tdoa_unpack(r)) ** 2
        np.testing.assert_allclose(o["noise"], np.mean(p[:200000]), rtol=1e-6)
        np.testing.assert_allclose(o["thr"], np.mean(p[:200000]) * 50.0, rtol=1e-6)


def test_amp_stats_are_the_references(golden_meta, g3_raws):
    for key, (idx, avg) in golden_meta["g3"]["amp_stats"].items():
        k, thr_s = key.split("_")
        got = ex.amp_stats(g3_raws[int(k)], float(thr_s))
        assert got["first"] == (-1 if idx is None else idx)
        if idx is not None:
            np.testing.assert_allclose(got["mean"], avg, rtol=1e-6)


@pytest.mark.parametrize("seed,jam,noise,window", [(1, 300_000, 200_000, 1000), (2, 250_123, 100_000, 513), (3, 1 << 40, 200_000, 1000),
                                                  (4, 260_000, 123_457, 8)])
def test_restatements_agree_with_the_oracle_on_synthetic_streams(seed, jam, noise, window):
    raw = generate(StreamSpec(seed=seed, jam_start=jam, jam_end=1 << 40, jam_sigma=60.0), 420_000)
    z = orc.tdoa_unpack(raw)
    assert ex.onset(raw, noise, window, 50.0)["start"] == orc.tdoa_onset(z, noise, window, 50.0)
    for thr in (0.0, 0.3):
        k, avg = orc.rssi_amp_stats(raw, thr)
        got = ex.amp_stats(raw, thr)
        assert got["first"] == (-1 if k is None else k)
        if k is not None:
            np.testing.assert_allclose(got["mean"], avg, rtol=1e-6)
    np.testing.assert_allclose(ex.chunk_power(raw, 65536), orc.chunk_power(raw), rtol=1e-6)


def test_xcorr_f64_is_the_references_lag_and_peak(golden_meta, g4_raws):
    """The float64 restatement of K5 against the reference's own lags and peaks (G4, both slice sizes, own and common
    starts) and against the oracle's complex64 arithmetic; its margin precondition holds on all of them."""
    g4 = golden_meta["g4"]
    on = g4["onset"]
    for n in gi.G4_SLICES:
        for a, b in ((0, 1), (0, 2), (1, 2)):
            zi = orc.tdoa_unpack(g4_raws[a][2 * on[a]:2 * (on[a] + n)])
            for kind, s in (("own", on[b]), ("common", on[a])):
                zj = orc.tdoa_unpack(g4_raws[b][2 * s:2 * (s + n)])
                lag, peak, run = ex.xcorr_f64(zj, zi)
                assert lag == g4[f"lags_{kind}_start"][f"{n}_{a}{b}"] == orc.xcorr_lag(zj, zi)[0]
                np.testing.assert_allclose(peak, g4["peaks"][f"{kind}_{n}_{a}{b}"], rtol=1e-6)
                assert 0.0 < run < 0.05 * peak


@pytest.mark.parametrize("n1,n0", [(1, 1), (2, 2), (1, 7), (7, 5), (100, 100), (1000, 999), (4097, 4097)])
def test_xcorr_f64_is_a_direct_correlation(n1, n0):
    """Every 'full' lag of the FFT restatement equals the direct sum (numpy.correlate conjugates its second argument:
    c[m] = sum_n sig1[n + m - (len(sig0)-1)] conj(sig0[n])), and lag / peak / runner-up are read off it as documented:
    first maximum, |c| there, largest |c| anywhere else.  Peaks planted at both ends of the lag range are found."""
    rng = np.random.default_rng(n1 * 7919 + n0)
    s1 = rng.normal(size=n1) + 1j * rng.normal(size=n1)
    s0 = rng.normal(size=n0) + 1j * rng.normal(size=n0)
    direct = np.correlate(s1, s0, "full")
    got = ex.xcorr_full_f64(s1, s0)
    assert got.shape == direct.shape
    np.testing.assert_allclose(got, direct, rtol=0, atol=1e-9 * np.abs(direct).max())
    for plant in (0, direct.size - 1, direct.size // 2):   # lag -(n0-1), lag n1-1, the middle
        a, b = s1.copy(), s0.copy()
        if plant == 0:
            b[-1], a[0] = 40.0, 40.0j
        elif plant == direct.size - 1:
            b[0], a[-1] = 40.0, -40.0
        else:
            a, b = np.zeros_like(a), np.zeros_like(b)
            a[:min(n0, n1)] = b[:min(n0, n1)] = s0[:min(n0, n1)]
        c = np.abs(np.correlate(a, b, "full"))
        k = int(np.argmax(c))
        lag, peak, run = ex.xcorr_f64(a, b)
        assert lag == k - (n0 - 1)
        if plant != direct.size // 2:
            assert k == plant
        np.testing.assert_allclose(peak, c[k], rtol=1e-12)
        rest = np.delete(c, k)
        np.testing.assert_allclose(run, rest.max() if rest.size else 0.0, rtol=1e-9, atol=1e-9 * c[k])
        assert lag == orc.xcorr_lag(a.astype(np.complex64), b.astype(np.complex64))[0]


@pytest.mark.parametrize("o2", [0, 1, 509, 510])
def test_o2_is_held_to_a_per_sample_loop(o2):
    """The o2 argument of msq / chunk_power / onset / amp_stats (2 * offset of gj_set_unpack, its ends and their
    neighbours) against plain Python integers, sample by sample."""
    import math
    rng = np.random.RandomState(40 + o2)
    raw = rng.randint(0, 256, 2 * 3001 + 1).astype(np.uint8)                 # a trailing odd byte
    raw[:8] = (0, 0, 255, 255, 0, 255, 255, 0)
    raw[2 * 2000:2 * 2600] = 255 if o2 < 255 else 0                          # loud from 2000 on
    e = [(2 * int(raw[2 * k]) - o2) ** 2 + (2 * int(raw[2 * k + 1]) - o2) ** 2 for k in range(raw.size // 2)]
    assert ex.msq(raw, o2).tolist() == e and max(e) == 2 * max(o2, 510 - o2) ** 2 and ex.msq(raw).tolist() == ex.msq(raw, 255).tolist()
    # K1
    got = ex.chunk_power(raw, 1000, eps=0.0, o2=o2)
    for c in range(got.size):
        part = e[500 * c:500 * (c + 1)]
        assert got[c] == np.float32(sum(part) / (4.0 * len(part)))
    # K4
    noise_samples, window, factor = 1500, 64, 1.5
    on = ex.onset(raw, noise_samples, window, factor, o2)
    noise = np.float32(sum(e[:noise_samples]) / (4.0 * noise_samples))
    thr = np.float32(noise * np.float32(factor))
    first = next((k for k in range(len(e) - window + 1) if sum(e[k:k + window]) * (0.25 / window) > float(thr)), None)
    assert first is not None and 1900 < first < 2000
    assert on["noise"] == noise and on["thr"] == thr and on["start"] == first + window // 2
    # K3
    for threshold in (0.0, 1.5):
        st = ex.amp_stats(raw, threshold, o2)
        amp = [math.sqrt(v) / 255.0 for v in e]
        k = next((k for k, a in enumerate(amp) if a > threshold), None)
        assert st["first"] == (k if k is not None else -1) and st["count"] == (len(e) - k if k is not None else 0)
        if k is not None:
            np.testing.assert_allclose(st["mean"], sum(amp[k:]) / (len(e) - k), rtol=1e-6)
