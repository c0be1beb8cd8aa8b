"""CPU side of the K-peak search and the same-PRN spoofing separation (gj_acq_peaks_dev, Device.acq_peaks,
gnss.AcqSearch.peaks, gnss.peak_threshold, spoof.scan_peaks): the interface, the threshold against its own equation, the
restatement the GPU tests compare with (tests/peaks_restatement.py) against the oracle's checkacquisition on the oracle's
own surfaces, the overpowered pair's margins on those surfaces, and the accuracy of the float chain on restated integers,
which sets the tolerances of the GPU test.  No GPU call is made."""
import dataclasses
import math

import numpy as np
import pytest

import corr_restatement as cr
import gpsjam
import host_lib
import peaks_restatement as pr
from gpsjam import _ffi, gnss, postcorr, spoof
from oracle import gpsjam_oracle as orc

NSAMP, NSAMPCHIP, CTIME = 2048, 2, 1023 / 1.023e6


# ------------------------------------------------------------------------------------------------ interface
def test_symbols_bindings_and_python_interface():
    lib = _ffi.load()
    assert len(_ffi.SIGNATURES["gj_acq_peaks_dev"][1]) == 9 and len(_ffi.SIGNATURES["gj_acq_peaks_workspace"][1]) == 3
    for name in ("gj_acq_peaks_dev", "gj_acq_peaks_workspace"):
        assert callable(getattr(lib, name))
    assert _ffi.GJ_VERSION == 150 == lib.gj_version()
    assert _ffi.GJ_ACQ_MAX_PEAKS == gpsjam.ACQ_MAX_PEAKS == pr.MAX_PEAKS == 8
    assert gpsjam.ACQ_PEAK_DTYPE.itemsize == 16 == gpsjam.ACQ_FLOOR_DTYPE.itemsize
    assert gpsjam.ACQ_PEAK_DTYPE.names == ("power", "code_index", "freq_index")
    assert gpsjam.ACQ_FLOOR_DTYPE.names == ("mean_power", "kept_columns", "reserved")
    for name in ("acq_peaks", "acq_peaks_dev", "acq_peaks_workspace"):
        assert callable(getattr(gpsjam.Device, name))
    assert callable(gnss.AcqSearch.peaks) and callable(spoof.scan_peaks) and callable(spoof.pair_phases_peaks)
    # the workspace is pure host arithmetic: three 256-byte aligned arrays of one record per column, 0 for a refused shape
    ws = lib.gj_acq_peaks_workspace(None, 2048, 32)
    assert ws == 2 * 8 * 2048 * 32 + 4 * 2048 * 32
    assert lib.gj_acq_peaks_workspace(None, 9, 1) == 2 * 256 + 256
    for nsamp, n_prn in ((7, 1), (65537, 1), (2048, 0), (-8, 1), (2048, -1)):
        assert lib.gj_acq_peaks_workspace(None, nsamp, n_prn) == 0


# ------------------------------------------------------------------------------------------------ the threshold
def erlang_tail(s, x):
    """Q(s, x) with exact rational terms summed by fsum: written apart from gnss._erlang_tail (no logarithms)."""
    term, terms = 1.0, []
    for j in range(s):
        terms.append(term)
        term *= x / (j + 1)
    return math.exp(-x) * math.fsum(terms)


@pytest.mark.parametrize("steps", [1, 2, 10, 64])
@pytest.mark.parametrize("n_cells", [1, 8, 71 * 2048, 4096 * 65536])
@pytest.mark.parametrize("pfa", [1e-1, 1e-3, 1e-9])
def test_peak_threshold_solves_its_equation(steps, n_cells, pfa):
    g = gnss.peak_threshold(steps, n_cells, pfa)
    assert n_cells * erlang_tail(steps, g * steps) == pytest.approx(pfa, rel=1e-9)
    if steps == 1:
        assert g == pytest.approx(math.log(n_cells / pfa), rel=1e-12)


def test_peak_threshold_falls_with_the_steps_and_its_edges():
    g = [gnss.peak_threshold(s, 71 * 2048, 1e-3) for s in range(1, 65)]
    assert all(a > b for a, b in zip(g, g[1:])) and g[-1] > 1.0
    assert g[9] == pytest.approx(3.93, abs=0.005), g[9]
    assert gnss.peak_threshold(10, 71 * 2048, 1e-6) > g[9] > gnss.peak_threshold(10, 71 * 512, 1e-3)
    assert gnss.peak_threshold(3, 1, 2.0) == 0.0
    for bad in ((0, 10, 1e-3), (1, 0, 1e-3), (1, 10, 0.0), (1, 10, float("nan"))):
        with pytest.raises(ValueError):
            gnss.peak_threshold(*bad)


# ------------------------------------------------------------------------------------------------ the restatement
def brute_top_k(P, k, guard):
    """The definition cell by cell with Python loops (small surfaces only)."""
    n_freq, nsamp = P.shape
    taken, peaks = [], []

    def out(c):
        return any(min(abs(c - c0), nsamp - abs(c - c0)) <= guard for c0 in taken)

    for _ in range(k):
        best = None
        for f in range(n_freq):
            for c in range(nsamp):
                if not out(c) and (best is None or P[f, c] > best[0]):
                    best = (float(P[f, c]), c, f)
        peaks.append(best)
        taken.append(best[1])
    cells = [P[f, c] for f in range(n_freq) for c in range(nsamp) if not out(c)]
    return peaks, (math.fsum(cells) / len(cells), len(cells) // n_freq)


def test_restatement_equals_the_cell_by_cell_loop():
    rng = np.random.default_rng(5)
    for n_freq, nsamp, k, guard in ((1, 8, 1, 0), (1, 8, 2, 1), (3, 29, 4, 2), (2, 16, 8, 0), (5, 40, 3, 5), (4, 9, 2, 1)):
        P = rng.integers(0, 6, (n_freq, nsamp)).astype(np.float64)         # many ties
        peaks, (mean, kept) = pr.top_k(P, k, guard)
        want, (wmean, wkept) = brute_top_k(P, k, guard)
        assert peaks == want and kept == wkept and mean == pytest.approx(wmean, rel=1e-15), (n_freq, nsamp, k, guard)
    P = np.full((3, 10), 2.5)
    assert pr.top_k(P, 3, 1)[0] == [(2.5, 0, 0), (2.5, 2, 0), (2.5, 4, 0)], "all equal: the smallest flat index each time"
    assert pr.top_k(P, 3, 1)[1] == (2.5, 3)


def oracle_surface(raw, prn, steps=10, first=0, freqs=None):
    """P[n_freq][nsamp] of the oracle's pcorrelator over ``steps`` steps, with no early stop."""
    freqs = list(gnss.doppler_bins()) if freqs is None else list(freqs)
    codex = orc.acq_code_fft(prn, NSAMP)
    P = np.zeros(len(freqs) * NSAMP, np.float64)
    for i in range(steps):
        loc = first + i * NSAMP
        data = (np.asarray(raw[2 * loc:2 * (loc + 2 * NSAMP)]).astype(np.int16) - 128).astype(np.int8)
        orc.acq_pcorrelator(data, 1.0 / cr.FS, NSAMP, freqs, 2 * NSAMP, codex, P)
    return P.reshape(len(freqs), NSAMP)


@pytest.fixture(scope="module")
def overpowered_surfaces():
    raw_a, _ = pr.overpowered_pair()
    return {cr.E2E_PRNS[k]: oracle_surface(raw_a, cr.E2E_PRNS[k]) for k in pr.E2E_IDX}


def test_peak_0_is_checkacquisitions_peak_on_the_oracles_surfaces(overpowered_surfaces):
    for prn, P in overpowered_surfaces.items():
        want = orc.acq_check(P.reshape(-1), NSAMP, P.shape[0], NSAMPCHIP, CTIME)
        (power, code, freq), = pr.top_k(P, 1, 2 * NSAMPCHIP)[0]
        assert (power, code, freq) == (want["maxP"], want["codei"], want["freqi"]), prn


def test_peak_1_is_checkacquisitions_second_power_in_one_row(overpowered_surfaces):
    """n_freq = 1 and guard = 2 nsampchip: peak 1's power is maxP2 and the kept columns are the reference's, for zones
    away from the wrap (the first and last positions that do not wrap among them) and across it.  The reference seeds
    its second maximum with column 0 whatever the zone.  Away from the wrap column 0 is outside the zone; a zone that
    wraps always holds column 0, so there the peak is put a chip or more from column 0, whose power is then below the
    second signal of the row (asserted) and the seed does not decide.  The row is PRN 14's, which holds both signals."""
    row = overpowered_surfaces[14][int(np.argmin(np.abs(gnss.doppler_bins() - cr.E2E_DOPPLER[2])))]
    peak = int(np.argmax(row))
    for at in (peak, 5, 1000, NSAMP - 5, 4, 3, 2, NSAMP - 4, NSAMP - 3, NSAMP - 2):
        shifted = np.roll(row, at - peak)
        assert int(np.argmax(shifted)) == at
        zone = pr.excluded(NSAMP, at, 2 * NSAMPCHIP)
        wraps = at - 2 * NSAMPCHIP <= 0 or at + 2 * NSAMPCHIP >= NSAMP
        assert bool(zone[0]) == wraps and zone.sum() == 4 * NSAMPCHIP + 1
        want = orc.acq_check(shifted.copy(), NSAMP, 1, NSAMPCHIP, CTIME)
        peaks, (mean, kept) = pr.top_k(shifted[None, :], 2, 2 * NSAMPCHIP)
        if wraps:
            assert shifted[0] < peaks[1][0], at
        assert peaks[0] == (want["maxP"], want["codei"], 0) and peaks[1][0] == want["maxP2"], at
        # the reference's mean is over the columns outside the FIRST zone: the same set as one peak's kept columns
        one, (mean1, kept1) = pr.top_k(shifted[None, :], 1, 2 * NSAMPCHIP)
        assert kept1 == NSAMP - zone.sum() and mean1 == pytest.approx(want["meanP"], rel=1e-12), at


def test_the_overpowered_pairs_margins(overpowered_surfaces):
    """The seed's check: on the oracle's surfaces every authentic peak is significant at PFA, no third peak is, and the
    single-peak test loses PRN 14, whose copies share a Doppler bin.  Re-measures the two recorded ratios."""
    gamma = gnss.peak_threshold(10, 71 * NSAMP, pr.PFA)
    freqs = gnss.doppler_bins()
    smallest, largest_third = math.inf, 0.0
    for k in pr.E2E_IDX:
        prn = cr.E2E_PRNS[k]
        peaks, (mean, kept) = pr.top_k(overpowered_surfaces[prn], 3, 2 * NSAMPCHIP)
        ratios = [p[0] / mean for p in peaks]
        print(f"PRN {prn}: ratios {ratios[0]:.2f} {ratios[1]:.2f} {ratios[2]:.2f} (gamma {gamma:.3f}), peaks {peaks}")
        for (power, code, freq), (code_true, dop_true) in zip(peaks, ((pr.spoof_code_index(k), pr.spoof_doppler(k)),
                                                                      (cr.E2E_CODE_INDEX[k], cr.E2E_DOPPLER[k]))):
            assert abs(code - code_true) <= 1.0 and abs(freqs[freq] - dop_true) <= 200.0, (prn, code, freqs[freq])
        assert ratios[1] > gamma > ratios[2], prn
        smallest, largest_third = min(smallest, ratios[1]), max(largest_third, ratios[2])
    raw_a, _ = pr.overpowered_pair()
    for prn in pr.ABSENT_PRNS:
        peaks, (mean, kept) = pr.top_k(oracle_surface(raw_a, prn), 1, 2 * NSAMPCHIP)
        print(f"absent PRN {prn}: ratio {peaks[0][0] / mean:.2f}")
        assert peaks[0][0] / mean < gamma, prn
        largest_third = max(largest_third, peaks[0][0] / mean)
    print(f"smallest authentic ratio {smallest:.3f}, largest third-peak ratio {largest_third:.3f}")
    assert smallest == pytest.approx(pr.E2E_MIN_AUTHENTIC_RATIO, rel=0.01) and largest_third == pytest.approx(pr.E2E_MAX_THIRD_RATIO, rel=0.01)
    lost = orc.acq_check(overpowered_surfaces[14].reshape(-1), NSAMP, 71, NSAMPCHIP, CTIME)
    print(f"PRN 14 through checkacquisition: peak ratio {lost['peakr']:.2f}")
    assert not lost["acquired"], "the gap: both copies in one Doppler row, the authentic one is the second power"


def test_noise_only_surfaces_stay_under_the_threshold():
    rng = np.random.default_rng(11)
    raw = cr.quantise(rng.normal(0.0, cr.E2E_SIGMA, 11 * NSAMP) + 1j * rng.normal(0.0, cr.E2E_SIGMA, 11 * NSAMP))
    gamma = gnss.peak_threshold(10, 71 * NSAMP, pr.PFA)
    for prn in (4, 14):
        peaks, (mean, kept) = pr.top_k(oracle_surface(raw, prn), 2, 2 * NSAMPCHIP)
        assert kept == NSAMP - 2 * 9 and peaks[0][0] / mean < gamma, (prn, peaks[0][0] / mean)


# ------------------------------------------------------------------------------------------------ the Python layers
class HostLib(host_lib.HostLib):
    """gj_corr_bank_dev and gj_acq_peaks_dev computed by the restatements on host memory (tests/host_lib.py)."""

    def gj_corr_bank_dev(self, ctx, d_iq, nbytes, first, n, B, d_codes, n_rows, d_channels, n_channels, taps, n_taps, d_out):
        taps = [int(taps[j]) for j in range(n_taps)]
        self.calls.append(("corr", first, n, B, n_rows, n_channels, tuple(taps)))
        codes = self.view(d_codes, n_rows * 1023, np.int16).reshape(n_rows, 1023)
        channels = [tuple(int(v) for v in c) for c in self.view(d_channels, n_channels, gpsjam.CORR_CHANNEL_DTYPE)]
        out = cr.bank(self.view(d_iq, nbytes), first, n, B, codes, channels, taps)
        self.view(d_out, out.size, np.int32)[:] = out.reshape(-1)
        return 0

    def gj_acq_peaks_dev(self, ctx, d_power, n_prn, n_freq, nsamp, k, guard, d_peaks, d_floor):
        self.calls.append(("peaks", n_prn, n_freq, nsamp, k, guard))
        P = self.view(d_power, n_prn * n_freq * nsamp, np.float64).reshape(n_prn, n_freq, nsamp)
        power, code, freq, mean, kept = pr.top_k_all(P, k, guard)
        rec = self.view(d_peaks, n_prn * k, gpsjam.ACQ_PEAK_DTYPE)
        rec["power"], rec["code_index"], rec["freq_index"] = power.reshape(-1), code.reshape(-1), freq.reshape(-1)
        fl = self.view(d_floor, n_prn, gpsjam.ACQ_FLOOR_DTYPE)
        fl["mean_power"], fl["kept_columns"], fl["reserved"] = mean, kept, 0
        return 0


@pytest.fixture
def host_dev():
    dev = host_lib.host_device(HostLib())
    yield dev
    dev._ctx = None            # a Capture that outlives the test frees nothing


def test_device_acq_peaks_on_the_host_double(host_dev):
    lib = host_dev._lib
    P = pr.random_surfaces(3, 2, 500)
    peaks, floor = host_dev.acq_peaks(P, k=2, guard=4)
    power, code, freq, mean, kept = pr.top_k_all(P, 2, 4)
    assert peaks.dtype == gpsjam.ACQ_PEAK_DTYPE and peaks.shape == (3, 2) and floor.dtype == gpsjam.ACQ_FLOOR_DTYPE and floor.shape == (3,)
    assert np.array_equal(peaks["power"], power) and np.array_equal(peaks["code_index"], code) and np.array_equal(peaks["freq_index"], freq)
    assert np.array_equal(floor["mean_power"], mean) and np.array_equal(floor["kept_columns"], kept)
    assert host_lib.mallocs(lib) == [P.nbytes, 16 * 3 * 2, 16 * 3] and lib.calls[-1] == ("peaks", 3, 2, 500, 2, 4)
    assert not lib.mem, "everything is freed"
    assert host_dev.kernel_calls == {"acq_peaks": 1}
    # a device buffer needs its shape; a refusal of the library raises and frees everything
    with host_dev.alloc(P.nbytes) as d_power:
        d_power.upload(P)
        again, _ = host_dev.acq_peaks(d_power, k=1, guard=0, shape=P.shape)
        assert np.array_equal(again["power"][:, 0], power[:, 0])
        with pytest.raises(ValueError):
            host_dev.acq_peaks(d_power, k=1)
        assert set(lib.mem) == {d_power.ptr}
    with pytest.raises(ValueError):
        host_dev.acq_peaks(np.zeros((4, 8)))
    lib.refuse("gj_acq_peaks_dev")
    with pytest.raises(gpsjam.GpsJamError) as e:
        host_dev.acq_peaks(P, k=9)
    assert str(e.value) == host_lib.REFUSED_TEXT and not lib.mem


def test_observe_takes_results_in_place_of_the_search(host_dev):
    """``results=None`` is the search's own answer; given, the search is not asked, and a PRN may stand twice."""
    a, _ = cr.e2e_pair("authentic")
    search = cr.GridSearch("authentic")
    own = postcorr.observe(host_dev, a, search)
    given = postcorr.observe(host_dev, a, search, results=search.search(a))
    assert [o.prn for o in own] == [o.prn for o in given] and all(np.array_equal(x.prompts, y.prompts) for x, y in zip(own, given))

    class Unasked(cr.GridSearch):
        def search(self, capture, first_sample=0):
            raise AssertionError("the search was asked")

    r = search.search(a)[0]
    twice = postcorr.observe(host_dev, a, Unasked("authentic"), results=[r, dataclasses.replace(r, code_index=r.code_index + 900)])
    assert [o.prn for o in twice] == [r.prn, r.prn]
    assert np.array_equal(twice[0].prompts, own[0].prompts)
    assert postcorr.cn0(twice[1].prompts, 1e-3) < own[0].cn0_dbhz - 10.0, "no signal at the second code phase"


def test_end_to_end_accuracy_sets_the_tolerances_and_the_verdicts_hold(host_dev):
    """Re-measures pr.E2E_CPU_ERROR_*, which the GPU test's tolerances are twice of, on the AUTHENTIC candidates of the
    overpowered pair, and checks both verdicts."""
    a, b = pr.overpowered_pair()
    rep = spoof.scan_peaks(host_dev, a, b, pr.TruthSearch("overpowered"), tol=cr.E2E_TOL)
    prns = [cr.E2E_PRNS[k] for k in pr.E2E_IDX]
    assert [c.prn for c in rep.candidates] == [p for p in prns for _ in (0, 1)], "every PRN twice, the strong copy first"
    assert rep.spoofed is True and rep.common_prns == sorted(prns) and rep.common == [0, 2, 4, 6, 8]
    assert rep.p_chance == pytest.approx(spoof.chance(5, 10, cr.E2E_TOL))
    assert [c.prn for c in rep.counterfeit] == prns == [c.prn for c in rep.authentic]
    assert rep.counterfeit == [rep.candidates[i] for i in (0, 2, 4, 6, 8)] and rep.authentic == [rep.candidates[i] for i in (1, 3, 5, 7, 9)]
    worst = {"phase": 0.0, "doppler": 0.0, "cn0": 0.0}
    for c, fake in zip(rep.candidates, [True, False] * 5):
        k = cr.E2E_PRNS.index(c.prn)
        psi, dop, cn0, code = ((cr.E2E_SPOOF_PHASE, pr.spoof_doppler(k), cr.E2E_CN0[k] + pr.SPOOF_GAIN_DB, pr.spoof_code_index(k)) if fake else
                               (cr.E2E_AUTHENTIC[k], cr.E2E_DOPPLER[k], cr.E2E_CN0[k], cr.E2E_CODE_INDEX[k]))
        e_ph, e_dop, e_cn0 = abs(float(cr.wrap(c.phase - psi))), abs(c.doppler_hz - dop), abs(c.cn0_dbhz - cn0)
        print(f"PRN {c.prn} {'counterfeit' if fake else 'authentic  '}: code {c.code_index}, phase {c.phase:+.4f} (error {e_ph:.4f}), Doppler error "
              f"{e_dop:.3f} Hz, C/N0 {c.cn0_dbhz:.2f} (error {e_cn0:.2f} dB), coherence {c.coherence:.3f}")
        assert abs(c.code_index - code) <= 1.0 and c.coherence > 0.8
        if fake:
            assert e_ph < cr.E2E_TOL, "inside the arc"
        else:
            worst = {"phase": max(worst["phase"], e_ph), "doppler": max(worst["doppler"], e_dop), "cn0": max(worst["cn0"], e_cn0)}
    print("worst of the authentic candidates:", worst)
    for key, recorded in (("phase", pr.E2E_CPU_ERROR_PHASE), ("doppler", pr.E2E_CPU_ERROR_DOPPLER), ("cn0", pr.E2E_CPU_ERROR_CN0)):
        assert abs(worst[key] - recorded) <= 0.1 * recorded, (key, worst[key], recorded)
    assert (pr.E2E_TOL_PHASE, pr.E2E_TOL_DOPPLER, pr.E2E_TOL_CN0) == (2 * pr.E2E_CPU_ERROR_PHASE, 2 * pr.E2E_CPU_ERROR_DOPPLER, 2 * pr.E2E_CPU_ERROR_CN0)
    # the authentic pair: one candidate per PRN, nothing shared, nothing listed
    a, b = cr.e2e_pair("authentic")
    rep = spoof.scan_peaks(host_dev, a, b, pr.TruthSearch("authentic"), tol=cr.E2E_TOL)
    assert [c.prn for c in rep.candidates] == prns and rep.spoofed is False and rep.counterfeit == [] == rep.authentic


def test_a_prn_counts_once_and_too_few_give_no_verdict(host_dev):
    a, b = pr.overpowered_pair()

    class Three(pr.TruthSearch):
        def peaks(self, *args, **kw):
            return super().peaks(*args, **kw)[:3]

    rep = spoof.scan_peaks(host_dev, a, b, Three("overpowered"), tol=cr.E2E_TOL)
    assert len(rep.candidates) == 6 and rep.spoofed is None and rep.counterfeit == [] == rep.authentic

    class Same(pr.TruthSearch):
        """Four candidates in the arc, of three PRNs: PRN 4's counterfeit twice."""
        def peaks(self, *args, **kw):
            out = super().peaks(*args, **kw)[:4]
            out[3] = gnss.AcqPeaks(out[3].prn, 10, 1.0, [out[3].peaks[1]])          # PRN 21: the authentic signal alone
            out[0] = gnss.AcqPeaks(out[0].prn, 10, 1.0, [out[0].peaks[0], out[0].peaks[0], out[0].peaks[1]])
            return out

    rep = spoof.scan_peaks(host_dev, a, b, Same("overpowered"), k=3, tol=cr.E2E_TOL)
    assert len(rep.common) == 4 and rep.common_prns == [4, 9, 14] and rep.spoofed is False
    assert spoof.scan_peaks(host_dev, a, b, Same("overpowered"), k=3, tol=cr.E2E_TOL, min_common=3).spoofed is True
