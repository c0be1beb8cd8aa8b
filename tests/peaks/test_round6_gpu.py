"""The K-peak search on the GPU (gj_acq_peaks_dev, Device.acq_peaks, gnss.AcqSearch.peaks) and what is built on it: the
same-PRN spoofing separation (spoof.scan_peaks).

This file sits in a package of its own on purpose, as tests/corr/ does: the suite orders GPU files by basename
(tests/conftest.py SUITE_ORDER, which tests/test_suite_order.py holds every GPU file to), and under the name
test_round6_gpu.py it runs in stage 2.

Yardstick: the plain-argmax restatement of the definition in include/gpsjam.h (tests/peaks_restatement.py, which
tests/test_peaks_host.py holds to a cell-by-cell loop and to the oracle's checkacquisition).  Peaks are comparisons only:
power bits, code index and freq index are equal, bit for bit, and so is kept_columns.  The floor is a sum of non-negative
doubles in another order than numpy's: within n_cells 2^-53 relative, the bound for any order.  Surfaces are uploaded
doubles, so most cases run no acquisition at all.  Every call writes into sentinel-filled buffers whose 256 bytes behind
the call's records must stay untouched.  The float observables of the end-to-end pair are held to twice the error that
tests/test_peaks_host.py measures on the CPU with the same host code on restated integers."""
import numpy as np
import pytest

import corr_restatement as cr
import gpsjam
import peaks_restatement as pr
from gpsjam import gnss, spoof
from gpu_lib import GJ_ERR_INVALID, GJ_ERR_UNSUPPORTED, SENTINEL, Guarded, refused
from gpu_lib import run_peaks as run

pytestmark = pytest.mark.gpu



def compare(dev, P, k, guard):
    peaks, floor = run(dev, P, k, guard)
    power, code, freq, mean, kept = pr.top_k_all(P, k, guard)
    note = f"shape {np.shape(P)} k {k} guard {guard}"
    np.testing.assert_array_equal(peaks["power"].view(np.uint64), power.view(np.uint64), err_msg=note)
    np.testing.assert_array_equal(peaks["code_index"], code, err_msg=note)
    np.testing.assert_array_equal(peaks["freq_index"], freq, err_msg=note)
    np.testing.assert_array_equal(floor["kept_columns"], kept, err_msg=note)
    assert not floor["reserved"].any()
    n_freq = np.shape(P)[1]
    assert np.all(np.abs(floor["mean_power"] - mean) <= pr.floor_bound(n_freq, kept) * mean), (note, floor["mean_power"], mean)
    return peaks, floor


def widest_guard(nsamp, k, most=4):
    """The largest guard up to ``most`` that k zones of an nsamp-column surface allow: k (2 guard + 1) < nsamp."""
    return min(most, ((nsamp - 1) // k - 1) // 2)


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("nsamp", [8, 500, 512, 1000, 2048, 4099])
def test_parity_with_the_restatement(dev, nsamp):
    """Random surfaces: ragged last tiles of 64 columns (8, 500, 1000, 4099), 1, 2 and 71 rows over four row waves, one to 32
    workgroups of picks.  At 8 columns eight zones leave no column: that call is refused, and seven peaks stand in."""
    for n_freq in (1, 2, 71):
        for n_prn in (1, 3, 32):
            P = pr.random_surfaces(n_prn, n_freq, nsamp)
            for k in (1, 2, 8):
                if k * 1 >= nsamp:
                    with pytest.raises(gpsjam.GpsJamError) as e:
                        run(dev, P, k, 0)
                    assert e.value.status == GJ_ERR_INVALID
                    k = nsamp - 1
                compare(dev, P, k, widest_guard(nsamp, k))
    again = [run(dev, pr.random_surfaces(3, 71, nsamp), 2, widest_guard(nsamp, 2)) for _ in (0, 1)]
    assert again[0][0].tobytes() == again[1][0].tobytes() and again[0][1].tobytes() == again[1][1].tobytes(), "two calls, identical bits"


def test_device_acq_peaks_is_the_restatement(dev):
    P = pr.random_surfaces(3, 71, 1000)
    calls = dev.kernel_calls.get("acq_peaks", 0)
    peaks, floor = dev.acq_peaks(P)                                    # k = 2, guard = 4
    assert dev.kernel_calls["acq_peaks"] == calls + 1
    want, want_floor = run(dev, P, 2, 4)
    assert peaks.tobytes() == want.tobytes() and floor.tobytes() == want_floor.tobytes()
    power, code, freq, mean, kept = pr.top_k_all(P, 2, 4)
    assert np.array_equal(peaks["power"], power) and np.array_equal(peaks["code_index"], code) and np.array_equal(floor["kept_columns"], kept)
    assert dev.acq_peaks_workspace(1000, 3) == 2 * 24064 + 12032, "two doubles and an int per column, each array to 256 bytes"
    with pytest.raises(gpsjam.GpsJamError) as e:
        dev.acq_peaks(P, k=9)
    assert e.value.status == GJ_ERR_UNSUPPORTED


# ------------------------------------------------------------------------------------------------ 2. ties
def flat(n_freq, nsamp, value=1.0):
    return np.full((1, n_freq, nsamp), value)


def test_equal_maxima_in_two_rows_of_one_column(dev):
    """The first row that attains the maximum wins: rows of one wave (2 and 6, 2 and 30: inside and across its six loads
    in flight), rows of two waves where the later wave holds the earlier row (5 before 6, 3 before 8), the last rows."""
    for n_freq, rows in ((71, (2, 6)), (71, (2, 30)), (71, (5, 6)), (71, (3, 8)), (71, (66, 70)), (71, (0, 70)), (2, (0, 1)), (7, (4, 6))):
        P = flat(n_freq, 300)
        for r in rows:
            P[0, r, 137] = 9.0
        peaks, _ = compare(dev, P, 2, 4)
        assert (peaks[0, 0]["power"], peaks[0, 0]["code_index"], peaks[0, 0]["freq_index"]) == (9.0, 137, rows[0]), rows


def test_equal_maxima_in_two_columns_the_flat_index_decides(dev):
    """The larger column holds the smaller row: its flat index is the smaller one and wins.  Columns of one thread of the pick
    (10 and 266), of two lanes, of two waves, and both orders."""
    for n_freq, (r_small, c_large), (r_large, c_small) in ((71, (2, 266), (5, 10)), (71, (2, 30), (5, 10)), (71, (0, 200), (70, 10)),
                                                          (2, (0, 1990), (1, 0)), (71, (3, 100), (3, 10))):
        P = flat(n_freq, 2000)
        P[0, r_small, c_large] = P[0, r_large, c_small] = 7.0
        peaks, _ = compare(dev, P, 2, 4)
        first = (r_small, c_large) if r_small * 2000 + c_large < r_large * 2000 + c_small else (r_large, c_small)
        second = (r_large, c_small) if first == (r_small, c_large) else (r_small, c_large)
        assert (peaks[0, 0]["freq_index"], peaks[0, 0]["code_index"]) == first and (peaks[0, 1]["freq_index"], peaks[0, 1]["code_index"]) == second
        assert peaks[0, 0]["power"] == peaks[0, 1]["power"] == 7.0


def test_an_all_equal_surface(dev):
    """Every pick is the smallest flat index left: row 0, columns 0, guard + 1, 2 guard + 2, ... (column 0's zone wraps)."""
    for n_freq, nsamp, k, guard in ((71, 500, 8, 4), (1, 8, 3, 0), (3, 4099, 8, 100), (2, 64, 2, 0)):
        peaks, floor = compare(dev, flat(n_freq, nsamp, 2.5), k, guard)
        assert peaks[0]["code_index"].tolist() == [j * (guard + 1) for j in range(k)] and not peaks[0]["freq_index"].any()
        assert floor[0]["mean_power"] == 2.5 and floor[0]["kept_columns"] == nsamp - (2 * guard + 1) - (k - 1) * (guard + 1)


# ------------------------------------------------------------------------------------------------ 3. zones
def test_zones_wrap_at_both_ends(dev):
    nsamp, guard = 500, 4
    for c0 in (0, nsamp - 1, 3, nsamp - 4):
        P = pr.random_surfaces(1, 5, nsamp).copy()
        P[0, 2, c0] = 1000.0
        # larger than everything else, inside the zone on the far side of the wrap and just outside it
        P[0, 4, (c0 + guard) % nsamp] = P[0, 1, (c0 - guard) % nsamp] = 900.0
        P[0, 3, (c0 - guard - 1) % nsamp] = 800.0
        peaks, floor = compare(dev, P, 2, guard)
        assert (peaks[0, 0]["code_index"], peaks[0, 0]["freq_index"]) == (c0, 2)
        assert (peaks[0, 1]["code_index"], peaks[0, 1]["freq_index"], peaks[0, 1]["power"]) == ((c0 - guard - 1) % nsamp, 3, 800.0)
        assert floor[0]["kept_columns"] == nsamp - (3 * guard + 2), "the two zones overlap: columns c0 - 2 guard - 1 .. c0 + guard"


@pytest.mark.parametrize("guard", [0, 1, 4, 37])
def test_a_larger_cell_at_guard_is_skipped_and_at_guard_plus_one_taken(dev, guard):
    nsamp = 1000
    for c0 in (400, 2, nsamp - 3):
        for side in (1, -1):
            for distance, taken in ((guard, False), (guard + 1, True)):
                P = pr.random_surfaces(1, 3, nsamp).copy()
                P[0, 1, c0] = 1000.0
                P[0, 0, (c0 + side * distance) % nsamp] = 999.0 if distance else 1000.0
                peaks, _ = compare(dev, P, 2, guard)
                assert peaks[0, 0]["code_index"] == c0 or distance == 0
                assert (peaks[0, 1]["power"] == 999.0) == taken, (guard, c0, side, distance)


def test_zones_that_leave_a_single_column(dev):
    """Eight zones of three columns tile columns 0 .. 23 of 25: column 24 alone is kept, and the floor is its mean."""
    P = pr.random_surfaces(2, 71, 25).copy()
    for p in range(2):
        for j in range(8):
            P[p, (7 * j + p) % 71, 3 * j + 1] = 1000.0 - j
    peaks, floor = compare(dev, P, 8, 1)
    assert peaks[0]["code_index"].tolist() == [3 * j + 1 for j in range(8)] == peaks[1]["code_index"].tolist()
    assert floor["kept_columns"].tolist() == [1, 1]
    assert np.all(np.abs(floor["mean_power"] - P[:, :, 24].mean(axis=1)) <= pr.floor_bound(71, 1) * floor["mean_power"])
    # and the widest zones the limits allow: one zone of 2 * 32767 + 1 columns of 65536, one column kept
    big = pr.random_surfaces(1, 1, 65536)
    _, floor = compare(dev, big, 1, 32767)
    assert floor[0]["kept_columns"] == 1


# ------------------------------------------------------------------------------------------------ 4. refusals
def test_refusals_enqueue_nothing(dev):
    P = pr.random_surfaces(3, 2, 500)
    I, U = GJ_ERR_INVALID, GJ_ERR_UNSUPPORTED
    with dev.alloc(P.nbytes) as d_power, Guarded(dev, 16 * 3 * 8) as d_peaks, Guarded(dev, 16 * 3) as d_floor:
        d_power.upload(P)
        cases = [  # d_power, n_prn, n_freq, nsamp, k, guard, d_peaks, d_floor, status
            (0, 3, 2, 500, 2, 4, d_peaks, d_floor, I),                                  # null pointers
            (d_power, 3, 2, 500, 2, 4, 0, d_floor, I),
            (d_power, 3, 2, 500, 2, 4, d_peaks, 0, I),
            (d_power.ptr + 4, 3, 2, 499, 2, 4, d_peaks, d_floor, I),                    # not 8-byte aligned
            (d_power, 3, 2, 500, 2, 4, d_peaks.ptr + 4, d_floor, I),
            (d_power, 3, 2, 500, 2, 4, d_peaks, d_floor.ptr + 4, I),
            (d_power, 3, 2, 7, 1, 0, d_peaks, d_floor, U),                              # nsamp 8 .. 65536
            (d_power, 3, 2, 0, 1, 0, d_peaks, d_floor, U),
            (d_power, 3, 2, -500, 1, 0, d_peaks, d_floor, U),
            (d_power, 3, 2, 65537, 1, 0, d_peaks, d_floor, U),
            (d_power, 3, 0, 500, 2, 4, d_peaks, d_floor, U),                            # n_freq 1 .. 4096
            (d_power, 3, -2, 500, 2, 4, d_peaks, d_floor, U),
            (d_power, 3, 4097, 500, 2, 4, d_peaks, d_floor, U),
            (d_power, 0, 2, 500, 2, 4, d_peaks, d_floor, I),                            # n_prn >= 1
            (d_power, -3, 2, 500, 2, 4, d_peaks, d_floor, I),
            (d_power, 3, 2, 500, 0, 4, d_peaks, d_floor, U),                            # k 1 .. 8
            (d_power, 3, 2, 500, -1, 4, d_peaks, d_floor, U),
            (d_power, 3, 2, 500, 9, 4, d_peaks, d_floor, U),
            (d_power, 3, 2, 500, 2, -1, d_peaks, d_floor, I),                           # guard >= 0
            (d_power, 3, 2, 500, 2, 125, d_peaks, d_floor, I),                          # 2 * 251 = 502 >= 500
            (d_power, 3, 2, 500, 4, 62, d_peaks, d_floor, I),                           # 4 * 125 = 500: not < 500
            (d_power, 3, 2, 500, 1, 250, d_peaks, d_floor, I),                          # 501
            (d_power, 3, 2, 500, 8, 2 ** 31 - 1, d_peaks, d_floor, I),                  # k (2 guard + 1) past int32
        ]
        for c in cases:                                      # nothing written behind each one of them
            refused(dev, dev.acq_peaks_dev, [(c[:-1], c[-1])], d_peaks, d_floor)
        # accepted: the limits themselves (4 * 125 - 1 = 499 < 500; one zone of 499 columns)
        dev.acq_peaks_dev(d_power, 3, 2, 500, 8, 30, d_peaks, d_floor)                  # 8 * 61 = 488
        dev.acq_peaks_dev(d_power, 3, 2, 500, 1, 249, d_peaks, d_floor)
        dev.synchronize()
        d_peaks.check_pads("peaks")
        d_floor.check_pads("floor")
    compare(dev, P, 2, 4)                                                               # the next valid call gives the parity bits


# ------------------------------------------------------------------------------------------------ 5. the search
@pytest.fixture(scope="module")
def search(dev):
    s = gnss.AcqSearch(dev, prns=sorted(cr.E2E_PRNS + (1,)))         # PRNs 1 and 27 are not in the overpowered pair
    yield s
    s.close()


def test_peak_0_is_the_searchs_own_maximum(dev, search, g1_raw):
    """AcqSearch.peaks: peak 0 of every PRN is the max_power / code_index / freq_index that gj_acq_search_dev reports in the
    SAME call, bit for bit, with and without signals in the capture; the surface is the one a never-passing threshold
    gives (every PRN integrates all steps), and self.threshold and self.d_out are left alone."""
    for raw, first in ((cr.e2e_pair("mixed")[0], 0), (cr.e2e_pair("mixed")[0], 4097), (g1_raw, 0)):
        with dev.capture(raw) as cap:
            mark = np.full(search.d_out.nbytes, SENTINEL, np.uint8)
            search.d_out.upload(mark)
            peaks, results = search.peaks(cap, first, k=3, want_results=True)
            assert search.threshold == gnss.ACQ_THRESHOLD and np.array_equal(search.d_out.download(np.uint8), mark)
        assert [p.prn for p in peaks] == search.prns == [r.prn for r in results]
        gamma = gnss.peak_threshold(search.intg, len(search.freqs) * search.nsamp, 1e-3)
        for p, r in zip(peaks, results):
            assert p.steps == r.steps == search.intg and not r.acquired and len(p.peaks) == 3
            top = p.peaks[0]
            assert (np.float64(top.power).tobytes(), top.code_index, top.freq_index) == (np.float64(r.max_power).tobytes(), r.code_index, r.freq_index), p.prn
            assert top.doppler_hz == search.freqs[top.freq_index] and top.ratio == top.power / p.mean_power
            assert [q.significant for q in p.peaks] == [q.ratio > gamma for q in p.peaks]
            assert p.peaks[0].power >= p.peaks[1].power >= p.peaks[2].power > p.mean_power > 0.0
    with pytest.raises(gpsjam.GpsJamError) as e:
        with dev.capture(cr.e2e_pair("mixed")[0]) as cap:
            search.peaks(cap, k=9)
    assert e.value.status == GJ_ERR_UNSUPPORTED


# ------------------------------------------------------------------------------------------------ 6. end to end
def test_the_overpowered_pair_end_to_end(dev, search):
    """Every PRN in the air twice, the counterfeit copy 4 dB up.  ``scan`` sees one peak per PRN: whatever it acquires it
    flags, and that is all it can say.  ``scan_peaks`` finds all five PRNs twice, puts the five strong candidates in the
    arc, and returns the five authentic ones within one sample and one Doppler bin of the truth, phase, Doppler and C/N0
    within twice the CPU chain's error.  Three peaks per PRN are searched: no third one is significant, nor any of the
    absent PRNs 1 and 27."""
    raw_a, raw_b = pr.overpowered_pair()
    prns = [cr.E2E_PRNS[k] for k in pr.E2E_IDX]
    with dev.capture(raw_a) as a, dev.capture(raw_b) as b:
        uploads = gpsjam.Capture.uploads
        single = spoof.scan(dev, a, b, search, tol=cr.E2E_TOL)
        rep = spoof.scan_peaks(dev, a, b, search, k=3, tol=cr.E2E_TOL)
        assert gpsjam.Capture.uploads == uploads
    # the gap: one peak per PRN, the counterfeit one; a PRN whose copies share a Doppler bin may not be acquired at all
    print(f"scan: acquired {single.prns}, common {single.common_prns}, spoofed {single.spoofed}")
    assert set(single.common_prns) <= set(single.prns) <= set(prns)
    if single.spoofed is not None:
        assert single.spoofed is True and len(single.common_prns) >= 4
    assert [c.prn for c in rep.candidates] == [p for p in sorted(prns) for _ in (0, 1)], "all five PRNs twice, nothing else"
    assert rep.spoofed is True and rep.common_prns == sorted(prns)
    assert rep.common == [0, 2, 4, 6, 8] and rep.counterfeit == [rep.candidates[i] for i in rep.common], "the strong candidates are in the arc"
    assert [c.prn for c in rep.authentic] == sorted(prns) and rep.authentic == [rep.candidates[i] for i in (1, 3, 5, 7, 9)]
    bin_hz = float(search.freqs[1] - search.freqs[0])
    for c in rep.counterfeit:
        k = cr.E2E_PRNS.index(c.prn)
        d = abs(c.code_index - pr.spoof_code_index(k))
        assert min(d, 2048 - d) <= 1.0 and abs(c.doppler_hz - pr.spoof_doppler(k)) <= bin_hz
        assert abs(float(cr.wrap(c.phase - cr.E2E_SPOOF_PHASE))) < cr.E2E_TOL
    for c in rep.authentic:
        k = cr.E2E_PRNS.index(c.prn)
        d = abs(c.code_index - cr.E2E_CODE_INDEX[k])
        e_ph, e_dop, e_cn0 = abs(float(cr.wrap(c.phase - cr.E2E_AUTHENTIC[k]))), abs(c.doppler_hz - cr.E2E_DOPPLER[k]), abs(c.cn0_dbhz - cr.E2E_CN0[k])
        print(f"authentic PRN {c.prn}: code {c.code_index}, ratio {c.ratio:.2f}, phase {c.phase:+.4f} (error {e_ph:.4f}, tolerance {pr.E2E_TOL_PHASE}), "
              f"Doppler error {e_dop:.3f} Hz ({pr.E2E_TOL_DOPPLER}), C/N0 {c.cn0_dbhz:.2f} (error {e_cn0:.2f} dB, {pr.E2E_TOL_CN0}), coherence {c.coherence:.3f}")
        assert min(d, 2048 - d) <= 1.0 and abs(c.doppler_hz - cr.E2E_DOPPLER[k]) <= bin_hz, (c.prn, c.code_index, c.doppler_hz)
        assert e_ph <= pr.E2E_TOL_PHASE, (c.prn, c.phase)
        assert e_dop <= pr.E2E_TOL_DOPPLER, (c.prn, c.doppler_hz)
        assert e_cn0 <= pr.E2E_TOL_CN0, (c.prn, c.cn0_dbhz)


def test_the_authentic_pair_has_no_second_candidates(dev, search):
    raw_a, raw_b = cr.e2e_pair("authentic")
    with dev.capture(raw_a) as a, dev.capture(raw_b) as b:
        rep = spoof.scan_peaks(dev, a, b, search, k=2, tol=cr.E2E_TOL)
    assert [c.prn for c in rep.candidates] == sorted(cr.E2E_PRNS[k] for k in pr.E2E_IDX), "one candidate per PRN"
    assert rep.spoofed is False and len(rep.common_prns) < 4 and rep.counterfeit == [] == rep.authentic
