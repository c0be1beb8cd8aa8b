"""CPU side of the acquisition search's edge tests (tests/acq_edges/test_acq_gpu.py is the GPU side).

 * pins tests/acq_restatement.py: exactly against integer dot products (the definition, no FFT), and against the
   complex64 oracle (oracle.gpsjam_oracle) on every capture of tests/acq_edges_inputs.py: equal decisions wherever the
   case is clear, power within the oracle's own measured error;
 * measures that error -- the oracle against exact power, as a share of the array's maximum, per input family -- prints
   it and holds acq_edges_inputs.E64_MEASURED to it (the GPU gates are 8 x these figures; nothing here sees a GPU);
 * asserts the conditions on the inputs: every case of families (a) (b) (c) (e) (g) is clear, the special shapes the GPU
   tests rely on are there (code index 0 with ratio exactly 1, row[0] deciding inside the zone, cnt = 3, a pass at a
   step past 17, exact ties of a few cells, 0/0), and prints the smallest margins;
 * shows on the CPU that the two peak-test rules the suite never reached -- the row[0] seed and the wrapped zone --
   change the records of family (a) by far more than the GPU tests' tolerances when they are dropped.
"""
import math

import numpy as np
import pytest

import acq_edges_inputs as ai
import acq_restatement as ar
from gpsjam import gnss
from oracle import gpsjam_oracle as orc

ORACLE_PRNS = 4          # PRNs per case run through the (slow, pure-Python) oracle mixer


def oracle_search(case, prn):
    """orc.acq_search with the case's threshold, nsampchip and bin count (it fixes them at 3.0, the rate's own and the
    whole table): the same calls in the same order.  0/0 raises ZeroDivisionError there, as in orc.acq_search."""
    raw = np.asarray(case.raw, np.uint8)
    freqs = list(gnss.doppler_bins(0.0, case.hband))[:case.n_freq]
    codex = orc.acq_code_fft(prn, case.nsamp, case.fs)
    P = np.zeros(case.n_freq * case.nsamp, np.float64)
    res = None
    for i in range(case.intg):
        loc = case.first + i * case.nsamp
        data = (raw[2 * loc:2 * (loc + 2 * case.nsamp)].astype(np.int16) - 128).astype(np.int8)
        orc.acq_pcorrelator(data, 1.0 / case.fs, case.nsamp, freqs, 2 * case.nsamp, codex, P)
        res = orc.acq_check(P, case.nsamp, case.n_freq, case.nsampchip, case.ctime, float(np.float32(case.threshold)))
        res["steps"] = i + 1
        if res["acquired"]:
            break
    return res, P


def test_oracle_search_restated_here_is_the_oracles():
    case = ai.existing_cases()[0]
    for prn in (3, 8):
        a, Pa = oracle_search(case, prn)
        b, Pb = orc.acq_search(case.raw, case.first, prn)
        assert a == b and Pa.tobytes() == Pb.tobytes()


def test_exact_power_is_the_definition():
    """The integer dot products of test_acq_host.py::test_pcorrelator_restatement_against_the_definition (the oracle's
    own block-wise mixer, no FFT anywhere) at every 97th code phase of three Doppler bins, two steps: equal as integers."""
    rng = np.random.default_rng(11)
    nsamp, m, prn = 2048, 4096, 9
    raw = (rng.integers(-40, 41, 2 * (3 * nsamp + 7)) + 128).astype(np.uint8)
    first = 7
    got = ar.exact_power(raw, first, prn, 2.048e6, 2, 7000.0)
    assert got.shape == (2, 71, nsamp) and got.dtype == np.int64
    rcode = np.zeros(m, np.int64)
    rcode[:nsamp] = orc.acq_rescode(orc.acq_gencode_l1ca(prn), (1 / 2.048e6) * 1.023e6, nsamp)
    freqs = gnss.doppler_bins()
    ks = np.arange(0, nsamp, 97)
    for f in (18, 35, 41):                                   # -3400, 0 and 1200 Hz
        want = np.zeros(ks.size, np.int64)
        for step in range(2):
            loc = first + step * nsamp
            data = (raw[2 * loc:2 * (loc + m)].astype(np.int16) - 128).astype(np.int8)
            II, QQ = orc.acq_mixcarr_sse2(data, 1 / 2.048e6, m, float(freqs[f]))
            II, QQ = II.astype(np.int64), QQ.astype(np.int64)
            for j, k in enumerate(ks):
                re, im = int(np.dot(np.roll(II, -k), rcode)), int(np.dot(np.roll(QQ, -k), rcode))
                want[j] += re * re + im * im
            np.testing.assert_array_equal(got[step, f, ks], want)


def all_cases():
    zone = [c0.at(c0.first + e) for c0 in ai.zone_cases() for e in range(ai.ZONE_EPOCHS)]
    return (list(ai.existing_cases()) + zone + list(ai.steps_cases()) + list(ai.ragged_cases()) + list(ai.extreme_cases())
            + [ai.race_case(fs) for fs in ai.RATES])


def oracle_prns(case):
    """At most ORACLE_PRNS of the case's PRNs: the first ones, and of tests/test_acq_gpu.py's 32 the present 1, 9, 31."""
    uniq = list(dict.fromkeys(case.prns))
    if case.name == "g:2048 all 32":
        return [1, 8, 9, 31]
    return uniq[:ORACLE_PRNS]


def test_restatement_against_the_oracle_and_the_oracles_error():
    """Every capture of the inputs module through the complex64 oracle: same decisions as the exact restatement wherever
    the case is clear, and its power error against exact, as a share of the array's maximum, per family."""
    worst = {"noise": (0.0, None), "saturated": (0.0, None)}
    compared = 0
    for case in all_cases():
        if "prns one" in case.name or "prns three" in case.name:
            continue                                         # the same captures and PRNs as the list of forty
        ref = ai.reference(case)
        for prn in oracle_prns(case):
            steps = ref[prn]
            want = steps[-1]
            if math.isnan(want["peakr"]):                    # all bytes 128: every power 0, the C divides 0 by 0
                with pytest.raises(ZeroDivisionError):
                    oracle_search(case, prn)
                assert not want["P"].any()
                continue
            got, P = oracle_search(case, prn)
            if case.family == "saturated":                   # the candidate rule: exact ties are decided by rounding
                assert got["steps"] == want["steps"] and not got["acquired"]
                assert got["freqi"] * case.nsamp + got["codei"] in want["ties"], (case, prn, got)
                at = ar.check(want["P"], case.nsamp, case.n_freq, case.nsampchip, case.ctime, case.threshold,
                              cell=got["freqi"] * case.nsamp + got["codei"])
                np.testing.assert_allclose([got["maxP"], got["maxP2"], got["meanP"]], [at["maxP"], at["maxP2"], at["meanP"]],
                                           rtol=0, atol=ai.E64_MEASURED["saturated"] * want["maxP"])
            elif ar.is_clear(steps):
                assert (got["acquired"], got["steps"], got["codei"], got["freqi"]) == \
                       (want["acquired"], want["steps"], want["codei"], want["freqi"]), (case, prn, got)
                np.testing.assert_allclose([got["maxP"], got["maxP2"], got["meanP"], got["peakr"]],
                                           [want["maxP"], want["maxP2"], want["meanP"], want["peakr"]], rtol=1e-4)
                compared += 1
            if got["steps"] == want["steps"]:
                err = float(np.max(np.abs(P.reshape(want["P"].shape) - want["P"])) / want["P"].max())
                if err > worst[case.family][0]:
                    worst[case.family] = (err, (case.name, prn))
                assert err <= ai.E64_MEASURED[case.family], (case, prn, err)
    for fam, (err, where) in worst.items():
        print(f"oracle (complex64) against exact power, family {fam}: {err:.3e} of the array's maximum at {where}; "
              f"E64_MEASURED {ai.E64_MEASURED[fam]:.1e}, GATE {ai.GATE[fam]:.2e}")
    for fam, (err, where) in worst.items():
        assert ai.E64_MEASURED[fam] <= 1.25 * err, "E64_MEASURED is the measured figure, rounded up by at most a quarter"
        assert ai.GATE[fam] == 8.0 * ai.E64_MEASURED[fam] and ai.GATE[fam] <= ai.OLD_GATE
    assert compared >= 150
    print(f"exact power: largest rounding residual {ar.SEEN['residual']:.2e} (asserted < 1e-3), largest integer power "
          f"{ar.SEEN['power']:.3e} (asserted < 2^53 = 9.0e15)")
    print(f"{compared} clear (case, PRN) searches decided alike by the oracle and the exact restatement")


def smallest_margins(cases, skip_ratio=lambda case, prn: False):
    cell, ratio = (math.inf, None), (math.inf, None)
    for case in cases:
        for prn, steps in ai.reference(case).items():
            for s in steps:
                if s["cell_margin"] < cell[0]:
                    cell = (s["cell_margin"], (case.name, prn, s["steps"]))
                if not skip_ratio(case, prn) and s["ratio_margin"] < ratio[0]:
                    ratio = (s["ratio_margin"], (case.name, prn, s["steps"]))
    return cell, ratio


def report(label, cell, ratio):
    print(f"{label}: smallest cell margin {cell[0]:.3e} at {cell[1]}, smallest ratio margin {ratio[0]:.3e} at {ratio[1]}")
    assert cell[0] >= ar.CLEAR_CELL and ratio[0] >= ar.CLEAR_RATIO


def test_zone_inputs():
    """(a): the peak is where the stride-1 series puts it, every case is clear (code index 0 excepted: its ratio is 1 by
    construction), cnt is nsamp - 4 nsampchip - 1 wrapped or not, and row[0] decides where it must."""
    cases = []
    for c0 in ai.zone_cases():
        decided_by_row0, zone_holds_0 = [], 0
        for e in range(ai.ZONE_EPOCHS):
            case = c0.at(c0.first + e)
            cases.append(case)
            last = ai.reference(case)[ai.ZONE_PRN][-1]
            codei = ai.zone_code_index(case, e)
            assert last["codei"] == codei and last["freqi"] == 7, (case, last["codei"], last["freqi"])   # 400 Hz of -1000 .. 1000
            assert last["cnt"] == case.nsamp - 4 * case.nsampchip - 1
            row = last["P"][last["freqi"]]
            in_zone = not ar.kept(case.nsamp, codei, case.nsampchip)[0]
            zone_holds_0 += in_zone
            if codei == 0:
                assert last["peakr"] == 1.0 and last["maxP2"] == last["maxP"] and not last["acquired"] and last["steps"] == 3
            else:
                assert last["acquired"] and last["steps"] == 1
                if in_zone and last["maxP2"] == row[0]:
                    decided_by_row0.append(codei)
        assert zone_holds_0 == 2 * min(2 * case.nsampchip, 6) + 1  # every wrapped shape on both sides, and the peak at 0
        if case.nsamp == 2048:
            assert {1, 2047} <= set(decided_by_row0), (c0, decided_by_row0)   # next to the peak row[0] IS the second peak
        if case.nsampchip == 511:
            assert last["cnt"] == 3
    cell, ratio = smallest_margins(cases, skip_ratio=lambda case, prn: ai.reference(case)[prn][-1]["codei"] == 0)
    report("(a) zone", cell, ratio)


def test_many_step_inputs():
    """(b): strong in one step, absent never, the weak one at 512 samples first passes at a step of the summary kernel's
    second trip, under a threshold that lies clear of the running maximum before it and of the passing ratio."""
    for case in ai.steps_cases():
        ref = ai.reference(case)
        assert ref[ai.STEPS_STRONG][-1]["steps"] == 1 and ref[ai.STEPS_STRONG][-1]["acquired"]
        assert ref[ai.STEPS_ABSENT][-1]["steps"] == case.intg and not ref[ai.STEPS_ABSENT][-1]["acquired"]
        weak = ref[ai.STEPS_WEAK][-1]
        if case.nsamp == 512:
            passes = case.intg >= ai.STEPS_WEAK_PASSES
            assert weak["acquired"] == passes and weak["steps"] == (ai.STEPS_WEAK_PASSES if passes else case.intg), (case, weak["steps"])
    assert 17 < ai.STEPS_WEAK_PASSES <= 64
    assert any(s[-1]["acquired"] and 1 < s[-1]["steps"] < 17 for c in ai.steps_cases() for s in ai.reference(c).values())
    report("(b) many steps", *smallest_margins(ai.steps_cases()))


def test_ragged_inputs():
    for label, prns in ai.RAGGED_PRNS.items():
        assert len(prns) == {"one": 1, "three": 3, "forty with repeats": 40}[label]
    forty = ai.RAGGED_PRNS["forty with repeats"]
    assert len(set(forty)) == 5 and all(forty.count(p) > 1 for p in set(forty))
    assert {c.n_freq for c in ai.ragged_cases() if c.nsamp == 512} == {1, 2, 5, 9}
    assert {c.n_freq for c in ai.ragged_cases() if c.nsamp == 1024} == {1, 2, 5, 9}
    assert {c.n_freq for c in ai.ragged_cases() if c.nsamp == 2048} == {1, 9}
    verdicts = {ai.reference(c)[p][-1]["acquired"] for c in ai.ragged_cases() for p in c.prns}
    assert verdicts == {True, False}
    report("(c) ragged shapes", *smallest_margins(ai.ragged_cases()))


def test_race_inputs():
    for fs in ai.RATES:
        case = ai.race_case(fs)
        assert len(case.prns) == 32 and case.n_freq == 71
        assert not any(s[-1]["acquired"] for s in ai.reference(case).values())
    report("(e) the race", *smallest_margins([ai.race_case(fs) for fs in ai.RATES]))


def test_existing_inputs():
    """(g): tests/test_acq_gpu.py's captures were not chosen for clear margins.  The PRNs of EXISTING_NOT_CLEAR have two
    noise cells within 1e-3 of each other at some step (or, PRN 17 of the first capture, a ratio within 1e-2 of 3.0): the
    GPU test holds their POWER to the gate like everyone's and their records to nothing.  The list is exactly the PRNs
    that are not clear -- none is left out for another reason."""
    for case in ai.existing_cases():
        ref = ai.reference(case)
        not_clear = sorted(p for p in ref if not ar.is_clear(ref[p]))
        assert not_clear == sorted(ai.EXISTING_NOT_CLEAR[case.name]), (case, not_clear)
        for p in not_clear:
            print(f"(g) {case.name} PRN {p}: not clear, smallest margins "
                  f"{min(s['cell_margin'] for s in ref[p]):.2e} (cell) {min(s['ratio_margin'] for s in ref[p]):.2e} (ratio)")
    clear = [(c, p) for c in ai.existing_cases() for p in c.prns if p not in ai.EXISTING_NOT_CLEAR[c.name]]
    cell = min(s["cell_margin"] for c, p in clear for s in ai.reference(c)[p])
    ratio = min(s["ratio_margin"] for c, p in clear for s in ai.reference(c)[p])
    print(f"(g) existing inputs, {len(clear)} clear PRNs: smallest cell margin {cell:.3e}, smallest ratio margin {ratio:.3e}")
    assert cell >= ar.CLEAR_CELL and ratio >= ar.CLEAR_RATIO


def test_extreme_inputs():
    """(d): all bytes 128 is 0/0; every other capture gives finite records and a tie set of a few cells, so that "the
    reported cell is a candidate" still holds the kernel to something."""
    sizes = {}
    for case in ai.extreme_cases():
        for prn, steps in ai.reference(case).items():
            assert len(steps) == case.intg and not steps[-1]["acquired"]
            for s in steps:
                if "constant 128" in case.name and "127" not in case.name:
                    assert not s["P"].any() and (s["codei"], s["freqi"]) == (0, 0)
                    assert math.isnan(s["peakr"]) and math.isnan(s["cn0"]) and s["meanP"] == 0.0
                    continue
                assert all(math.isfinite(s[k]) for k in ("maxP", "maxP2", "meanP", "peakr", "cn0")) and s["maxP2"] > 0
                assert 1 <= s["ties"].size <= ai.TIE_SET_CAP, (case, prn, s["ties"].size)
                key = case.name.split(" ", 1)[1]
                sizes[key] = max(sizes.get(key, 0), int(s["ties"].size))
    print("(d) largest tie set per capture:", sizes)
    assert sizes["constant 0"] == sizes["constant 255"] == 8 and sizes["nyquist full scale"] == sizes["uniform bytes"] == 1


def test_dropped_rules_show_in_the_zone_cases():
    """The two rules of checkacquisition that no test reached, dropped ON THE CPU: the records of family (a) move by far
    more than the GPU tests' tolerance (GATE (1 + ratio) on the peak ratio).  The GPU tests were also run against kernels
    with these mutations: profiles/NOTES_acq_edges.md says which test turned red."""
    tol = lambda r: ai.GATE["noise"] * (1.0 + r)
    seed_hits, wrap_hits = [], []
    for c0 in ai.zone_cases():
        for e in range(ai.ZONE_EPOCHS):
            case = c0.at(c0.first + e)
            good = ai.reference(case)[ai.ZONE_PRN][-1]
            P = good["P"]
            for hits, kw in ((seed_hits, {"seed": False}), (wrap_hits, {"wrapped": False})):
                bad = ar.check(P, case.nsamp, case.n_freq, case.nsampchip, case.ctime, case.threshold, **kw)
                if abs(bad["peakr"] - good["peakr"]) > 1e3 * tol(good["peakr"]) or bad["cnt"] != good["cnt"]:
                    hits.append((case.nsamp, case.nsampchip, good["codei"]))
    assert (2048, 2, 1) in seed_hits and (2048, 2, 2047) in seed_hits and (2048, 2, 0) in seed_hits
    assert {(n, c) for n, c, _ in wrap_hits} >= {(2048, 2), (1024, 1), (2048, 1), (2048, 100), (2048, 511)}
    assert all(n != 512 for n, _, _ in wrap_hits)            # nsampchip 0: the zone is the peak alone and never wraps
    print(f"seed dropped: {len(seed_hits)} zone epochs change; wrapped rule dropped: {len(wrap_hits)} change")
