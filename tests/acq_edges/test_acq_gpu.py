"""The acquisition search (gj_acq_search_dev in both forms, gj_acq_series_dev) at the edges of its peak test, on EXACT power.

This file sits in a package next to the acquisition stage on purpose, like tests/acq_series/: the suite orders GPU files by
basename (tests/conftest.py SUITE_ORDER), and under the name test_acq_gpu.py it runs in stage 2 with the search it tests.

The reference is tests/acq_restatement.py -- the correlation as the integers it is, checkacquisition in float64 -- on the
captures of tests/acq_edges_inputs.py; tests/test_acq_edges_host.py pins both on the CPU, measures the complex64 oracle's
error against exact power (E64_MEASURED) and asserts that every case of families (a) (b) (c) (e) (g) is clear.

Gates.  Power: |P_gpu - P_exact| <= GATE max(P_exact) per (PRN, step array), GATE = 8 x E64_MEASURED of the family (a
second correct complex64 chain with another butterfly order and table rounding): 3.2e-6 on the noise captures, 2.16e-5 on
the saturated ones, against the 2e-4 of tests/test_acq_gpu.py.  Records, from the same gate: max, second and mean power
absolute GATE max_power (a mean of cells is no further off than its worst cell); the ratio r = max / second relative
GATE (1 + r) (both terms off by GATE max: dr / r <= GATE + GATE r); cn0 = 10 log10(max / mean / ctime) absolute
(10 / ln 10) GATE (1 + max / mean).  Indices, steps and the verdict are exact: the cases are clear.

"step form" = acq_inv_kernel + acq_check_kernel (a power array is asked for), "single launch" = acq_inv_all_kernel +
acq_summary_kernel (none is), "series" = the single launch with the epoch on grid.y.
"""
import numpy as np
import pytest

import acq_edges_inputs as ai
import acq_restatement as ar
from gpsjam import gnss

pytestmark = pytest.mark.gpu

REC, RECORD = ai.REC, ai.RECORD
records, check_record, check_values, check_power = ai.records, ai.check_record, ai.check_values, ai.check_power


def searcher(dev, case):
    srch = gnss.AcqSearch(dev, prns=case.prns, fs=case.fs, intg=case.intg, threshold=case.threshold, hband=case.hband)
    assert srch.nsamp == case.nsamp and srch.ctime == case.ctime
    srch.nsampchip = case.nsampchip            # the rate's own unless the case overrides it
    srch.freqs = srch.freqs[:case.n_freq]      # the first rows of the phase table [n_freq][m] are a table of their own
    return srch


def single_launch(dev, srch, cap, nbytes, first):
    srch.search_dev(cap, nbytes, first)
    dev.synchronize()
    return srch.d_out.download(np.uint8, REC * len(srch.prns)).tobytes()


def step_form(dev, srch, cap, nbytes, first):
    """(record bytes, P [n_prn][n_freq][nsamp]): a PRN's rows are frozen at the step that acquires it."""
    shape = (len(srch.prns), len(srch.freqs), srch.nsamp)
    with dev.alloc(8 * int(np.prod(shape))) as d_power:
        srch.search_dev(cap, nbytes, first, d_power)
        dev.synchronize()
        return srch.d_out.download(np.uint8, REC * len(srch.prns)).tobytes(), d_power.download(np.float64).reshape(shape)


def series(dev, srch, cap, nbytes, first, stride, n_epochs):
    with dev.alloc(REC * n_epochs * len(srch.prns)) as d_out:
        dev.reserve(srch.series_workspace(n_epochs))
        srch.series_dev(cap, nbytes, first, stride, n_epochs, d_out)
        dev.synchronize()
        raw = d_out.download(np.uint8, REC * n_epochs * len(srch.prns)).tobytes()
    return [raw[e * REC * len(srch.prns):(e + 1) * REC * len(srch.prns)] for e in range(n_epochs)]


def check_clear_case(dev, case, cap, nbytes=None, skip=()):
    """Both forms of one search against the restatement: every record, and the step form's power.  PRNs in `skip`: power
    only."""
    ref = ai.reference(case)
    srch = searcher(dev, case)
    nbytes = cap.nbytes if nbytes is None else nbytes
    try:
        fast = records(single_launch(dev, srch, cap, nbytes, case.first))
        slow_raw, P = step_form(dev, srch, cap, nbytes, case.first)
        slow = records(slow_raw)
    finally:
        srch.close()
    worst = 0.0
    for k, prn in enumerate(case.prns):
        want = ref[prn][-1]
        worst = max(worst, check_power(P[k], want, case, (case, prn)))
        if prn in skip:
            continue
        check_record(fast[k], want, case, (case, prn, "single launch"))
        check_record(slow[k], want, case, (case, prn, "step form"))
    print(f"{case}: step-form power within {worst:.2e} of exact (gate {case.gate:.2e})")
    return fast, slow


# ------------------------------------------------------------------------------------------- (a) the zone and the seed
@pytest.mark.parametrize("c0", ai.zone_cases(), ids=repr)
def test_zone_and_seed(dev, c0):
    """The code index walks 6 .. 0, nsamp - 1 .. nsamp - 6 through a stride-1 series: every wrapped shape of the exclusion
    zone on both sides, row[0] inside the zone (where it seeds maxvd whatever the zone says) and AT the peak (ratio
    exactly 1: the seed is the maximum itself).  The series and a loop of step-form searches against the restatement."""
    srch = searcher(dev, c0)
    worst = 0.0
    try:
        with dev.capture(c0.raw) as cap:
            epochs = series(dev, srch, cap, cap.nbytes, c0.first, 1, ai.ZONE_EPOCHS)
            for e in range(ai.ZONE_EPOCHS):
                case = c0.at(c0.first + e)
                want = ai.reference(case)[ai.ZONE_PRN][-1]
                slow_raw, P = step_form(dev, srch, cap, cap.nbytes, case.first)
                worst = max(worst, check_power(P[0], want, case, (case, "step form")))
                for form, raw in (("series", epochs[e]), ("step form", slow_raw)):
                    got = records(raw)[0]
                    assert int(got["code_index"]) == ai.zone_code_index(case, e), (case, form, got)
                    if want["codei"] == 0:
                        # the peak at index 0 seeds its own second peak: 1.0 bit for bit, never acquired
                        assert got["peak_ratio"] == 1.0 and got["second_power"] == got["max_power"], (case, form, got)
                        assert not got["acquired"] and got["steps"] == case.intg and got["freq_index"] == want["freqi"]
                        check_values(got, want, case, (case, form))
                        continue
                    check_record(got, want, case, (case, form))
                    row0 = want["P"][want["freqi"], 0]
                    if not ar.kept(case.nsamp, want["codei"], case.nsampchip)[0] and want["maxP2"] == row0:
                        assert abs(got["second_power"] - row0) <= case.gate * want["maxP"], (case, form, got, row0)
                    assert want["cnt"] == case.nsamp - 4 * case.nsampchip - 1
    finally:
        srch.close()
    print(f"{c0}: step-form power within {worst:.2e} of exact over {ai.ZONE_EPOCHS} epochs (gate {c0.gate:.2e})")


# ------------------------------------------------------------------------------------------- (b) many steps
@pytest.mark.parametrize("case", ai.steps_cases(), ids=repr)
def test_many_steps(dev, case):
    """intg up to 64: the summary kernel's waves take steps w, w + 16, ... -- a second, third and fourth trip -- and win[]
    fills to its 64 entries.  A strong satellite stops at step 1, an absent PRN runs them all, the weak one passes at
    step 31 of 64 (and at none of 16 or 17)."""
    with dev.capture(case.raw) as cap:
        fast, _ = check_clear_case(dev, case, cap)
    steps = {prn: int(fast[k]["steps"]) for k, prn in enumerate(case.prns)}
    assert steps[ai.STEPS_STRONG] == 1 and steps[ai.STEPS_ABSENT] == case.intg
    if case.nsamp == 512:
        assert steps[ai.STEPS_WEAK] == min(case.intg, ai.STEPS_WEAK_PASSES)


# ------------------------------------------------------------------------------------------- (c) ragged shapes
@pytest.mark.parametrize("case", ai.ragged_cases(), ids=repr)
def test_ragged_shapes(dev, case):
    """n_freq that does not fill a workgroup's 2 or 4 transforms (dead transforms vote through sh_need), one bin, one
    PRN, a PRN count that is no friendly number; every repeat of a PRN gives the bytes of its first occurrence."""
    with dev.capture(case.raw) as cap:
        fast, slow = check_clear_case(dev, case, cap)
    for form in (fast, slow):
        first_seen = {}
        for k, prn in enumerate(case.prns):
            k0 = first_seen.setdefault(prn, k)
            assert form[k].tobytes() == form[k0].tobytes(), (case, prn, k, k0)


# ------------------------------------------------------------------------------------------- (d) degenerate captures
@pytest.mark.parametrize("case", ai.extreme_cases(), ids=repr)
def test_degenerate_and_saturated(dev, case):
    """All bytes 128: every power is 0 and the C divides 0 by 0 -- NaN, not acquired, all steps run.  The others: exact
    ties (8 cells on the constants) are decided by rounding, so each form's reported cell must be A CANDIDATE of the
    restatement's tie set and its record the restatement's AT THAT CELL; each form is held to this, not to the other."""
    ref = ai.reference(case)
    srch = searcher(dev, case)
    try:
        with dev.capture(case.raw) as cap:
            fast = records(single_launch(dev, srch, cap, cap.nbytes, case.first))
            slow_raw, P = step_form(dev, srch, cap, cap.nbytes, case.first)
    finally:
        srch.close()
    for k, prn in enumerate(case.prns):
        want = ref[prn][-1]
        if not want["P"].any():
            assert not P[k].any()
            for form, got in (("single launch", fast[k]), ("step form", records(slow_raw)[k])):
                assert got["max_power"] == 0.0 and got["second_power"] == 0.0 and got["mean_power"] == 0.0, (case, form, got)
                assert (got["code_index"], got["freq_index"]) == (0, 0), (case, form, got)
                assert np.isnan(got["peak_ratio"]) and np.isnan(got["cn0"]), (case, form, got)
                assert not got["acquired"] and got["steps"] == case.intg, (case, form, got)
            continue
        err = check_power(P[k], want, case, (case, prn))
        for form, got in (("single launch", fast[k]), ("step form", records(slow_raw)[k])):
            assert all(np.isfinite(got[f]) for f in ("max_power", "second_power", "mean_power", "peak_ratio", "cn0")), (case, form, got)
            assert not got["acquired"] and got["steps"] == case.intg, (case, form, got)
            cell = int(got["freq_index"]) * case.nsamp + int(got["code_index"])
            assert cell in want["ties"], (case, prn, form, cell, want["ties"])
            at = ar.check(want["P"], case.nsamp, case.n_freq, case.nsampchip, case.ctime, case.threshold, cell=cell)
            check_values(got, at, case, (case, prn, form))
        print(f"{case} PRN {prn}: step-form power within {err:.2e} of exact (gate {case.gate:.2e}), tie set {want['ties'].size}")


# ------------------------------------------------------------------------------------------- (e) the race
@pytest.mark.parametrize("fs", ai.RATES)
def test_race_does_not_show(dev, fs):
    """Noise only, 32 PRNs x 71 bins: no row stands out, so many rows raise gmax in whatever order they arrive.  Sixteen
    single launches and five stride-0 epochs of a series give the same BYTES; the verdicts are the step form's and the
    restatement's."""
    case = ai.race_case(fs)
    with dev.capture(case.raw) as cap:
        fast, _ = check_clear_case(dev, case, cap)
        srch = searcher(dev, case)
        try:
            runs = [single_launch(dev, srch, cap, cap.nbytes, case.first) for _ in range(ai.RACE_RUNS)]
            epochs = series(dev, srch, cap, cap.nbytes, case.first, 0, 5)
        finally:
            srch.close()
    assert all(r == fast.tobytes() for r in runs)
    assert all(e == fast.tobytes() for e in epochs)


# ------------------------------------------------------------------------------------------- (f) past byte 2^32
def test_past_byte_2_32(dev):
    """The window at sample 2^31 + 1 of one allocation of 4 GiB + 1 MiB (never filled: only the window is read): the bytes
    of the same window searched as a small capture of its own -- both forms, and a two-epoch series."""
    case = ai.existing_cases()[0].at(1)
    raw = case.raw
    assert 2 * ai.FAR_SAMPLE + raw.size <= ai.BIG and 2 * ai.FAR_FIRST > 2 ** 32
    assert 2 * (1 + ai.FAR_STRIDE + (case.intg + 1) * case.nsamp) <= raw.size
    srch = searcher(dev, case)
    try:
        with dev.capture(raw) as cap:
            near = (single_launch(dev, srch, cap, cap.nbytes, 1), *step_form(dev, srch, cap, cap.nbytes, 1),
                    series(dev, srch, cap, cap.nbytes, 1, ai.FAR_STRIDE, 2))
        big = dev.alloc(ai.BIG)
        try:
            assert big.ptr and big.nbytes == ai.BIG
            big.upload(raw, offset=2 * ai.FAR_SAMPLE)
            assert big.download(np.uint8, 64, offset=2 * ai.FAR_SAMPLE).tobytes() == raw[:64].tobytes()
            far = (single_launch(dev, srch, big, ai.BIG, ai.FAR_FIRST), *step_form(dev, srch, big, ai.BIG, ai.FAR_FIRST),
                   series(dev, srch, big, ai.BIG, ai.FAR_FIRST, ai.FAR_STRIDE, 2))
        finally:
            big.free()
    finally:
        srch.close()
    assert far[0] == near[0] and far[1] == near[1] and far[2].tobytes() == near[2].tobytes() and far[3] == near[3]
    assert near[3][0] == near[0]                                   # epoch 0 of the series is the single search


# ------------------------------------------------------------------------------------------- (g) the existing inputs
@pytest.mark.parametrize("case", ai.existing_cases(), ids=repr)
def test_existing_inputs_at_the_gate(dev, case):
    """tests/test_acq_gpu.py's captures at GATE instead of its 2e-4: the step form's power of every PRN, both forms' records
    of every PRN that is clear (ai.EXISTING_NOT_CLEAR lists the others; the host test asserts the list is exactly those)."""
    with dev.capture(case.raw) as cap:
        check_clear_case(dev, case, cap, skip=ai.EXISTING_NOT_CLEAR[case.name])

