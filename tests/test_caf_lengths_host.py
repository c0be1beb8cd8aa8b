"""CPU side of the cross-ambiguity search's length and shift-edge tests (tests/caf_lengths/test_round6_gpu.py): the
float64 yardstick ``sweep_bins`` is held to the two existing evaluations of the definition, the table of cases is pinned,
and the preconditions the GPU tests rest on -- the planted (lag, bin) is the reference's answer, NO searched cell is a
near tie, the runner-up bin stands clear -- are asserted for every case whose reference is affordable here (L <= 2^20;
the GPU tests assert the same on the references they compute for the longer ones).  The margins found are printed, and
noted in profiles/NOTES_caf_lengths.md.  No GPU call is made."""
import time

import numpy as np
import pytest
from scipy import signal

import caf_lengths_inputs as ci
import caf_restatement as caf
import k5_check as k5
from gpsjam import _ffi

HOST_MAX_L = 1 << 20


# ------------------------------------------------------------------ the yardstick
def test_sweep_bins_is_the_sweep_on_a_range_and_the_definition_anywhere():
    n = 3000
    a0, a1 = caf.make_antennas(n, [(0, 0.0), (-9, 17.0)], seed=5)
    first, nb = 12, 9
    assert ci.sweep_bins(a1, a0, range(first, first + nb)) == caf.sweep(a1, a0, first, nb)
    L = caf.fft_len(n)
    far = [-(L // 2 - 1), -4097, -17, -1, 0, 1, 16, 17, 4095, L // 2 - 1]
    got = ci.sweep_bins(a1, a0, far[::-1])[::-1]                       # the order of the list is the order of the answer
    for b, r in zip(far, got):
        d = caf.direct_bin(a1, a0, b)
        assert r.lag == d.lag or r.margin < caf.LAG_NEAR_TIE, (b, r, d)
        np.testing.assert_allclose([r.peak, r.margin], [d.peak, d.margin], rtol=1e-5, atol=1e-6)
    # the other unpack convention, against the words of the header taken literally
    xj, xi = ci.unpack(a1, 128.0), ci.unpack(a0, 128.0)
    assert xj[0] == complex(float(a1[0]) - 128.0, float(a1[1]) - 128.0)
    c = signal.correlate(xj * np.exp(-2j * np.pi * 17 * np.arange(n) / L), xi, mode="full")
    r = ci.sweep_bins(a1, a0, [17], offset=128.0)[0]
    assert r.lag == int(np.argmax(np.abs(c))) - (n - 1) == -9
    np.testing.assert_allclose(r.peak, np.abs(c).max(), rtol=1e-12)
    assert ci.unpack(a1).astype(np.complex64).tobytes() == caf.unpack(a1).tobytes()      # the default is caf's


def test_winner_of_a_list_keeps_the_tie_rule():
    recs = [caf.BinPeak(1, 2.0, 0.5), caf.BinPeak(2, 3.0, 0.4), caf.BinPeak(3, 3.0, 0.3), caf.BinPeak(4, 1.0, 0.2)]
    s = ci.winner_of([-7, -2, 40, 41], recs)
    assert (s.lag, s.bin, s.peak, s.margin_lag, s.margin_bin) == (2, -2, 3.0, 0.4, 0.0)      # the earlier of two equal bins
    # all-zero slices under offset 128: |c| is 0 everywhere -- the earliest bin, the smallest m, margins 0
    z = np.full(2 * 50, 128, np.uint8)
    s = ci.search_bins(z, z, list(range(-3, 4)), offset=128.0)
    assert (s.lag, s.bin, s.peak, s.margin_lag, s.margin_bin) == (-49, -3, 0.0, 0.0, 0.0)
    assert all((r.lag, r.peak) == (-49, 0.0) for r in s.bins)


# ------------------------------------------------------------------ 1: the table
def test_the_table_reaches_every_column_kernel_at_both_edges_of_its_bucket():
    cases = ci.LENGTH_CASES
    ids = [c.id for c in cases]
    assert len(ids) == len(set(ids)) == 6 * 2 * 9 + 3 * 4
    for L in ci.LENGTHS:
        L1, half = L // 4096, L // 2
        mine = [c for c in cases if c.L == L]
        assert {c.n for c in mine} == {L // 4 + 1, L // 2} and all(caf.fft_len(c.n) == L for c in mine)
        assert all(-half < b < half for c in mine for b in c.searched)
        assert all(c.delay != 0 and abs(c.delay) < 20 for c in mine)
        if L <= ci.FULL_MAX_L:
            for n in (L // 4 + 1, L // 2):
                sub = [c for c in mine if c.n == n]
                assert [c.bin for c in sub] == ci.edge_bins(L) and len({c.delay for c in sub}) == 9
                assert all(c.thin == "" for c in sub)
        else:
            assert [(c.n, c.bin, c.thin) for c in mine] == [(half, L1 + 1, "thin3of9"), (half, -1, "thin3of9"),
                                                            (half, half - 1, "thin3of9"), (L // 4 + 1, -1, "thin1of9")]
            assert all("thin" in c.id for c in mine)
    assert [L // 4096 for L in ci.LENGTHS] == [16, 32, 64, 128, 256, 512, 1024, 2048, 4096]
    # the shift's edges: bin -1 carries in every row but the first and wraps the rotation; the largest bins are searched alone
    c = next(c for c in cases if c.L == 1 << 16 and c.bin == -1)
    assert c.searched == [-2, -1, 0] and (-1) % 16 == 15 and ((-1) % (1 << 16)) // 16 == 4095
    assert next(c for c in cases if c.L == 1 << 16 and c.bin == 32767).searched == [32767]


@pytest.mark.parametrize("L", [L for L in ci.LENGTHS if L <= HOST_MAX_L], ids=lambda L: f"L1={L // 4096}")
def test_no_searched_cell_is_a_near_tie_and_the_runner_up_bin_stands_clear(L):
    t0 = time.time()
    low = {}
    for case in (c for c in ci.LENGTH_CASES if c.L == L):
        want = ci.length_reference(case, ci.length_capture(case))      # asserts the preconditions
        lag_m = min(r.margin for r in want.bins)
        cur = low.setdefault(case.n, [1.0, 1.0])
        cur[0] = min(cur[0], lag_m)
        if len(want.bins) > 1:
            cur[1] = min(cur[1], want.margin_bin)
        else:
            assert want.margin_bin == 1.0
    for n, (lag_m, bin_m) in sorted(low.items()):
        print(f"L = 2^{L.bit_length() - 1} n = {n}: smallest lag margin {lag_m:.4f} (needs {ci.LAG_NEAR_TIE:g}), "
              f"smallest bin margin {bin_m:.4f} (needs {ci.GAP:g})")
        # the probe of this construction: lag margins of 0.96 and more, bin margins about 0.098 at n = L/4 + 1 (a
        # one-bin offset is a quarter cycle across the slice) and 0.36 at n = L/2
        assert lag_m > 0.9 and 0.08 < bin_m < 0.45
    print(f"L = 2^{L.bit_length() - 1}: {time.time() - t0:.1f} s of float64 reference")


# ------------------------------------------------------------------ 2: planted peaks under a bin (the size affordable here)
def test_a_planted_burst_keeps_its_lag_and_margin_under_a_bin():
    n = ci.PLANT_N[0]
    assert caf.fft_len(n) == 2 * n == 1 << 16
    for b in ci.plant_bins(n):
        rng = np.random.default_rng(n + b)
        low = 1.0
        for lag in k5.k5_edge_lags(n):
            s0, s1 = k5.k5_planted(n, lag, rng, width=1 if abs(lag) >= n - 2 else None)
            Z0, Z1 = ci.spectrum(s0), ci.spectrum(s1)
            fwd, rev = ci.bin_of_spectra(Z1, Z0, b, n), ci.bin_of_spectra(Z0, Z1, b, n)
            assert (fwd.lag, rev.lag) == (lag, -lag), (b, lag, fwd, rev)
            low = min(low, fwd.margin, rev.margin)
        print(f"n = {n} bin {b}: smallest margin of a planted peak {low:.4f} (needs {ci.GAP:g})")
        assert low > ci.GAP
    assert ci.plant_bins(n) == [17, -1] and ci.plant_bins(ci.PLANT_N[1]) == [2049, -1]
    assert ci.PLANT_N == k5.K5_PLANT_N


# ------------------------------------------------------------------ 3: the clip, on the host
def test_a_request_above_the_counters_is_clipped_to_688_per_pair():
    """gj_xcorr_caf_workspace is host arithmetic and grows with the bins of a launch: a clip that gave way would show
    here, without a launch whose column workgroups count arrivals behind the sync area."""
    lib = _ffi.load()

    def ws(n_pairs, n_bins, bpl, n_ant=3, n=ci.CLIP_N):
        return lib.gj_xcorr_caf_workspace(None, n_ant, n, n_pairs, n_bins, bpl)

    nb = ci.CLIP_BINS[1]
    assert ci.CLIP_WORDS // 7 == 98 and nb == 129
    assert ws(7, nb, 4096) == ws(7, nb, 99) == ws(7, nb, 98) > ws(7, nb, 97) > ws(7, nb, 1) > 0
    assert ws(1, 4096, 4096) == ws(1, 4096, 689) == ws(1, 4096, 688) > ws(1, 4096, 687)
    assert ws(136, 129, 4096) == ws(136, 129, 5) > ws(136, 129, 4), "688 // 136 = 5"
    assert ws(7, 50, 4096) == ws(7, 50, 50) > ws(7, 50, 49), "never more than the call has"


# ------------------------------------------------------------------ 4: the largest call
def test_the_largest_calls_subset_holds_its_winner_and_runner_up():
    bins = ci.big_subset()
    last = ci.BIG_FIRST + ci.BIG_BINS - 1
    assert ci.BIG_BINS == _ffi.GJ_CAF_MAX_BINS and len(bins) <= 64 and {ci.BIG_FIRST, last} <= set(bins)
    seams = range(ci.BIG_FIRST + ci.BIG_BATCH, last, ci.BIG_BATCH)
    assert len(seams) == 15 and all(s - 1 in bins and s in bins for s in seams)
    assert (ci.BIG_BIN - ci.BIG_FIRST) // ci.BIG_BATCH == 15, "the winner lies in the last batch"
    assert (128 << 20) // (caf.fft_len(ci.BIG_N) * 8) == ci.BIG_BATCH < ci.CLIP_WORDS
    a0, a1 = ci.big_capture()
    want = ci.search_bins(a1, a0, bins)
    low = ci.assert_no_near_tie(want, "largest call")
    print(f"largest call: winner {(want.lag, want.bin)} margin_lag {want.margin_lag:.4f} margin_bin {want.margin_bin:.3e}; "
          f"smallest lag margin of the {len(bins)} cells {low:.4f}")
    assert (want.lag, want.bin) == (ci.BIG_LAG, ci.BIG_BIN)
    # a neighbouring bin keeps 1 - (pi n / L)^2 / 6 = 1 - 3.8e-4 of the peak: the gap must still be many float32 ulps
    assert 2e-4 < want.margin_bin < 6e-4
    # the subset's runner-up bin is the runner-up of the whole range: every bin within 200 of the winner, evaluated
    # (further off, |sinc(x)| <= 1 / (pi x) = 0.11 at x = n 200 / L bounds the planted source and the rest is noise)
    near = list(range(ci.BIG_BIN - 200, last + 1))
    peaks = np.array([r.peak for r in ci.sweep_bins(a1, a0, near)])
    order = np.argsort(-peaks)
    assert near[order[0]] == ci.BIG_BIN and abs(near[order[1]] - ci.BIG_BIN) == 1
    np.testing.assert_allclose(1.0 - peaks[order[1]] / peaks[order[0]], want.margin_bin, rtol=1e-9)


# ------------------------------------------------------------------ 5: the three-antenna case at L1 = 64
@pytest.mark.parametrize("offset", [127.5, ci.GNSSDEC[0]])
def test_the_slot_case_under_both_conventions(offset):
    assert caf.fft_len(ci.SLOT_N) // 4096 == 64
    assert [ci.slot_truth(p) for p in ci.SLOT_PAIRS] == [(4, 65), (-6, 1), (-10, -64)]
    raws = ci.slot_capture()
    for p in ci.SLOT_PAIRS:
        want = ci.slot_reference(raws, p, offset)                      # asserts truth and no near tie
        print(f"offset {offset} pair {p}: {want[:5]}, smallest lag margin {min(r.margin for r in want.bins):.4f} over "
              f"{len(want.bins)} bins")
        assert want.margin_bin > ci.GAP and want.margin_lag > 0.5
