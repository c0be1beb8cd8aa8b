"""CPU checks of the two restatements the GPU tests in tests/floor_result hold the library to.

tests/floor_restatement.py: the restated baseline IS numpy.percentile, bit for bit, on every map the GPU tests use (the
grid, the short maps, the sensitive maps, the special maps, the captures' exact power maps); the maps listed as sensitive
really separate a once-rounded lerp from numpy's, and there are as many as the GPU tests count on.

tests/result_restatement.py: the restated result vector is gpsjam.sharded.pack_results (torch on the CPU) element for
element; the float32 order the packing kernel adds in stays within the derived bound of the float64 mean."""
from fractions import Fraction

import numpy as np
import pytest

import exact_restatement as ex
import floor_restatement as fr
import result_restatement as rr


def same_f32(got, want) -> bool:
    """Bit for bit, except that any NaN equals any NaN and a zero's sign does not matter (the rule turns both into 1.0)."""
    got, want = np.float32(got), np.float32(want)
    if np.isnan(want) or np.isnan(got):
        return bool(np.isnan(want) and np.isnan(got))
    return bool(got == want)


def numpy_rule(pm, pct):
    with np.errstate(invalid="ignore", over="ignore"), np.testing.suppress_warnings() as sup:
        sup.filter(RuntimeWarning)
        got = np.percentile(pm, float(pct))
    assert got.dtype == np.float32
    return got


# --------------------------------------------------------------------------------------- the floor rule
@pytest.mark.parametrize("kind", fr.KINDS)
def test_restated_baseline_is_numpy_on_the_grid(kind):
    for n in fr.GRID_N:
        pm = fr.grid_map(kind, n)
        assert pm.dtype == np.float32 and pm.size == n
        for pct in fr.GRID_PCT:
            assert same_f32(fr.baseline(pm, pct), numpy_rule(pm, pct)), (kind, n, pct)


def test_restated_baseline_is_numpy_on_the_short_and_sensitive_maps():
    assert len(fr.short_maps()) == 63 * 8
    for n, k in fr.short_maps():
        pm = fr.short_map(n, k)
        assert pm.size == n and pm.max() / pm.min() <= 10.0
        for pct in fr.SHORT_PCT + (0.1, 33.3, 95):
            assert same_f32(fr.baseline(pm, pct), numpy_rule(pm, pct)), (n, k, pct)
    for n, seed, pct in fr.SENSITIVE_MAPS:
        pm = fr.short_map(n, seed)
        assert same_f32(fr.baseline(pm, pct), numpy_rule(pm, pct)), (n, seed, pct)


def test_restated_baseline_is_numpy_on_the_special_maps():
    sm = fr.special_maps()
    for name, (pm, pcts) in sm.items():
        for pct in pcts:
            assert same_f32(fr.baseline(pm, pct), numpy_rule(pm, pct)), (name, pct)
    for where in ("first", "middle", "last"):
        pm, pcts = sm[f"nan {where}"]
        for pct in pcts:
            base, thr, count, mask = fr.floor_rule(pm, pct, 6)
            assert np.isnan(base) and np.isnan(thr) and count == 0 and not mask.any()
    pm, pcts = sm["all negative"]
    for pct in pcts:
        base, thr, count, mask = fr.floor_rule(pm, pct, 6)
        assert base == 1.0 and thr == fr.ratio_of(6) and count == 0
    assert np.isposinf(np.sort(sm["+inf largest"][0])[-1]) and np.isneginf(np.sort(sm["-inf smallest"][0])[0])
    assert np.signbit(sm["signed zeros"][0][3]) and not np.signbit(sm["signed zeros"][0][4])


def test_rounding_helper_rounds_to_nearest_even():
    one, ulp = Fraction(1), Fraction(1, 1 << 23)
    assert fr._round_f32(one + ulp / 2) == np.float32(1.0)                          # tie: the even neighbour is below
    assert fr._round_f32(one + 3 * ulp / 2) == np.float32(1.0) + np.float32(2.0 ** -22)   # tie: the even one is above
    assert fr._round_f32(one + ulp / 2 + Fraction(1, 1 << 60)) == np.nextafter(np.float32(1), np.float32(2))
    # a lerp whose product is exact: both evaluations round the same sum
    a, b, g = np.float32(1.0), np.float32(1.0) + np.float32(2.0 ** -22), np.float32(0.375)
    assert fr.lerp(a, b, g) == np.float32(1.0) + np.float32(2.0 ** -23)
    assert fr.once_rounded(a, b, g) == np.float32(1.0) + np.float32(2.0 ** -23)
    assert fr.lerp(np.float32(3), np.float32(5), np.float32(0.75)) == np.float32(4.5)


def test_the_sensitive_maps_are_sensitive():
    maps = fr.SENSITIVE_MAPS
    assert len(maps) >= 32 and len(set(maps)) == len(maps)
    assert sum(1 for m in maps if m[2] == 5) >= 8
    for n, seed, pct in maps:
        assert 2 <= n <= 64
        pm = fr.short_map(n, seed)
        a, b, g = fr.neighbours(pm, pct)
        assert fr.once_rounded(a, b, g) != fr.lerp(a, b, g), (n, seed, pct)
        # one unit in the last place apart, never more
        assert abs(int(fr.once_rounded(a, b, g).view(np.int32)) - int(fr.lerp(a, b, g).view(np.int32))) == 1
    # a power-of-two quantile leaves g a multiple of 1/4: the product is exact and no map can be sensitive
    assert not any(fr.is_sensitive(fr.short_map(n, k), 25) for n, k in fr.short_maps())


def test_the_captures_power_maps():
    caps = fr.SENSITIVE_CAPTURES
    assert len(caps) >= 8 and len(set(caps)) == len(caps)
    others = fr.other_captures()
    assert 95 <= len(others) <= 110 and not set(others) & set(caps)
    for k, (n, seed) in enumerate(list(caps) + others):
        raw = fr.capture(n, seed)
        assert 2 <= n <= 64 and raw.dtype == np.uint8 and raw.size == n * fr.CAPTURE_CHUNK
        pm = fr.capture_power(raw)
        assert fr.is_sensitive(pm, 5) == (k < len(caps)), (n, seed)
        assert pm.max() / pm.min() > (1.2 if n < 4 else 2.0), "the noise level differs from chunk to chunk"
        for pct in (5, 25):
            assert same_f32(fr.baseline(pm, pct), numpy_rule(pm, pct))
        if k < len(caps) + 6:                           # the vectorised map is K1's exact map; widening keeps it bit for bit
            np.testing.assert_array_equal(pm, ex.chunk_power(raw, fr.CAPTURE_CHUNK))
            wide = fr.widen(raw)
            assert wide.size == 64 * raw.size
            np.testing.assert_array_equal(fr.capture_power(wide, 65536), pm)
            if k < 3:
                np.testing.assert_array_equal(ex.chunk_power(wide, 65536), pm)


def test_floor_rule_is_the_oracles_on_dense_maps():
    """Where the reference's own expression (float64 threshold) and the header's float32 rule can be compared: the
    baseline is the same number, the threshold its float32 rounding."""
    from oracle import gpsjam_oracle as orc
    for n in (20, 257, 16385):
        pm = fr.grid_map("uniform", n)
        base, thr, count, mask = fr.floor_rule(pm, 5, 6.0)
        want_base, want_thr, _ = orc.power_threshold(pm)
        assert base == np.float32(want_base)
        np.testing.assert_allclose(thr, want_thr, rtol=2e-7)
        assert count == int(mask.sum()) == int((pm > thr).sum())


# --------------------------------------------------------------------------------------- the result vector
def test_result_cases_cover_what_they_name():
    cases = rr.result_cases()
    assert {c["nperseg"] for c in cases.values()} >= {16, 32, 64, 128, 1024, 4096}
    assert {c["rows"] for c in cases.values()} >= {0, 1, 15, 16, 17, 31, 33, 263}
    assert {c["n_chunks"] for c in cases.values()} >= {1, 983, 984, 985, 625, 262_150}
    assert {(c["pair_cap"], c["n_pairs"]) for c in cases.values()} >= {(0, 0), (3, 0), (3, 2), (3, 3), (28, 28)}
    assert {c["rank"] for c in cases.values()} >= {0, 2}
    assert any(c["first_index"] == -1 for c in cases.values())
    assert len([k for k in cases if k.startswith("mixed")]) == 12
    assert all(c["n_pairs"] <= c["pair_cap"] for c in cases.values())
    # a vector longer than the 256 x 1024 elements one pass of the copy blocks covers
    assert rr.result_len(262_150, 1024, 3) - 1024 > 256 * 1024


@pytest.mark.parametrize("name", ["base", "rows 263", "pairs 28 of 28", "rank 2"])
def test_restated_vector_is_the_torch_packer(name):
    import torch
    from gpsjam import sharded
    assert (sharded.HEADER, sharded.PAIR_FIELDS, sharded.LAG_INVALID) == (rr.HEADER, rr.PAIR_FIELDS, rr.LAG_INVALID)
    c = rr.result_cases()[name]
    amp, onset, _ = rr.records(1)
    psd = rr.psd_rows(c["rows"], c["nperseg"], 1)
    power = np.random.default_rng(5).uniform(50, 150, c["n_chunks"]).astype(np.float32)
    stats = np.array([55.5, 221.0, 17.0], np.float32)
    pairs, lags, peaks, margins = rr.pair_table(c["n_pairs"], 1)
    spec32 = torch.from_numpy(psd).mean(dim=0)
    want = sharded.pack_results(
        c["n_chunks"], c["nperseg"], torch.from_numpy(power), torch.from_numpy(stats), torch.tensor(int(amp["first"])),
        torch.tensor(int(amp["count"])), torch.tensor(float(amp["mean"]), dtype=torch.float32), torch.tensor(int(onset["start"])),
        torch.tensor(0 if c["rank"] == 0 else rr.LAG_INVALID), torch.tensor(0.0), torch.tensor(float(onset["noise"]), dtype=torch.float32),
        spec32, c["rows"], c["rank"], pairs=[tuple(p) for p in pairs.reshape(-1, 2)[:c["n_pairs"]].tolist()],
        pair_lags=torch.from_numpy(lags), pair_peaks=torch.from_numpy(peaks), pair_margins=torch.from_numpy(margins),
        capacity=c["pair_cap"], onset_margins=(float(onset["hit"]), float(onset["before"])), onset_guard=torch.tensor(int(onset["guard"])),
        onset_threshold=float(onset["thr"]), amp_sum=float(amp["sum"]),
        onset_record=torch.from_numpy(np.frombuffer(onset.tobytes(), np.int64).copy()),
        amp_record=torch.from_numpy(np.frombuffer(amp.tobytes(), np.int64).copy())).numpy()
    got = rr.pack_result(c["n_chunks"], power, stats, amp, onset, psd, c["rows"], c["nperseg"], c["rank"], c["n_pairs"],
                         c["pair_cap"], pairs, lags, peaks, margins, spectrum=spec32.numpy())
    assert got.shape == want.shape == (sharded.result_len(c["n_chunks"], c["nperseg"], c["pair_cap"]),)
    assert got.tobytes() == want.tobytes(), np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))[:10]
    # and the unpacker reads back what went in
    res = sharded.unpack_results(torch.from_numpy(got))
    assert (res.rank, res.n_above, res.amp_first, res.onset) == (c["rank"], 17, int(amp["first"]), int(onset["start"]))
    assert len(res.solved) == c["n_pairs"]


def test_part_vector_layout():
    amp, onset, part = rr.records(2)
    nper, rows, rows_cap = 16, 3, 5
    tiles = np.array([(1.5, 7), (2.5, -1)], rr.TILE_T)
    v = rr.pack_part(rank=3, antenna=1, part=2, parts=4, first_chunk=10, n_chunks=2, chunk_cap=4, first_row=6, rows=rows,
                     rows_cap=rows_cap, first_tile=10, n_tiles=2, tile_cap=3, first_sample=327680, nperseg=nper, n_pairs=1, pair_cap=2,
                     power=np.array([60.0, 70.0], np.float32), amp=part, onset=onset, tiles=tiles, psd=rr.psd_rows(rows, nper, 2),
                     pairs=np.array([0, 2], np.int32), lags=np.array([-4], np.int32), peaks=np.array([9.0], np.float32),
                     margins=np.array([0.5], np.float32))
    assert v.size == rr.part_len(4, 3, rows_cap, nper, 2) == 40 + 4 + 6 + 10 + 40
    assert v[0] == 2 and v[8] == rr.LAG_INVALID and list(v[20:26]) == [1, 2, 4, 10, 6, 327680] and v[28] == 2 and v[29] == 10
    assert list(v[40:44]) == [60.0, 70.0, 0.0, 0.0]
    assert v[44] == 1.5 and v[45:46].view(np.int64)[0] == 7 and v[47:48].view(np.int64)[0] == -1 and not v[48:50].any()
    assert list(v[50:60]) == [0, 2, -4, 9.0, 0.5, 0, 0, 0, 0, 0]
    back = v[60:].view(np.float32)
    assert back[:rows * nper].tobytes() == rr.psd_rows(rows, nper, 2).tobytes() and not back[rows * nper:].any()
    assert v[36:40].tobytes() == part.tobytes() and v[32:36].tobytes() == onset.tobytes()


def test_spectrum_bound_holds_for_the_kernels_float32_order():
    """The bound (ceil(rows / 16) + 17) 2^-24 is derived, not measured; the float32 order restated in numpy stays inside
    it on every shape the GPU tests use, and a mean taken in another order or precision is told apart where it matters."""
    worst = 0.0
    for name, c in rr.result_cases().items():
        if c["rows"] == 0:
            continue
        psd = rr.psd_rows(c["rows"], c["nperseg"], 3)
        r = rr.spectrum_ratio(rr.kernel_order_spectrum(psd, c["rows"], c["nperseg"]), psd, c["rows"], c["nperseg"])
        worst = max(worst, r)
        assert r <= 1.0, (name, r)
    print(f"float32 order restated: largest error / bound {worst:.3f}")
    assert rr.spectrum_bound(263) == (17 + 17) * 2.0 ** -24 and rr.spectrum_bound(1) == 18 * 2.0 ** -24
    # a packer that left out the last row, or divided by rows + 1, is far outside
    psd = rr.psd_rows(263, 64, 4)
    assert rr.spectrum_ratio(psd[:262].astype(np.float64).mean(axis=0), psd, 263, 64) > 100
    assert rr.spectrum_ratio(psd.astype(np.float64).sum(axis=0) / 264, psd, 263, 64) > 100
