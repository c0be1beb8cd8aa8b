"""The noise-floor rule and the result vector on the GPU, each against its numpy restatement.

Floor rule (tests/floor_restatement.py; tests/test_floor_result_host.py holds the restatement to numpy.percentile on every
map used here): baseline and threshold bit for bit, count and mask from the threshold, in the three kernels the rule is
compiled into -- gj_power_threshold_dev, workgroup 0 of gj_capture_scan_dev's tail launch, and the statistics launch of
gj_split_combine_dev.  The maps that decide are the SENSITIVE ones: short maps on which a lerp whose product and sum are
rounded once differs from numpy's, which rounds them separately.  The fused scan and the part kernels take chunk sizes
that are multiples of 65536 only (1024-byte chunks go through K1 alone + gj_power_threshold_dev), so the captures reach
those two kernels widened: every 1024-byte chunk repeated 64 times, which keeps the exact power map bit for bit.

Result vector (tests/result_restatement.py): gj_pack_result_dev, gj_pack_results_dev and gj_pack_part_dev write into a
0xA5-filled buffer with guard bytes; every element is compared (bytes; the mean spectrum within the derived bound of the
float64 mean), none is left as it was, the guards stay."""
import numpy as np
import pytest

import gpsjam
from gpsjam import _ffi
import floor_restatement as fr
import result_restatement as rr
from gpu_lib import GJ_ERR_UNSUPPORTED, SENTINEL, Guarded

pytestmark = pytest.mark.gpu

NOISE, WINDOW, FACTOR = 200000, 1000, 50.0


def payload(g) -> np.ndarray:
    """What the call wrote into a Guarded buffer; the pads on either side of it must be untouched."""
    g.check_pads("output")
    return g.read()


def same_bits(got, want) -> bool:
    got, want = np.float32(got), np.float32(want)
    if np.isnan(want):
        return bool(np.isnan(got))
    return got.view(np.uint32) == want.view(np.uint32)


# --------------------------------------------------------------------------------------- the floor rule
class Rule:
    """gj_power_threshold_dev with buffers kept over many calls."""

    def __init__(self, dev, n_max):
        self.dev = dev
        self.d_pow, self.d_st, self.d_st2 = dev.alloc(4 * n_max), dev.alloc(16), dev.alloc(16)
        self.mask = Guarded(dev, n_max)

    def run(self, pm, pct, rise_db):
        """(stats, mask) of one call with a mask and one without; the two calls' stats are the same bytes."""
        n = pm.size
        self.d_pow.upload(pm)
        self.mask.refill(n)
        self.d_st.upload(np.full(16, SENTINEL, np.uint8))
        self.d_st2.upload(np.full(16, SENTINEL, np.uint8))
        self.dev.power_threshold_dev(self.d_pow, n, self.d_st, self.mask.ptr, pct=float(pct), rise_db=float(rise_db))
        self.dev.power_threshold_dev(self.d_pow, n, self.d_st2, None, pct=float(pct), rise_db=float(rise_db))
        self.dev.synchronize()
        st, st2 = self.d_st.download(np.uint8, 16), self.d_st2.download(np.uint8, 16)
        assert st.tobytes() == st2.tobytes(), "the statistics depend on whether a mask is asked for"
        assert np.all(st[12:] == SENTINEL)
        return st[:12].view(np.float32), payload(self.mask)

    def free(self):
        for b in (self.d_pow, self.d_st, self.d_st2, self.mask):
            b.free()


def departs(stats, pm, pct, rise_db) -> bool:
    """The baseline or the threshold is not the restatement's, bit for bit."""
    base, thr, _, _ = fr.floor_rule(pm, pct, rise_db)
    return not (same_bits(stats[0], base) and same_bits(stats[1], thr))


def held(stats, mask, pm, pct, rise_db, what):
    base, thr, count, want_mask = fr.floor_rule(pm, pct, rise_db)
    assert same_bits(stats[0], base), (what, "baseline", float(stats[0]), float(base))
    assert same_bits(stats[1], thr), (what, "threshold", float(stats[1]), float(thr))
    assert stats[2] == count, (what, "count", float(stats[2]), count)
    if mask is not None:
        np.testing.assert_array_equal(mask, want_mask, err_msg=str(what))


@pytest.mark.parametrize("n", fr.GRID_N)
@pytest.mark.parametrize("kind", fr.KINDS)
def test_rule_on_the_grid(dev, kind, n):
    pm = fr.grid_map(kind, n)
    rule = Rule(dev, n)
    for pct in fr.GRID_PCT:
        for rise in fr.GRID_RISE:
            stats, mask = rule.run(pm, pct, rise)
            held(stats, mask, pm, pct, rise, (kind, n, pct, rise))
    rule.free()


@pytest.mark.parametrize("pct", fr.SHORT_PCT)
def test_rule_on_short_maps(dev, pct):
    rule = Rule(dev, 64)
    for n, k in fr.short_maps():
        pm = fr.short_map(n, k)
        for rise in (0, 6):
            stats, mask = rule.run(pm, pct, rise)
            held(stats, mask, pm, pct, rise, (n, k, pct, rise))
    rule.free()


def test_rule_on_the_sensitive_maps(dev):
    """Where a fused lerp is one unit in the last place off numpy's."""
    rule = Rule(dev, 64)
    got = [(m, rule.run(fr.short_map(m[0], m[1]), m[2], 6)) for m in fr.SENSITIVE_MAPS]
    rule.free()
    off = [m for m, (stats, _) in got if departs(stats, fr.short_map(m[0], m[1]), m[2], 6)]
    print(f"gj_power_threshold_dev departs from numpy on {len(off)} of {len(got)} sensitive maps: {off}")
    for (n, seed, pct), (stats, mask) in got:
        held(stats, mask, fr.short_map(n, seed), pct, 6, (n, seed, pct))


def test_rule_on_the_special_maps(dev):
    rule = Rule(dev, 64)
    for name, (pm, pcts) in fr.special_maps().items():
        for pct in pcts:
            for rise in (0, 6):
                stats, mask = rule.run(pm, pct, rise)
                held(stats, mask, pm, pct, rise, (name, pct, rise))
                if name.startswith("nan"):
                    assert np.isnan(stats[0]) and np.isnan(stats[1]) and stats[2] == 0 and not mask.any()
    rule.free()


class Scan:
    """gj_capture_scan_dev with d_stats and d_mask, buffers kept over many calls."""

    def __init__(self, dev, nbytes_max, nch_max):
        self.dev = dev
        self.d_iq, self.d_pow, self.d_st = dev.alloc(nbytes_max + 16), dev.alloc(4 * nch_max), dev.alloc(16)
        self.d_amp, self.d_on = dev.alloc(32), dev.alloc(32)
        self.mask = Guarded(dev, nch_max)
        self.loaded = None

    def run(self, key, raw, chunk_bytes, pct, rise_db):
        """(power map the call wrote, stats, mask)."""
        if self.loaded != key:
            self.d_iq.upload(raw)
            self.loaded = key
        nch = raw.size // chunk_bytes
        self.mask.refill(nch)
        self.d_pow.upload(np.full(4 * nch, SENTINEL, np.uint8))
        self.d_st.upload(np.full(16, SENTINEL, np.uint8))
        self.dev.capture_scan_dev(self.d_iq, raw.size, chunk_bytes, self.d_pow, 0.0, self.d_amp, NOISE, WINDOW, FACTOR, self.d_on,
                                  d_stats=self.d_st, d_mask=self.mask.ptr, pct=float(pct), rise_db=float(rise_db))
        self.dev.synchronize()
        return self.d_pow.download(np.float32, nch), self.d_st.download(np.float32, 3), payload(self.mask)

    def free(self):
        for b in (self.d_iq, self.d_pow, self.d_st, self.d_amp, self.d_on, self.mask):
            b.free()


def all_captures():
    return [(c, True) for c in fr.SENSITIVE_CAPTURES] + [(c, False) for c in fr.other_captures()]


@pytest.mark.parametrize("chunk_bytes", [fr.CAPTURE_CHUNK, 65536])
def test_rule_inside_the_capture_scan(dev, chunk_bytes):
    """chunk_bytes 1024: K1 alone, then the rule's own kernel; 65536 (the captures widened): workgroup 0 of the tail."""
    wide = chunk_bytes // fr.CAPTURE_CHUNK
    scan = Scan(dev, 64 * chunk_bytes, 64)
    off, n_sens = [], 0
    for (n, seed), sensitive in all_captures():
        raw = fr.capture(n, seed)
        want_pm = fr.capture_power(raw)
        if wide > 1:
            raw = fr.widen(raw, wide)
        for pct in (5, 25):
            for rise in (0, 6):
                pm, stats, mask = scan.run((n, seed), raw, chunk_bytes, pct, rise)
                np.testing.assert_array_equal(pm, want_pm)
                if sensitive and (pct, rise) == (5, 6):
                    n_sens += 1
                    if departs(stats, pm, pct, rise):
                        off.append((n, seed))
                        continue
                held(stats, mask, pm, pct, rise, (n, seed, pct, rise, chunk_bytes))
    scan.free()
    print(f"gj_capture_scan_dev at chunk_bytes {chunk_bytes} departs from numpy on {len(off)} of {n_sens} sensitive captures: {off}")
    assert not off


COMBINE_OTHERS = [(n, k) for n, k in fr.other_captures() if n >= 7 and k == 0][::6][:8]


def combine_groups():
    """Four deployments of four captures each (as four antennas), two sensitive ones in each; the world sizes differ."""
    sens = list(fr.SENSITIVE_CAPTURES[:8])
    assert len(COMBINE_OTHERS) == 8 and min(n for n, _ in sens) >= 7
    return [(world, sens[2 * g:2 * g + 2] + COMBINE_OTHERS[2 * g:2 * g + 2]) for g, world in enumerate((2, 3, 4, 8))]


def combined_vectors(dev, world, caps):
    """The combined result vectors of the single-process split rehearsal (gpsjam.split.emulated_rank0) over the widened
    captures `caps`; the combine plan carries the library's default rule, 5 % and 6 dB."""
    import torch
    from gpsjam import split
    raws = [torch.from_numpy(fr.widen(fr.capture(n, seed))).cuda() for n, seed in caps]
    work = torch.cuda.Stream()
    torch.cuda.set_stream(work)
    dev.set_stream(work.cuda_stream)
    try:
        st = split.emulated_rank0(dev, [int(r.numel()) for r in raws], lambda p, b0, b1: raws[p.antenna][b0:b1].contiguous(),
                                  lambda a, nbytes: raws[a][:nbytes].contiguous(), world, chunk_bytes=65536, chunk_samples=32768,
                                  nperseg=256, slice_samples=4096, noise_samples=20000, rssi_threshold=0.0)
        assert len(st.parts) > len(caps), "the captures really are cut"
        got = st.step()
        vecs = [got[a].cpu().numpy().copy() for a in range(len(caps))]
        torch.cuda.synchronize()
        st.close()
    finally:
        torch.cuda.set_stream(torch.cuda.default_stream())
        dev.set_stream(None, external=False)
    return vecs


@pytest.mark.parametrize("group", range(4))
def test_rule_inside_the_split_combine(dev, group):
    """Header slots 1..3 of every combined vector against the restatement on that vector's own power map."""
    world, caps = combine_groups()[group]
    vecs = combined_vectors(dev, world, caps)
    off = []
    for (n, seed), v in zip(caps, vecs):
        assert int(v[0]) == n
        pm = v[rr.HEADER:rr.HEADER + n].astype(np.float32)
        np.testing.assert_array_equal(pm, fr.capture_power(fr.capture(n, seed)))
        stats = v[1:4].astype(np.float32)
        assert np.array_equal(stats.astype(np.float64), v[1:4])
        if (n, seed) in fr.SENSITIVE_CAPTURES and departs(stats, pm, 5.0, 6.0):
            off.append((n, seed))
            continue
        held(stats, None, pm, 5.0, 6.0, (n, seed, world))
    print(f"gj_split_combine_dev (world {world}) departs from numpy on {len(off)} of 2 sensitive captures: {off}")
    assert not off


# --------------------------------------------------------------------------------------- the result vector
class Inputs:
    """The device-resident inputs of one result vector, and the same on the host."""

    def __init__(self, dev, c, seed):
        self.c, self.bufs = c, []
        self.amp, self.onset, self.amp_part = rr.records(seed, c.get("first_index"))
        rng = np.random.default_rng(35_000 + seed)
        self.power = rng.uniform(50, 150, c["n_chunks"]).astype(np.float32)
        self.stats = np.array([rng.uniform(40, 60), rng.uniform(200, 240), float(rng.integers(0, c["n_chunks"] + 1))], np.float32)
        self.psd = rr.psd_rows(c["rows"], c["nperseg"], seed)
        up = lambda a: self._up(dev, a)
        self.d_power, self.d_stats, self.d_amp, self.d_onset = up(self.power), up(self.stats), up(self.amp), up(self.onset)
        self.d_amp_part = up(self.amp_part)
        self.d_psd = up(self.psd) if c["rows"] else None

    def _up(self, dev, a):
        a = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
        b = dev.alloc(max(a.nbytes, 16)).upload(a)
        self.bufs.append(b)
        return b

    def free(self):
        for b in self.bufs:
            b.free()


class Pairs:
    def __init__(self, dev, n, seed):
        self.host = rr.pair_table(n, seed)
        self.bufs = [dev.alloc(max(a.nbytes, 16)).upload(a.view(np.uint8)) for a in self.host]

    def free(self):
        for b in self.bufs:
            b.free()


def vector_held(label, raw_bytes, want, psd, rows, nperseg, n_chunks) -> float:
    """Every element of the vector is written; everything but the spectrum equals the restatement's bytes; the spectrum
    lies within the bound.  Returns the largest error / bound of the spectrum."""
    got = raw_bytes.view(np.float64)
    assert got.size == want.size
    untouched = np.flatnonzero(raw_bytes.view(np.uint64) == np.uint64(0xA5A5A5A5A5A5A5A5))
    assert untouched.size == 0, (label, "elements never written", untouched[:10])
    s0 = rr.HEADER + n_chunks
    for name, sl in (("header", slice(0, rr.HEADER)), ("power map", slice(rr.HEADER, s0)), ("pair block", slice(s0 + nperseg, None))):
        bad = np.flatnonzero(got[sl].view(np.uint64) != want[sl].view(np.uint64))
        assert bad.size == 0, (label, name, bad[:10], got[sl][bad[:4]], want[sl][bad[:4]])
    spec = got[s0:s0 + nperseg]
    assert np.array_equal(spec.astype(np.float32).astype(np.float64), spec), "the spectrum is float32 values"
    if rows == 0:
        assert spec.tobytes() == bytes(8 * nperseg), (label, "no rows: a zero spectrum")
        return 0.0
    ratio = rr.spectrum_ratio(spec, psd, rows, nperseg)
    print(f"{label}: spectrum error / bound {ratio:.3f} (bound {rr.spectrum_bound(rows):.2e} relative)")
    assert ratio <= 1.0, (label, ratio)
    return ratio


RESULT_CASES = rr.result_cases()


@pytest.mark.parametrize("name", list(RESULT_CASES), ids=lambda s: s.replace(" ", "_"))
def test_pack_result(dev, name):
    c = RESULT_CASES[name]
    seed = list(RESULT_CASES).index(name)
    x, pairs = Inputs(dev, c, seed), Pairs(dev, c["n_pairs"], seed)
    out = Guarded(dev, 8 * rr.result_len(c["n_chunks"], c["nperseg"], c["pair_cap"]))
    have = c["n_pairs"] > 0
    dev.pack_result_dev(c["n_chunks"], x.d_power, x.d_stats, x.d_amp, x.d_onset, x.d_psd, c["rows"], c["nperseg"], c["rank"],
                        c["n_pairs"], c["pair_cap"], *(pairs.bufs if have else [None] * 4), out.ptr)
    dev.synchronize()
    want = rr.pack_result(c["n_chunks"], x.power, x.stats, x.amp, x.onset, x.psd, c["rows"], c["nperseg"], c["rank"],
                          c["n_pairs"], c["pair_cap"], *pairs.host)
    assert want[8] == (0.0 if c["rank"] == 0 else rr.LAG_INVALID) and (c["first_index"] != -1 or want[4] == -1.0)
    vector_held(name, payload(out), want, x.psd, c["rows"], c["nperseg"], c["n_chunks"])
    for b in (x, pairs, out):
        b.free()


def test_pack_results_three_captures(dev):
    """One launch for three captures of different lengths, row counts and pair capacities; each against the restatement."""
    nperseg = 1024
    cs = [dict(nperseg=nperseg, n_chunks=1, rows=0, pair_cap=3, n_pairs=3, rank=0),
          dict(nperseg=nperseg, n_chunks=262_150, rows=17, pair_cap=0, n_pairs=0, rank=1),
          dict(nperseg=nperseg, n_chunks=625, rows=263, pair_cap=28, n_pairs=2, rank=2)]
    xs = [Inputs(dev, c, 100 + a) for a, c in enumerate(cs)]
    pairs = Pairs(dev, 3, 100)                                  # shared: a capture's vector carries the first n_pairs of them
    outs = [Guarded(dev, 8 * rr.result_len(c["n_chunks"], nperseg, c["pair_cap"])) for c in cs]
    no_rows = dev.alloc(4 * nperseg)                            # rows == 0: the pointer must still be a buffer's
    desc = [_ffi.CombineCapture(n_chunks=c["n_chunks"], rows=c["rows"], n_tiles=0, total_bytes=0, n_parts=1, antenna=c["rank"],
                                n_pairs=c["n_pairs"], pair_cap=c["pair_cap"], d_power=x.d_power.ptr, d_stats=x.d_stats.ptr,
                                d_tiles=None, d_amp_parts=None, d_onset_parts=None, d_amp=x.d_amp.ptr, d_onset=x.d_onset.ptr,
                                d_psd=x.d_psd.ptr if c["rows"] else no_rows.ptr, d_out=o.ptr) for c, x, o in zip(cs, xs, outs)]
    dev.pack_results_dev(desc, nperseg, *pairs.bufs)
    dev.synchronize()
    for a, (c, x, o) in enumerate(zip(cs, xs, outs)):
        want = rr.pack_result(c["n_chunks"], x.power, x.stats, x.amp, x.onset, x.psd, c["rows"], nperseg, c["rank"], c["n_pairs"],
                              c["pair_cap"], *pairs.host)
        vector_held(f"capture {a}", payload(o), want, x.psd, c["rows"], nperseg, c["n_chunks"])
    for b in xs + outs + [pairs, no_rows]:
        b.free()


@pytest.mark.parametrize("full", [False, True], ids=["below_capacity", "at_capacity"])
def test_pack_part(dev, full):
    """Every count below its capacity (zero fill in between) and every count equal to it."""
    nperseg = 64
    cap = dict(chunk_cap=37, tile_cap=37, rows_cap=9, pair_cap=4)
    cnt = dict(n_chunks=37, n_tiles=37, rows=9, n_pairs=4) if full else dict(n_chunks=21, n_tiles=20, rows=5, n_pairs=1)
    x = Inputs(dev, dict(nperseg=nperseg, n_chunks=cnt["n_chunks"], rows=cnt["rows"]), 200 + full)
    pairs = Pairs(dev, cnt["n_pairs"], 200)
    rng = np.random.default_rng(36_000)
    tiles = np.zeros(cnt["n_tiles"], rr.TILE_T)
    tiles["sum"], tiles["first"] = rng.uniform(0, 1e4, tiles.size), rng.integers(-1, 1 << 20, tiles.size)
    d_tiles = dev.alloc(16 * tiles.size).upload(tiles.view(np.uint8))
    hdr = dict(rank=3, antenna=1, part=2, parts=5, first_chunk=74, first_row=18, first_tile=74, first_sample=74 * 32768)
    n = dev.part_result_len(cap["chunk_cap"], cap["tile_cap"], cap["rows_cap"], nperseg, cap["pair_cap"])
    assert n == rr.part_len(cap["chunk_cap"], cap["tile_cap"], cap["rows_cap"], nperseg, cap["pair_cap"])
    out = Guarded(dev, 8 * n)
    a = _ffi.PartPack(hdr["rank"], hdr["antenna"], hdr["part"], hdr["parts"], hdr["first_chunk"], cnt["n_chunks"], cap["chunk_cap"],
                      hdr["first_row"], cnt["rows"], cap["rows_cap"], hdr["first_tile"], cnt["n_tiles"], cap["tile_cap"],
                      hdr["first_sample"], nperseg, cnt["n_pairs"], cap["pair_cap"], 0, x.d_power.ptr, x.d_amp_part.ptr, x.d_onset.ptr,
                      d_tiles.ptr, x.d_psd.ptr, *[b.ptr for b in pairs.bufs])
    dev.pack_part_dev(a, out.ptr)
    dev.synchronize()
    want = rr.pack_part(**hdr, **cap, **cnt, nperseg=nperseg, power=x.power, amp=x.amp_part, onset=x.onset, tiles=tiles, psd=x.psd,
                        pairs=pairs.host[0], lags=pairs.host[1], peaks=pairs.host[2], margins=pairs.host[3])
    got = payload(out)
    assert got.size == want.nbytes
    bad = np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))
    assert bad.size == 0, (bad[:10], got.view(np.float64)[bad[:4]], want[bad[:4]])
    for b in (x, pairs, out, d_tiles):
        b.free()


@pytest.mark.parametrize("nperseg", [0, -64, 100, 8, 8192])
def test_pack_result_refuses_what_the_batched_packer_refuses(dev, nperseg):
    """gj_pack_result_dev takes nperseg as gj_pack_results_dev does: a power of two in 16 .. 4096, or GJ_ERR_UNSUPPORTED
    and nothing written."""
    c = dict(rr.BASE, nperseg=64, n_pairs=0)
    x = Inputs(dev, c, 300)
    out = Guarded(dev, 8 * rr.result_len(c["n_chunks"], 8192, c["pair_cap"]))
    with pytest.raises(gpsjam.GpsJamError) as e:
        dev.pack_result_dev(c["n_chunks"], x.d_power, x.d_stats, x.d_amp, x.d_onset, x.d_psd, c["rows"], nperseg, 0, 0, c["pair_cap"],
                            None, None, None, None, out.ptr)
    assert e.value.status == GJ_ERR_UNSUPPORTED
    dev.synchronize()
    out.check_untouched("a refused call")
    desc = _ffi.CombineCapture(n_chunks=c["n_chunks"], rows=c["rows"], n_tiles=0, total_bytes=0, n_parts=1, antenna=0, n_pairs=0,
                               pair_cap=c["pair_cap"], d_power=x.d_power.ptr, d_stats=x.d_stats.ptr, d_tiles=None, d_amp_parts=None,
                               d_onset_parts=None, d_amp=x.d_amp.ptr, d_onset=x.d_onset.ptr, d_psd=x.d_psd.ptr, d_out=out.ptr)
    with pytest.raises(gpsjam.GpsJamError) as e2:
        dev.pack_results_dev([desc], nperseg)
    assert e2.value.status == e.value.status
    x.free(), out.free()
