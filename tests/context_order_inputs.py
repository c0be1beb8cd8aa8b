"""One small probe per user of a context's workspace arena (ctx->ws), for tests/context_order and
tests/test_context_order_host.py.

Every kernel has a test file of its own that holds it to a restatement.  What those files cannot see is the state the calls
of ONE context share: the arena that fifteen or so entry points carve up, each by its own layout, and that ensure_workspace
replaces while earlier kernels are still queued.  A probe here is one such call made small:

  * ``Probe(dev, spec)`` uploads the inputs and allocates sentinel-filled (0xA5), padded outputs ONCE (two sets, "slots",
    so that a queue may hold a probe twice);
  * ``enqueue(slot)`` makes the ``*_dev`` call and returns: no host wait, any number of times;
  * ``download(slot)`` waits, checks the pads and returns the outputs as bytes; ``scrub(slot)`` puts the sentinels back;
  * ``check(outs, conv)`` holds those bytes to the restatement with the inputs, helpers and tolerances of the kernel's
    own test package (imported, not copied);
  * ``spec.need(dev)`` is the workspace the call asks for, through the library's own ``*_workspace`` function where one
    exists (None where none does; K2's takes a context, the others answer without one).

Inputs are made once per process from fixed seeds and never written to."""
import functools
import os
import random
import re
from typing import Callable, NamedTuple, Tuple

import numpy as np

import acq_edges_inputs as ai
import gpsjam
from gpsjam import _ffi, gnss
from gpsjam.synth import StreamSpec, generate
from gpu_lib import CAF_REC, Guarded, caf_records, make_slots

DEFAULT = (127.5, 1.0 / 127.5)
CONVENTIONS = (DEFAULT, (128.0, 1.0 / 128.0), (0.0, 1.0), (255.0, 1.0))     # the order test 6 queues them in
FILLS = (0x00, 0xFF, 0x7F)          # zeros (what fresh pages hold), NaN / all-ones, large finite float / large positive int
GJ_INJECT_FILL_WORKSPACE = 2        # include/gpsjam.h
NOISE, WINDOW, FACTOR = 200000, 1000, 50.0
FS = 2.048e6
MiB = 1 << 20


class Built(NamedTuple):
    keep: list                      # device buffers and objects that must outlive the probe
    out_sizes: Tuple[int, ...]
    launch: Callable                # launch(outs): enqueue on the context's stream
    check: Callable                 # check(outs_bytes, conv): the kernel's own check against its restatement


class Spec(NamedTuple):
    name: str
    entries: Tuple[str, ...]        # extern "C" entry points the probe calls
    layout: str                     # which carving of the arena it uses
    honours_unpack: bool            # results follow gj_set_unpack's offset
    build: Callable                 # build(dev) -> Built
    need: Callable                  # need(dev | None) -> bytes | None
    waits: bool = False             # the entry point itself synchronises (cannot sit in a queue without a host wait)


def lib():
    return _ffi.load()


def _ctx(dev):
    return dev._ctx if dev is not None else None


# ------------------------------------------------------------------------------------------------ inputs, once per process
@functools.lru_cache(maxsize=None)
def k1_capture():
    nbytes = 3 * 65536 + 24690      # three chunks and a ragged fourth
    raw = generate(StreamSpec(seed=71, jam_start=60000, jam_end=1 << 40, jam_sigma=50.0), nbytes // 2)
    raw.setflags(write=False)
    return raw


@functools.lru_cache(maxsize=None)
def scan_capture():
    raw = generate(StreamSpec(seed=72, jam_start=400_000, jam_end=1 << 40, jam_sigma=60.0), MiB)   # 2 MiB, an onset inside
    raw.setflags(write=False)
    return raw


@functools.lru_cache(maxsize=None)
def amp_capture():
    nbytes = 9 * 65536 + 12346 + 2
    raw = generate(StreamSpec(seed=73, jam_start=230_000, jam_end=1 << 40, jam_sigma=70.0), nbytes // 2 + 1)[:nbytes]
    raw.setflags(write=False)
    return raw


@functools.lru_cache(maxsize=None)
def welch_capture(n, seed=500):
    return tuple(generate(StreamSpec(seed=seed + a, antenna=a, jam_start=n // 3, jam_end=2 * n // 3, jam_sigma=30.0 + 10 * a), n)
                 for a in range(3))


PART_TILE, PART_SLICE = 65536, 30000
PART_BYTES = 40 * PART_TILE
PART_CUTS = (13 * PART_TILE, 28 * PART_TILE)      # the second part of tests/test_round5_gpu.py's split: the onset lies in it


@functools.lru_cache(maxsize=None)
def part_capture():
    raw = generate(StreamSpec(seed=12, jam_start=900_000, jam_end=1 << 40, jam_sigma=60.0), PART_BYTES // 2)
    raw.setflags(write=False)
    return raw


K5_SPECS = [(0, 0.0), (4, 0.0), (-6, 0.0)]
CAF_SPECS = [(0, 0.0), (4, 1.0), (-6, -1.0)]       # pairwise offsets 1, -1 and -2 bins: all inside bins -2 .. 2
PAIRS = [(0, 1), (0, 2), (1, 2)]
CAF_FIRST, CAF_BINS, CAF_BPL = -2, 5, 2


@functools.lru_cache(maxsize=None)
def antennas(n, caf_offsets):
    import caf_restatement as caf
    return tuple(caf.make_antennas(n, CAF_SPECS if caf_offsets else K5_SPECS, seed=47 + (n % 97)))


ACQ_FS = 0.512e6                                   # nsamp 512: the shortest the wrapper offers
ACQ_PRNS = [3, 17, 3]                              # one repeated; 3 is in the capture, 17 is not
ACQ_INTG = 3


@functools.lru_cache(maxsize=None)
def acq_case():
    nsamp = ai.nsamp_of(ACQ_FS)
    raw = ai.gps_like(2 * 700 + (ACQ_INTG + 1) * nsamp + ai.TAIL + 5, [(3, 200.0, nsamp // 3, 9.0)], fs=ACQ_FS, seed=49)
    return ai.Case("context order 512", raw, ACQ_FS, ACQ_PRNS, first=5, intg=ACQ_INTG, hband=600.0)


SERIES_STRIDE, SERIES_EPOCHS, SERIES_EPL = 700, 3, 2
BIG_SERIES_PRNS = [3, 17, 25]
BIG_SERIES_SATS = [(3, 1400.0, 517, 9.0), (17, -3000.0, 1201, 1.5), (25, 5230.0, 88, 3.0)]     # tests/acq_series SATS
BIG_SERIES_STRIDE = 1500


@functools.lru_cache(maxsize=None)
def big_series_capture(n_epochs):
    n = 1000 + (n_epochs - 1) * BIG_SERIES_STRIDE + 11 * 2048 + 3 * 2048
    raw = ai.series_like(n, BIG_SERIES_SATS)
    raw.setflags(write=False)
    return raw


# ------------------------------------------------------------------------------------------------ small helpers
def _view(b, dtype, count=None):
    return np.frombuffer(b, dtype, -1 if count is None else count)


def _default_only(conv):
    return conv == DEFAULT


def _restated(conv):
    """The conventions the restatements of the CAF and of the row sums are held at by their own files."""
    return conv in CONVENTIONS[:2]


def _quiet_searcher(dev, *args, **kw):
    """An AcqSearch whose constructor does not pre-size the arena: the probes' queues want the growth to happen in flight."""
    dev.reserve = lambda nbytes: None
    try:
        return gnss.AcqSearch(dev, *args, **kw)
    finally:
        del dev.reserve


# ------------------------------------------------------------------------------------------------ K1 and the fused scan
def _build_chunk_power(dev):
    import exact_restatement as ex
    raw = k1_capture()
    cap = dev.alloc(raw.size + 16).upload(raw)
    nch = dev.chunk_count(raw.size, 65536)

    def check(outs, conv):
        assert nch == 4
        if _default_only(conv):
            np.testing.assert_array_equal(_view(outs[0], np.float32), ex.chunk_power(raw, 65536))
    return Built([cap], (4 * nch,), lambda outs: dev.chunk_power_dev(cap, raw.size, 65536, outs[0]), check)


def _check_scan(raw, power, amp, onset, conv):
    import exact_restatement as ex
    from oracle import gpsjam_oracle as orc
    if not _default_only(conv):
        return
    np.testing.assert_array_equal(_view(power, np.float32), ex.chunk_power(raw, 65536))
    ex.check_exact(amp, onset, raw, 0.1)
    assert _view(onset, ex.ONSET_T)[0]["start"] == orc.tdoa_onset(orc.tdoa_unpack(raw)) > 0


def _build_scan(fused_tail):
    def build(dev):
        raw = scan_capture()
        cap = dev.alloc(raw.size + 16).upload(raw)
        nch = dev.chunk_count(raw.size, 65536)
        sb = dev.tdoa_slot_bytes(PART_SLICE)

        def launch(outs):
            if fused_tail:
                dev.capture_scan_dev(cap, raw.size, 65536, outs[0], 0.1, outs[1], NOISE, WINDOW, FACTOR, outs[2], d_stats=outs[3],
                                     d_mask=outs[4], slice_samples=PART_SLICE, d_slot=outs[5])
            else:
                dev.stream_scan_dev(cap, raw.size, 65536, outs[0], 0.1, outs[1], NOISE, WINDOW, FACTOR, outs[2])

        def check(outs, conv):
            _check_scan(raw, outs[0], outs[1], outs[2], conv)
            if fused_tail and _default_only(conv):
                start = int(_view(outs[2], np.int64, 1)[0])
                assert outs[5][16:16 + 2 * PART_SLICE] == raw[2 * start:2 * (start + PART_SLICE)].tobytes(), "the slot is the slice at the onset"
                assert _view(outs[4], np.uint8).max() <= 1, "the mask was written"
        sizes = (4 * nch, 32, 32) + ((16, nch, sb) if fused_tail else ())
        return Built([cap], sizes, launch, check)
    return build


def _build_amp_onset(which, offset):
    def build(dev):
        raw = amp_capture()
        cap = dev.alloc(raw.size + 16).upload(raw)
        nbytes = raw.size - 2
        piece = raw[offset:offset + nbytes]

        def launch(outs):
            if which == "amp":
                dev.amp_stats_dev(cap.ptr + offset, nbytes, 0.2, outs[0])
            else:
                dev.onset_dev(cap.ptr + offset, nbytes, NOISE, WINDOW, FACTOR, outs[0])

        def check(outs, conv):
            import exact_restatement as ex
            if not _default_only(conv):
                return
            if which == "amp":
                a, want = _view(outs[0], ex.AMP_T)[0], ex.amp_stats(piece, 0.2)
                assert (a["i"], a["c"]) == (want["first"], want["count"]) and want["count"] > 0
                np.testing.assert_allclose(a["s"], want["sum"], rtol=2e-7)
                np.testing.assert_allclose(a["m"], want["mean"], rtol=2e-7)
            else:
                o, want = _view(outs[0], ex.ONSET_T)[0], ex.onset(piece, NOISE, WINDOW, FACTOR)
                assert want["start"] > 0
                for f in ("start", "guard", "noise", "thr", "hit"):
                    assert o[f] == want[f], (f, o, want)
        return Built([cap], (32,), launch, check)
    return build


# ------------------------------------------------------------------------------------------------ K2
def _check_welch(raw, got_bytes, rows, nperseg, chunk, conv):
    from oracle import gpsjam_oracle as orc
    got = _view(got_bytes, np.float32).reshape(rows, nperseg)
    assert np.isfinite(got).all()
    if not _default_only(conv):
        return
    lin, _, _ = orc.widmo_waterfall(raw, nperseg=nperseg, chunk_samples=chunk)
    keep = lin > 1e-12
    assert got.shape == lin.shape and float(np.max(np.abs(got[keep] - lin[keep]) / lin[keep])) < 1e-4      # tests/test_round5_gpu.py


def _build_welch(nperseg, chunk, n, timed=False):
    def build(dev):
        raw = welch_capture(n)[1]
        cap = dev.alloc(2 * n + 16).upload(raw)
        rows = dev.welch_rows(2 * n, chunk, nperseg)
        call = dev.welch_timed_dev if timed else dev.welch_dev
        return Built([cap], (4 * rows * nperseg,), lambda outs: call(cap, 2 * n, chunk, nperseg, FS, outs[0]),
                     lambda outs, conv: _check_welch(raw, outs[0], rows, nperseg, chunk, conv))
    return build


def _build_welch_batch(nperseg, chunk, n):
    def build(dev):
        raws = welch_capture(n)
        caps = [dev.alloc(2 * n + 16).upload(r) for r in raws]
        rows = dev.welch_rows(2 * n, chunk, nperseg)

        def check(outs, conv):
            for r, o in zip(raws, outs):
                _check_welch(r, o, rows, nperseg, chunk, conv)
        return Built(caps, (4 * rows * nperseg,) * 3, lambda outs: dev.welch_batch_dev(caps, 2 * n, chunk, nperseg, FS, list(outs)), check)
    return build


def _part_view(dev, keep):
    raw = part_capture()
    b0, b1 = PART_CUTS[0] - PART_TILE, min(PART_BYTES, PART_CUTS[1] + 2 * PART_SLICE + PART_TILE)
    buf = dev.alloc(b1 - b0 + 16).upload(raw[b0:b1])
    d_noise = dev.alloc(2 * NOISE).upload(raw[:2 * NOISE])
    keep += [buf, d_noise]
    return _ffi.PartView(buf.ptr, b1 - b0, b0, PART_CUTS[0], PART_CUTS[1] - PART_CUTS[0], PART_BYTES, d_noise.ptr)


PART_CHUNK_SAMPLES, PART_NPERSEG = 32768, 1024


def _build_part_welch(dev):
    keep = []
    view = _part_view(dev, keep)
    own = part_capture()[PART_CUTS[0]:PART_CUTS[1]]
    rows = dev.welch_rows(own.size, PART_CHUNK_SAMPLES, PART_NPERSEG)
    assert rows == 15
    return Built(keep + [view], (4 * rows * PART_NPERSEG,), lambda outs: dev.part_welch_dev(view, PART_CHUNK_SAMPLES, PART_NPERSEG, FS, outs[0]),
                 lambda outs, conv: _check_welch(own, outs[0], rows, PART_NPERSEG, PART_CHUNK_SAMPLES, conv))


def _build_part_scan(with_slot):
    def build(dev):
        import exact_restatement as ex
        from oracle import gpsjam_oracle as orc
        keep = []
        view = _part_view(dev, keep)
        raw = part_capture()
        own = raw[PART_CUTS[0]:PART_CUTS[1]]
        nch = own.size // PART_TILE
        sb = dev.tdoa_slot_bytes(PART_SLICE)

        def launch(outs):
            if with_slot:
                dev.part_capture_scan_dev(view, 65536, outs[0], 0.0, outs[1], outs[2], NOISE, WINDOW, FACTOR, outs[3],
                                          slice_samples=PART_SLICE, d_slot=outs[4])
            else:
                dev.part_scan_dev(view, 65536, outs[0], 0.0, outs[1], outs[2], NOISE, WINDOW, FACTOR, outs[3])

        def check(outs, conv):
            if not _default_only(conv):
                return
            np.testing.assert_array_equal(_view(outs[0], np.float32), ex.chunk_power(own, 65536))
            start = int(_view(outs[3], np.int64, 1)[0])
            assert start == orc.tdoa_onset(orc.tdoa_unpack(raw)) and PART_CUTS[0] // 2 <= start < PART_CUTS[1] // 2
            if with_slot:
                assert outs[4][16:16 + 2 * PART_SLICE] == raw[2 * start:2 * (start + PART_SLICE)].tobytes()
        sizes = (4 * nch, 16 * dev.amp_tile_count(own.size), 32, 32) + ((sb,) if with_slot else ())
        return Built(keep + [view], sizes, launch, check)
    return build


# ------------------------------------------------------------------------------------------------ K5 and the CAF
def _check_k5(raws, outs, conv):
    import k5_check as k5
    if not _default_only(conv):
        return
    lags, peaks, margins = _view(outs[0], np.int32), _view(outs[1], np.float32), _view(outs[2], np.float32)
    for k, (i, j) in enumerate(PAIRS):
        e = k5.expect(raws[i], raws[j])
        assert e["lag"] == K5_SPECS[j][0] - K5_SPECS[i][0]
        k5.check(lags[k], peaks[k], margins[k], e, f"pair {(i, j)}")


def _build_xcorr(n, slots=False):
    def build(dev):
        raws = antennas(n, False)
        if slots:
            d_slots, sb = make_slots(dev, raws, n)
            keep = [d_slots]

            def launch(outs):
                dev.xcorr_slots_dev(d_slots, sb, 3, n, PAIRS, outs[0], outs[1], outs[2])
        else:
            caps = [dev.alloc(2 * n + 16).upload(r) for r in raws]
            d_starts = dev.alloc(8 * 3).upload(np.zeros(3, np.int64))
            keep = caps + [d_starts]

            def launch(outs):
                dev.xcorr_lags_dev(caps, [2 * n] * 3, d_starts, n, PAIRS, outs[0], outs[1], outs[2])
        return Built(keep, (12, 12, 12), launch, lambda outs, conv: _check_k5(raws, outs, conv))
    return build


def _build_caf(n, slots=False):
    def build(dev):
        import caf_lengths_inputs as ci
        raws = antennas(n, True)
        if slots:
            d_slots, sb = make_slots(dev, raws, n)
            keep = [d_slots]

            def launch(outs):
                dev.xcorr_caf_slots_dev(d_slots, sb, 3, n, PAIRS, CAF_FIRST, CAF_BINS, outs[0], outs[1], outs[2], bins_per_launch=CAF_BPL)
        else:
            caps = [dev.alloc(2 * n + 16).upload(r) for r in raws]
            d_starts = dev.alloc(8 * 3).upload(np.zeros(3, np.int64))
            keep = caps + [d_starts]

            def launch(outs):
                dev.xcorr_caf_dev(caps, [2 * n] * 3, d_starts, n, PAIRS, CAF_FIRST, CAF_BINS, outs[0], outs[1], outs[2], bins_per_launch=CAF_BPL)

        def check(outs, conv):
            if not _restated(conv):
                return
            recs = caf_records(outs[0])
            lags = _view(outs[1], np.int32).reshape(3, CAF_BINS)
            peaks = _view(outs[2], np.float32).reshape(3, CAF_BINS)
            bins = list(range(CAF_FIRST, CAF_FIRST + CAF_BINS))
            for k, (i, j) in enumerate(PAIRS):
                assert recs[k].reserved == 0.0
                want = caf_reference(n, i, j, conv[0])
                assert (want.lag, want.bin) == (CAF_SPECS[j][0] - CAF_SPECS[i][0], int(CAF_SPECS[j][1] - CAF_SPECS[i][1]))
                ci.hold(recs[k], lags[k], peaks[k], want, f"n {n} pair {(i, j)} offset {conv[0]}")
            assert bins[0] == -2
        return Built(keep, (CAF_REC * 3, 4 * 3 * CAF_BINS, 4 * 3 * CAF_BINS), launch, check)
    return build


@functools.lru_cache(maxsize=None)
def caf_reference(n, i, j, offset):
    import caf_lengths_inputs as ci
    raws = antennas(n, True)
    return ci.search_bins(raws[j], raws[i], list(range(CAF_FIRST, CAF_FIRST + CAF_BINS)), offset)


# ------------------------------------------------------------------------------------------------ acquisition
def _acq_searcher(dev, case):
    srch = _quiet_searcher(dev, prns=case.prns, fs=case.fs, intg=case.intg, threshold=case.threshold, hband=case.hband)
    assert srch.nsamp == case.nsamp == 512
    return srch


def _check_acq_records(rec_bytes, case, what):
    got = ai.records(rec_bytes)
    ref = ai.reference(case)
    for k, prn in enumerate(case.prns):
        ai.check_record(got[k], ref[prn][-1], case, (what, prn))
    return got


def _build_acq_search(with_power):
    def build(dev):
        case = acq_case()
        srch = _acq_searcher(dev, case)
        cap = dev.alloc(case.raw.size + 16).upload(case.raw)
        cells = len(case.prns) * len(srch.freqs) * srch.nsamp

        def launch(outs):
            srch._search_dev(cap, case.raw.size, case.first, outs[1] if with_power else None, srch.threshold, outs[0])

        def check(outs, conv):
            got = _check_acq_records(outs[0], case, "power form" if with_power else "single launch")
            assert bool(got[0]["acquired"]) and bool(got[2]["acquired"]) and not bool(got[1]["acquired"])
            assert int(got[1]["steps"]) == case.intg >= 2, "the absent PRN runs every step: running maxima and done flags are used"
            assert outs[0][:ai.REC] == outs[0][2 * ai.REC:], "the repeated PRN: the same record"
            if with_power:
                P = _view(outs[1], np.float64).reshape(len(case.prns), len(srch.freqs), srch.nsamp)
                for k, prn in enumerate(case.prns):
                    ai.check_power(P[k], ai.reference(case)[prn][-1], case, ("power form", prn))
        return Built([srch, cap], (ai.REC * len(case.prns),) + ((8 * cells,) if with_power else ()), launch, check)
    return build


def _build_acq_series(dev):
    case = acq_case()
    srch = _acq_searcher(dev, case)
    cap = dev.alloc(case.raw.size + 16).upload(case.raw)
    per = ai.REC * len(case.prns)

    def check(outs, conv):
        for e in range(SERIES_EPOCHS):
            _check_acq_records(outs[0][e * per:(e + 1) * per], case.at(case.first + e * SERIES_STRIDE), f"series epoch {e}")
    return Built([srch, cap], (per * SERIES_EPOCHS,),
                 lambda outs: srch.series_dev(cap, case.raw.size, case.first, SERIES_STRIDE, SERIES_EPOCHS, outs[0], SERIES_EPL), check)


def _build_big_series(n_epochs):
    """The series at the reference's own rate (nsamp 2048, 71 bins, intg 10) with every epoch in ONE launch: a rung of the
    ladder.  Held to the oracle's search at the first and the last epoch, as tests/acq_series does."""
    def build(dev):
        raw = big_series_capture(n_epochs)
        srch = _quiet_searcher(dev, prns=BIG_SERIES_PRNS)
        cap = dev.alloc(raw.size + 16).upload(raw)
        per = ai.REC * len(BIG_SERIES_PRNS)

        def check(outs, conv):
            for e in (0, n_epochs - 1):
                first = 1000 + e * BIG_SERIES_STRIDE
                for k, prn in enumerate(BIG_SERIES_PRNS):
                    r = gnss._AcqStruct.from_buffer_copy(outs[0], e * per + k * ai.REC)
                    want = big_series_reference(n_epochs, first, prn)
                    assert bool(r.acquired) == want["acquired"] and r.steps == want["steps"], (e, prn, want)
                    if want["peakr"] > 1.5:
                        assert (r.code_index, r.freq_index) == (want["codei"], want["freqi"]), (e, prn, want)
                        np.testing.assert_allclose(r.peak_ratio, want["peakr"], rtol=2e-3)
                        np.testing.assert_allclose(r.cn0, want["cn0"], atol=0.02)
        return Built([srch, cap], (per * n_epochs,),
                     lambda outs: srch.series_dev(cap, raw.size, 1000, BIG_SERIES_STRIDE, n_epochs, outs[0], n_epochs), check)
    return build


@functools.lru_cache(maxsize=None)
def big_series_reference(n_epochs, first, prn):
    from oracle import gpsjam_oracle as orc
    return orc.acq_search(big_series_capture(n_epochs), first, prn)[0]


_SURFACE = {}


def search_surface():
    """P [n_prn][n_freq][nsamp] of the power-form search probe, taken once on a context of its own: the K-peak probe's
    input ("the power array of the search above")."""
    if "P" not in _SURFACE:
        with gpsjam.Device(0) as dev:
            p = Probe(dev, SPECS["acq_search_power"], slots=1)
            try:
                p.enqueue()
                outs = p.download()
                p.check(outs, DEFAULT)
            finally:
                p.free()
        case = acq_case()
        P = np.frombuffer(outs[1], np.float64).reshape(len(case.prns), -1, case.nsamp).copy()
        P.setflags(write=False)
        _SURFACE["P"] = P
    return _SURFACE["P"]


PEAKS_K, PEAKS_GUARD = 2, 4


def _build_peaks(dev):
    import peaks_restatement as pr
    P = search_surface()
    n_prn, n_freq, nsamp = P.shape
    d_power = dev.alloc(P.nbytes).upload(P)

    def check(outs, conv):
        peaks = _view(outs[0], gpsjam.ACQ_PEAK_DTYPE).reshape(n_prn, PEAKS_K)
        floor = _view(outs[1], gpsjam.ACQ_FLOOR_DTYPE)
        power, code, freq, mean, kept = pr.top_k_all(P, PEAKS_K, PEAKS_GUARD)               # tests/peaks compare()
        np.testing.assert_array_equal(peaks["power"].view(np.uint64), power.view(np.uint64))
        np.testing.assert_array_equal(peaks["code_index"], code)
        np.testing.assert_array_equal(peaks["freq_index"], freq)
        np.testing.assert_array_equal(floor["kept_columns"], kept)
        assert not floor["reserved"].any()
        assert np.all(np.abs(floor["mean_power"] - mean) <= pr.floor_bound(n_freq, kept) * mean)
        assert len(set(power[1].tolist())) == PEAKS_K, "no tie between the peaks of a surface"
    return Built([d_power], (16 * n_prn * PEAKS_K, 16 * n_prn),
                 lambda outs: dev.acq_peaks_dev(d_power, n_prn, n_freq, nsamp, PEAKS_K, PEAKS_GUARD, outs[0], outs[1]), check)


# ------------------------------------------------------------------------------------------------ the row sums
def _build_sk(nfft, hop, m, n_rows, first=1):
    def build(dev):
        import ridge_restatement as rr
        import skurt_restatement as sr
        raw = rr.parity_capture()
        cap = dev.alloc(raw.size + 16).upload(raw)
        assert n_rows <= gpsjam.sk_rows(raw.size, first, nfft, hop, m)

        def check(outs, conv):
            got = tuple(_view(o, np.float32).reshape(n_rows, nfft) for o in outs)
            if not _restated(conv):
                return
            sr.compare(got, sk_powers(nfft, hop, first, m * n_rows, conv), m, n_rows, ("context order", nfft, m, conv))
        return Built([cap], (4 * n_rows * nfft,) * 3,
                     lambda outs: dev.spectral_kurtosis_dev(cap, raw.size, first, nfft, hop, m, n_rows, outs[0], outs[1], outs[2]), check)
    return build


@functools.lru_cache(maxsize=None)
def sk_powers(nfft, hop, first, n_frames, conv):
    import ridge_restatement as rr
    import skurt_restatement as sr
    p = sr.frame_powers(rr.parity_capture(), nfft, hop, first, n_frames, conv[0], conv[1])
    p.setflags(write=False)
    return p


def _build_csd(nfft, hop, m, n_rows):
    def build(dev):
        import csd_restatement as cs
        a, b = cs.parity_pair()
        ca, cb = dev.alloc(a.size + 16).upload(a), dev.alloc(b.size + 16).upload(b)
        fa, fb = cs.PARITY_FIRST_A, cs.PARITY_FIRST_B
        assert n_rows <= gpsjam.csd_rows(a.size, fa, b.size, fb, nfft, hop, m)

        def check(outs, conv):
            cells = (n_rows, nfft)
            got = (_view(outs[0], np.float32).reshape(cells), _view(outs[1], np.float32).reshape(cells),
                   _view(outs[2], np.complex64).reshape(cells), _view(outs[3], np.float32).reshape(cells))
            if _restated(conv):
                cs.compare(got, csd_reference(nfft, hop, m, n_rows, conv), ("context order", nfft, m, conv))
        return Built([ca, cb], (4 * n_rows * nfft, 4 * n_rows * nfft, 8 * n_rows * nfft, 4 * n_rows * nfft),
                     lambda outs: dev.cross_spectrum_dev(ca, a.size, fa, cb, b.size, fb, nfft, hop, m, n_rows, outs[0], outs[1], outs[2], outs[3]),
                     check)
    return build


@functools.lru_cache(maxsize=None)
def csd_reference(nfft, hop, m, n_rows, conv):
    import csd_restatement as cs
    a, b = cs.parity_pair()
    return cs.csd(a, b, nfft, hop, m, cs.PARITY_FIRST_A, cs.PARITY_FIRST_B, n_rows, conv[0], conv[1])


# ------------------------------------------------------------------------------------------------ the needs
def _need_welch(nbytes, chunk, nperseg, captures=1):
    return lambda dev: None if dev is None else captures * int(lib().gj_welch_workspace(dev._ctx, nbytes, chunk, nperseg))


def _need_part_welch(dev):
    if dev is None:
        return None
    keep = []
    try:
        return int(dev.part_welch_workspace(_part_view(dev, keep), PART_CHUNK_SAMPLES, PART_NPERSEG))
    finally:
        for b in keep:
            b.free()


def _no_function(dev):
    return None


def _need_acq(with_power):
    def need(dev):
        c = acq_case()
        return int(lib().gj_acq_workspace(_ctx(dev), c.nsamp, c.n_freq, len(c.prns), c.intg, 1 if with_power else 0))
    return need


def _need_series(dev):
    c = acq_case()
    return int(lib().gj_acq_series_workspace(_ctx(dev), c.nsamp, c.n_freq, len(c.prns), c.intg, SERIES_EPOCHS, SERIES_EPL))


def _need_big_series(n_epochs):
    return lambda dev: int(lib().gj_acq_series_workspace(_ctx(dev), 2048, 71, len(BIG_SERIES_PRNS), 10, n_epochs, n_epochs))


def _need_peaks(dev):
    c = acq_case()
    return int(lib().gj_acq_peaks_workspace(_ctx(dev), c.nsamp, len(c.prns)))


def _need_rows(fn, nfft, m, n_rows):
    return lambda dev: int(getattr(lib(), fn)(_ctx(dev), nfft, m, n_rows))


def _need_xcorr(n):
    return lambda dev: int(lib().gj_xcorr_workspace(_ctx(dev), 3, n, len(PAIRS)))


def _need_caf(n):
    return lambda dev: int(lib().gj_xcorr_caf_workspace(_ctx(dev), 3, n, len(PAIRS), CAF_BINS, CAF_BPL))


# ------------------------------------------------------------------------------------------------ the catalogue
K5_N = 50000                      # L = 131072
W1 = (1024, 131072, 900_000)      # tests/test_round5_gpu.py's batch shapes
W2 = (4096, 200_000, 1_000_000)
ROWS = dict(nfft=256, hop=256, m=40, n_rows=8)          # three blocks per row, the last one short
ROWS_4096 = dict(nfft=4096, hop=4096, m=2, n_rows=8)
LADDER_SK = dict(nfft=256, hop=18, m=40, n_rows=176)
LADDER_CAF_N = 100_000            # L = 2^18 (tests/caf_lengths SLOT_N)
LADDER_K5_N = 600_000             # L = 2^21

_CATALOGUE = [
    Spec("chunk_power", ("gj_chunk_power_dev",), "K1: 16 bytes per chunk", True, _build_chunk_power, _no_function),
    Spec("capture_scan", ("gj_capture_scan_dev",), "fused scan + tail", True, _build_scan(True), _no_function),
    Spec("stream_scan", ("gj_stream_scan_dev",), "fused scan", True, _build_scan(False), _no_function),
    Spec("amp_stats_unaligned", ("gj_amp_stats_dev",), "scan on a copy of the capture inside the arena", True, _build_amp_onset("amp", 2), _no_function),
    Spec("amp_stats_aligned", ("gj_amp_stats_dev",), "scan, amplitude form", True, _build_amp_onset("amp", 0), _no_function),
    Spec("onset_unaligned", ("gj_onset_dev",), "scan on a copy of the capture inside the arena", True, _build_amp_onset("onset", 2), _no_function),
    Spec("onset_aligned", ("gj_onset_dev",), "scan, onset form", True, _build_amp_onset("onset", 0), _no_function),
    Spec("welch_1024", ("gj_welch_dev",), "K2 partial spectra", True, _build_welch(*W1), _need_welch(2 * W1[2], W1[1], W1[0])),
    Spec("welch_4096", ("gj_welch_dev",), "K2 partial spectra", True, _build_welch(*W2), _need_welch(2 * W2[2], W2[1], W2[0])),
    Spec("welch_timed", ("gj_welch_timed_dev",), "K2 partial spectra", True, _build_welch(*W1, timed=True), _need_welch(2 * W1[2], W1[1], W1[0]),
         waits=True),
    Spec("welch_batch", ("gj_welch_batch_dev",), "K2 partial spectra of three captures", True, _build_welch_batch(*W1),
         _need_welch(2 * W1[2], W1[1], W1[0], captures=3)),
    Spec("part_welch", ("gj_part_welch_dev",), "K2 partial spectra, planned for the whole capture", True, _build_part_welch, _need_part_welch),
    Spec("part_scan", ("gj_part_scan_dev",), "fused scan of a part", True, _build_part_scan(False), _no_function),
    Spec("part_capture_scan", ("gj_part_capture_scan_dev",), "fused scan of a part + slot", True, _build_part_scan(True), _no_function),
    Spec("xcorr_lags", ("gj_xcorr_lags_dev",), "K5 spectra, products, candidates", True, _build_xcorr(K5_N), _need_xcorr(K5_N)),
    Spec("xcorr_slots", ("gj_xcorr_slots_dev",), "K5 spectra, products, candidates", True, _build_xcorr(K5_N, slots=True), _need_xcorr(K5_N)),
    Spec("xcorr_caf", ("gj_xcorr_caf_dev",), "CAF spectra, bins of a launch, ridge candidates", True, _build_caf(K5_N), _need_caf(K5_N)),
    Spec("xcorr_caf_slots", ("gj_xcorr_caf_slots_dev",), "CAF spectra, bins of a launch, ridge candidates", True, _build_caf(K5_N, slots=True),
         _need_caf(K5_N)),
    Spec("acq_search", ("gj_acq_search_dev",), "search: flags, spectra, row records, running maxima", False, _build_acq_search(False), _need_acq(False)),
    Spec("acq_search_power", ("gj_acq_search_dev",), "search, power form: flags, spectra", False, _build_acq_search(True), _need_acq(True)),
    Spec("acq_series", ("gj_acq_series_dev",), "series: spectra, row records, running maxima per epoch", False, _build_acq_series, _need_series),
    Spec("acq_peaks", ("gj_acq_peaks_dev",), "column maxima, sums and rows", False, _build_peaks, _need_peaks),
    Spec("sk_256", ("gj_sk_dev",), "row partials, two planes", True, _build_sk(**ROWS), _need_rows("gj_sk_workspace", 256, 40, 8)),
    Spec("csd_256", ("gj_csd_dev",), "row partials, four planes", True, _build_csd(**ROWS), _need_rows("gj_csd_workspace", 256, 40, 8)),
    Spec("sk_4096", ("gj_sk_dev",), "row partials, two planes", True, _build_sk(**ROWS_4096), _need_rows("gj_sk_workspace", 4096, 2, 8)),
    Spec("csd_4096", ("gj_csd_dev",), "row partials, four planes", True, _build_csd(**ROWS_4096), _need_rows("gj_csd_workspace", 4096, 2, 8)),
    # scaled for the ladder only: more rows, a longer slice, more epochs
    Spec("sk_256_rows176", ("gj_sk_dev",), "row partials, two planes", True, _build_sk(**LADDER_SK), _need_rows("gj_sk_workspace", 256, 40, 176)),
    Spec("xcorr_caf_100000", ("gj_xcorr_caf_dev",), "CAF at L = 2^18", True, _build_caf(LADDER_CAF_N), _need_caf(LADDER_CAF_N)),
    Spec("acq_series_2048x2", ("gj_acq_series_dev",), "series, two epochs of the reference's rate in one launch", False, _build_big_series(2),
         _need_big_series(2)),
    Spec("xcorr_lags_600000", ("gj_xcorr_lags_dev",), "K5 at L = 2^21", True, _build_xcorr(LADDER_K5_N), _need_xcorr(LADDER_K5_N)),
    Spec("acq_series_2048x9", ("gj_acq_series_dev",), "series, nine epochs in one launch", False, _build_big_series(9), _need_big_series(9)),
]
SPECS = {s.name: s for s in _CATALOGUE}
assert len(SPECS) == len(_CATALOGUE)

#: the growth test: ascending by need, need[k+1] >= 2 need[k] + 2 MiB, so that every rung must replace the arena
LADDER = ("sk_256_rows176", "xcorr_lags", "xcorr_caf_100000", "acq_series_2048x2", "xcorr_lags_600000", "acq_series_2048x9")
LADDER_KERNELS = {"sk_256_rows176": "k_skurt", "xcorr_lags": "k_xcorr (K5)", "xcorr_caf_100000": "k_xcorr (CAF)", "acq_series_2048x2": "k_acq",
                  "xcorr_lags_600000": "k_xcorr (K5)", "acq_series_2048x9": "k_acq"}
#: every probe but the ladder's scaled ones: the catalogue of tests 1, 4, 5
SMALL = tuple(s.name for s in _CATALOGUE if s.name not in LADDER or s.name == "xcorr_lags")
#: those that can sit in a queue with no host wait
QUEUED = tuple(n for n in SMALL if not SPECS[n].waits)
#: the offset-honouring probes of test 6, one per kernel family, and the one that must not follow the convention
CONVENTION_PROBES = ("chunk_power", "capture_scan", "welch_1024", "xcorr_lags", "xcorr_caf", "sk_256", "csd_256")
FIXED_128_PROBE = "acq_search"
QUEUE_SEEDS = (11, 23, 37, 41, 53, 67, 79, 97)


def ladder_holds(needs):
    """[(k, need[k], need[k+1])] of the rungs that break need[k+1] >= 2 need[k] + 2 MiB."""
    return [(k, a, b) for k, (a, b) in enumerate(zip(needs, needs[1:])) if not b >= 2 * a + 2 * MiB]


def seeded_queue(seed, names=QUEUED):
    """[(probe name, slot, fill byte | None)]: every probe twice (slot 0 is its first place in the queue, slot 1 its second)
    in an order shuffled by ``seed``, a fill byte of the seed's choosing in front of every third call."""
    rng = random.Random(seed)
    order = list(names) * 2
    rng.shuffle(order)
    fill, phase = rng.choice(FILLS), rng.randrange(3)
    seen, out = {}, []
    for k, name in enumerate(order):
        out.append((name, seen.get(name, 0), fill if k % 3 == phase else None))
        seen[name] = 1
    return out


# ------------------------------------------------------------------------------------------------ who uses the arena
#: function that calls ensure_workspace or reads ctx->ws -> the extern "C" entry points that reach it (csrc/*.hip, *.h)
WORKSPACE_USERS = {
    "ensure_workspace": (),                                                        # the arena's own code
    "gj_destroy": (),
    "gj_debug_inject": (),                                                         # the fill hook of these tests
    "gj_reserve": ("gj_reserve",),
    "gj_welch_timed_dev": ("gj_welch_timed_dev",),
    "launch_chunk_power": ("gj_chunk_power_dev", "gj_stream_scan_dev", "gj_capture_scan_dev"),
    "stream_scan_impl": ("gj_stream_scan_dev", "gj_capture_scan_dev", "gj_part_scan_dev", "gj_part_capture_scan_dev"),
    "launch_amp_onset": ("gj_amp_stats_dev", "gj_onset_dev"),
    "launch_welch": ("gj_welch_dev", "gj_part_welch_dev"),
    "launch_welch_batch": ("gj_welch_batch_dev",),
    "launch_xcorr": ("gj_xcorr_lags_dev", "gj_xcorr_slots_dev"),
    "launch_xcorr_caf": ("gj_xcorr_caf_dev", "gj_xcorr_caf_slots_dev"),
    "launch_acq_search": ("gj_acq_search_dev",),
    "launch_acq_series": ("gj_acq_series_dev",),
    "acq_run": ("gj_acq_search_dev",),
    "acq_series_run": ("gj_acq_series_dev",),
    "gj_acq_peaks_dev": ("gj_acq_peaks_dev",),
    "row_workspace": ("gj_sk_dev", "gj_csd_dev"),
}
EXEMPT = {"gj_reserve": "grows the arena and launches nothing: tests 3 and 4 call it between queued probes instead of probing it"}

_FUNCTION = re.compile(r"^(?:static |inline |extern )*(?:[A-Za-z_][\w:<>]*[\s\*&]+)+(\w+)\([^;]*$")
_USE = re.compile(r"ensure_workspace\(|ctx->ws\b")


def workspace_users(csrc):
    """{function name: [file:line]} of every function in csrc/*.hip and *.h whose body calls ensure_workspace or names
    ctx->ws.  A function starts on a line at column 0 that ends without a semicolon."""
    found = {}
    for fname in sorted(os.listdir(csrc)):
        if not fname.endswith((".hip", ".h")):
            continue
        current = None
        with open(os.path.join(csrc, fname)) as f:
            for no, line in enumerate(f, 1):
                m = _FUNCTION.match(line)
                if m and not line.startswith((" ", "\t", "//", "#", "}")):
                    current = m.group(1)
                declaration = not line.startswith((" ", "\t")) and line.rstrip().endswith(";")
                if _USE.search(line.split("//")[0]) and not declaration:
                    assert current, f"{fname}:{no}: a workspace use outside any function"
                    found.setdefault(current, []).append(f"{fname}:{no}")
    return found


# ------------------------------------------------------------------------------------------------ the probe
class Probe:
    def __init__(self, dev, spec, slots=2):
        self.dev, self.spec = dev, spec
        self.built = spec.build(dev)
        self.outs = [[Guarded(dev, s) for s in self.built.out_sizes] for _ in range(slots)]

    def scrub(self, slot=0):
        for b in self.outs[slot]:
            b.refill()

    def enqueue(self, slot=0):
        self.built.launch(self.outs[slot])

    def download(self, slot=0):
        """The outputs as bytes (waits for the stream); the pads on either side of them must still hold the sentinel."""
        for k, b in enumerate(self.outs[slot]):
            b.check_pads(f"output {k} ({self.spec.name})")
        return tuple(b.read().tobytes() for b in self.outs[slot])

    def check(self, outs, conv=DEFAULT):
        self.built.check(outs, conv)

    def need(self):
        return self.spec.need(self.dev)

    def free(self):
        for b in [x for slot in self.outs for x in slot] + list(self.built.keep):
            for closer in ("close", "free"):
                if hasattr(b, closer):
                    getattr(b, closer)()
                    break
