"""Every user of a context's workspace arena in ONE queue: order, growth in flight, a dirty arena, the convention and the
stream at enqueue time.

This file sits in a package of its own for the reason tests/ridge/test_round6_gpu.py gives: the suite orders GPU files by
basename (tests/conftest.py SUITE_ORDER, which tests/test_suite_order.py holds every GPU file to), and under the name
test_round6_gpu.py it runs in stage 2.

The rest of the suite shares one session-wide context whose arena reaches its final size early, queues one entry point at
a time and waits after each.  A word of the arena that a kernel reads before its own call has written it then reads
whatever the allocator or the last call left there -- within a kernel's own file mostly the same kernel's right answer
in the same layout -- and whether that passes is luck.  Here the arena's contents are set.  Every test makes its OWN
context (at most two are alive at once), and the probes of tests/context_order_inputs.py -- one per entry point that uses
ctx->ws -- are queued behind one another with no host wait:

  1. alone: each probe on a fresh context passes its kernel's own check against the restatement; THESE bytes are what
     every later test expects (bit for bit: the same call on the same device; no tolerance anywhere below);
  2. growth in flight: a ladder of six probes, each needing more than twice the one before, queued behind a busy stream so
     that every rung replaces the arena while its predecessors are still queued;
  3. retired arenas: the same with gj_synchronize (which reaps) after every second rung, and with gj_reserve between rungs;
  4. every predecessor: all ordered pairs (p, q), with the whole arena filled with 0x00, 0xFF and 0x7F in front of every call;
  5. seeded random queues of all probes, each twice, with fills in front of a third of the calls;
  6. gj_set_unpack between queued calls: each result is the solitary one under ITS convention;
  7. gj_set_stream between queued calls that use one arena region by different layouts, with a growing rung behind each
     switch, and with a fill of the whole arena as the first call on the new stream while the old one is still working
     (the one form that goes red without the switch's event: profiles/NOTES_context_order.md).

Measured on an MI355X: the busy probe and the ladder's six growing calls are enqueued in 1.3 ms against the 100 ms the
stream is kept busy.

The ladder's inequality is asserted from the library's own *_workspace answers, never from a restated growth policy."""
import contextlib
import time

import pytest

import context_order_inputs as co
import gpsjam
from gpu_lib import SENTINEL

pytestmark = pytest.mark.gpu

BUSY_MS = 100.0                       # gj_probe_busy_dev's cap
_SOLO = {}


def solitary(name, conv=co.DEFAULT):
    """The outputs of one probe alone on a fresh context under ``conv``, held to the restatement; computed once."""
    key = (name, conv)
    if key not in _SOLO:
        if name == "acq_peaks":
            co.search_surface()       # on a context of its own, before this one exists
        with gpsjam.Device(0) as dev:
            dev.set_unpack(*conv)
            p = co.Probe(dev, co.SPECS[name], slots=1)
            try:
                p.enqueue()
                outs = p.download()
                p.check(outs, conv)
                p.enqueue()
                assert p.download() == outs, f"{name}: two calls on one context, different bits"
            finally:
                p.free()
        _SOLO[key] = outs
    return _SOLO[key]


@contextlib.contextmanager
def fresh(names, slots=2):
    """A new context with the named probes built on it: everything allocated and uploaded, the arena untouched."""
    dev, probes = gpsjam.Device(0), {}
    try:
        for n in names:
            probes[n] = co.Probe(dev, co.SPECS[n], slots)
        yield dev, probes
    finally:
        try:
            dev.synchronize()
        finally:
            for p in probes.values():
                p.free()
            dev.close()


def fill(dev, byte):
    dev.debug_inject(co.GJ_INJECT_FILL_WORKSPACE, byte)


def same(probes, expect, names, slot=0, what=""):
    for n in names:
        got = probes[n].download(slot)
        assert len(got) == len(expect[n])
        for k, (g, e) in enumerate(zip(got, expect[n])):
            assert g == e, f"{what}: {n}, output {k}: not the bits of the call alone"
        probes[n].scrub(slot)


# ------------------------------------------------------------------------------------------------ 1. alone
@pytest.mark.parametrize("name", [s.name for s in co._CATALOGUE])
def test_alone_against_the_restatement(name):
    outs = solitary(name)
    assert all(len(o) for o in outs)
    assert any(o != bytes([SENTINEL]) * len(o) for o in outs), "the call wrote its outputs"


# ------------------------------------------------------------------------------------------------ 2. growth in flight
def ladder_needs(probes):
    needs = [probes[n].need() for n in co.LADDER]
    assert all(isinstance(x, int) and x > 0 for x in needs)
    assert not co.ladder_holds(needs), (needs, co.ladder_holds(needs))
    assert len(needs) >= 6 and len({co.LADDER_KERNELS[n] for n in co.LADDER}) >= 4
    assert co.MiB <= needs[0] < 2 * co.MiB and needs[-1] <= 256 * co.MiB
    return needs


def test_growth_in_flight():
    expect = {n: solitary(n) for n in co.LADDER}
    with fresh(co.LADDER, slots=1) as (dev, probes):
        needs = ladder_needs(probes)
        t0 = time.perf_counter()
        dev.probe_busy_dev(BUSY_MS)
        for n in co.LADDER:
            probes[n].enqueue()
        ms = 1e3 * (time.perf_counter() - t0)
        print(f"ladder needs (MiB): {[round(x / co.MiB, 2) for x in needs]}; busy probe + {len(co.LADDER)} growing calls enqueued in "
              f"{ms:.2f} ms of host time against a stream kept busy for {BUSY_MS:.0f} ms")
        assert ms < BUSY_MS, f"the enqueues took {ms:.1f} ms: the arena was not replaced under queued work"
        same(probes, expect, co.LADDER, what="ascending, every rung replaces the arena")
        dev.probe_busy_dev(BUSY_MS)
        for n in co.LADDER:
            probes[n].enqueue()
        same(probes, expect, co.LADDER, what="ascending on the full-size arena")
        dev.probe_busy_dev(BUSY_MS)
        for n in reversed(co.LADDER):
            probes[n].enqueue()
        same(probes, expect, co.LADDER, what="descending on the full-size arena")


# ------------------------------------------------------------------------------------------------ 3. retired arenas
def test_retired_arenas_are_reaped_between_rungs():
    expect = {n: solitary(n) for n in co.LADDER}
    with fresh(co.LADDER, slots=1) as (dev, probes):
        ladder_needs(probes)
        for k, n in enumerate(co.LADDER):
            if k % 2 == 0:
                dev.probe_busy_dev(10.0)
            probes[n].enqueue()
            if k % 2 == 1:
                dev.synchronize()         # reaps the arenas the two rungs retired
        same(probes, expect, co.LADDER, what="gj_synchronize after every second rung")


def test_reserve_between_queued_rungs():
    expect = {n: solitary(n) for n in co.LADDER}
    with fresh(co.LADDER, slots=1) as (dev, probes):
        needs = ladder_needs(probes)
        t0 = time.perf_counter()
        dev.probe_busy_dev(BUSY_MS)
        for k, n in enumerate(co.LADDER):
            probes[n].enqueue()
            if k + 1 < len(needs) and k % 2 == 0:
                dev.reserve(needs[k + 1])  # replaces the arena that the rung just queued is going to use
        ms = 1e3 * (time.perf_counter() - t0)
        print(f"busy probe + ladder with gj_reserve behind rungs 0, 2, 4: {ms:.2f} ms of host time")
        assert ms < BUSY_MS
        same(probes, expect, co.LADDER, what="gj_reserve between queued rungs")


# ------------------------------------------------------------------------------------------------ 4. every predecessor
@pytest.mark.parametrize("byte", co.FILLS, ids=[f"fill_{b:02x}" for b in co.FILLS])
def test_every_predecessor_on_a_dirty_arena(byte):
    names = co.SMALL
    expect = {n: solitary(n) for n in names}
    with fresh(names) as (dev, probes):
        needs = [x for x in (p.need() for p in probes.values()) if x]
        dev.reserve(max(needs))
        for n in names:                   # the probes without a *_workspace function bring the arena to its final size
            probes[n].enqueue()
        dev.synchronize()
        for p in probes.values():
            p.scrub()
        t0 = time.perf_counter()
        for pn in names:
            for qn in names:
                fill(dev, byte)
                probes[pn].enqueue(0)
                fill(dev, byte)
                probes[qn].enqueue(1)
                got = probes[qn].download(1)
                assert got == expect[qn], f"fill {byte:#04x}: {qn} behind {pn}: output {[g == e for g, e in zip(got, expect[qn])].index(False)} differs"
                probes[qn].scrub(1)
        print(f"fill {byte:#04x}: {len(names) ** 2} ordered pairs of {len(names)} probes in {time.perf_counter() - t0:.2f} s")


# ------------------------------------------------------------------------------------------------ 5. seeded random queues
@pytest.mark.parametrize("seed", co.QUEUE_SEEDS)
def test_seeded_random_queue(seed):
    names = co.QUEUED
    queue = co.seeded_queue(seed, names)
    expect = {n: solitary(n) for n in names}
    with fresh(names) as (dev, probes):
        t0 = time.perf_counter()
        dev.probe_busy_dev(BUSY_MS)
        for n, slot, byte in queue:
            if byte is not None:
                fill(dev, byte)
            probes[n].enqueue(slot)
        ms = 1e3 * (time.perf_counter() - t0)
        print(f"seed {seed}: {len(queue)} calls and {sum(b is not None for _, _, b in queue)} fills enqueued in {ms:.2f} ms of host time")
        for slot in (0, 1):
            same(probes, expect, names, slot, what=f"seed {seed}, place {slot + 1} in the queue")


# ------------------------------------------------------------------------------------------------ 6. the convention at enqueue time
def test_the_convention_is_the_one_at_enqueue_time():
    names = co.CONVENTION_PROBES + (co.FIXED_128_PROBE,)
    expect = {(n, c): solitary(n, c) for n in names for c in co.CONVENTIONS}
    for n in co.CONVENTION_PROBES:
        assert co.SPECS[n].honours_unpack and expect[(n, co.CONVENTIONS[0])] != expect[(n, co.CONVENTIONS[1])], f"{n} follows the convention"
    assert not co.SPECS[co.FIXED_128_PROBE].honours_unpack
    for c in co.CONVENTIONS:
        assert expect[(co.FIXED_128_PROBE, c)] == expect[(co.FIXED_128_PROBE, co.DEFAULT)], "the acquisition search always unpacks with 128"
    with fresh(names, slots=len(co.CONVENTIONS)) as (dev, probes):
        dev.probe_busy_dev(BUSY_MS)
        for n in names:
            for slot, conv in enumerate(co.CONVENTIONS):
                dev.set_unpack(*conv)
                probes[n].enqueue(slot)
        dev.set_unpack()
        for slot, conv in enumerate(co.CONVENTIONS):
            same(probes, {n: expect[(n, conv)] for n in names}, names, slot, what=f"unpack {conv}")
        assert dev.get_unpack() == co.DEFAULT


# ------------------------------------------------------------------------------------------------ 7. the stream switch
@pytest.mark.parametrize("rungs", [(), ("xcorr_caf_100000", "acq_series_2048x2")], ids=["one_arena", "a_growing_rung_behind_each_switch"])
def test_the_stream_switch_orders_two_layouts_of_one_region(rungs):
    import torch
    names = ("csd_256", "sk_256", "xcorr_lags") + rungs
    expect = {n: solitary(n) for n in names}
    side = torch.cuda.Stream()
    with fresh(names, slots=1) as (dev, probes):
        if rungs:
            needs = [probes[n].need() for n in ("csd_256",) + rungs]
            assert not co.ladder_holds(needs), needs
        try:
            dev.probe_busy_dev(BUSY_MS)
            probes["csd_256"].enqueue()
            dev.set_stream(side.cuda_stream)
            if rungs:
                probes[rungs[0]].enqueue()
            probes["sk_256"].enqueue()            # the cross-spectrum's region, by the kurtosis' layout
            dev.set_stream(None, external=False)
            if rungs:
                probes[rungs[1]].enqueue()
            probes["xcorr_lags"].enqueue()
            dev.synchronize()
        finally:
            dev.set_stream(None, external=False)
            side.synchronize()
        same(probes, expect, names, what="across two stream switches")


def test_the_stream_switch_holds_back_a_fill_until_the_old_stream_is_done():
    """The first call on the new stream is a memset over the whole arena, and the old stream is running the ladder's
    largest rung twice (three launches each over 200 MiB of spectra, row records and running maxima): only the event of
    gj_set_stream keeps the fill from landing in the middle of them.  No busy probe in front: the rung itself is the work
    in flight."""
    import torch
    big = co.LADDER[-1]
    names = (big, "sk_256", "xcorr_lags")
    expect = {n: solitary(n) for n in names}
    side = torch.cuda.Stream()
    with fresh(names) as (dev, probes):
        probes[big].enqueue(0)
        dev.synchronize()                          # the arena has its size; nothing is queued
        probes[big].scrub(0)
        try:
            probes[big].enqueue(0)
            probes[big].enqueue(1)
            dev.set_stream(side.cuda_stream)
            fill(dev, 0xFF)
            probes["sk_256"].enqueue()
            dev.set_stream(None, external=False)
            fill(dev, 0x7F)
            probes["xcorr_lags"].enqueue()
            dev.synchronize()
        finally:
            dev.set_stream(None, external=False)
            side.synchronize()
        same(probes, expect, names, 0, what="a fill right behind the switch")
        same(probes, expect, (big,), 1, what="a fill right behind the switch, the rung's second call")
