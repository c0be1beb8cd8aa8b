"""HIP streams that really run side by side.

The HIP runtime maps streams onto a small pool of hardware queues (``GPU_MAX_HW_QUEUES``, four by default; a new stream
gets the least-used queue) and two streams on ONE queue execute one after the other.  The pipelines here keep K2 on one
stream and a chain of small kernels on a second (and, on the combining rank of a split run, a third) precisely so that
they overlap -- and the kernel traces of round 4 showed both failure modes: a third stream on the main stream's queue
(K2 queued behind the combine), and, with eight queues, the deployment step's second stream on its first one's (the step
took 1.13 instead of 0.47 ms).  Which queue a stream lands on depends on every stream the process has made before, so it
cannot be arranged; it can be TESTED: keep one stream busy with a spinning wave (gj_probe_busy_dev) and see whether an
event recorded on the other completes meanwhile.

The pipelines' cross-stream step protocol is defined here once (``StepStreams``, with ``side_context``, ``PsdPingPong``,
``pair_outputs`` and ``scan_workspace``): ``gpsjam.sharded.AntennaStream`` and ``gpsjam.split.SplitStreams`` are step
pipelines over it, and ``gpsjam.local.LocalAntennas`` makes its side streams and K5 outputs with the same parts.
"""
from __future__ import annotations

import contextlib
import logging
import os
from typing import Sequence, Tuple

import torch

from ._ffi import GJ_LAG_INVALID

_log = logging.getLogger("gpsjam.streams")


def runs_beside(dev, busy_stream, other_stream, busy_ms: float = 2.0) -> bool:
    """True when work on ``other_stream`` completes while ``busy_stream`` (the stream ``dev`` is bound to) is occupied:
    the two do not share a hardware queue.

    Only the two streams involved are synchronised (a pipeline in mid-step on other streams of the device is not
    stalled), and the verdict is read from the GPU's own time stamps of two events -- ``other`` finished well before
    ``busy`` -- rather than from host polling, so a descheduled host thread cannot turn it."""
    busy_stream.synchronize()
    other_stream.synchronize()
    done_busy, done_other = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    dev.probe_busy_dev(busy_ms)                   # gj_probe_busy_dev: one spinning wave on the context's stream
    done_busy.record(busy_stream)
    done_other.record(other_stream)
    done_other.synchronize()
    done_busy.synchronize()
    return done_other.elapsed_time(done_busy) > 0.5 * busy_ms


def stream_beside_checked(against: Sequence[Tuple[object, "torch.cuda.Stream"]], device=None, priority: int = 0, tries: int = 8):
    """(stream, overlaps): a new stream and whether it runs side by side with every stream of ``against``
    ([(Device bound to it, stream), ...]).  Candidates that share a queue with one of them are kept alive until the
    search ends (so the next candidate is dealt another queue) and dropped afterwards.  If none of ``tries`` candidates
    qualifies the last one is returned with ``overlaps`` False and a warning logged: the pipeline is still correct (its
    cross-stream ordering is by events), its streams just do not overlap.  Inside a stream capture nothing can be
    probed (a synchronisation would invalidate the capture): the candidate is returned untested, with a warning."""
    if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
        _log.warning("stream_beside called inside a stream capture: the new stream is not tested for overlap")
        return torch.cuda.Stream(device=device, priority=priority), False
    rejected, cand, ok = [], None, False
    for _ in range(max(1, tries)):
        cand = torch.cuda.Stream(device=device, priority=priority)
        if all(runs_beside(dev, s, cand) for dev, s in against):
            ok = True
            break
        rejected.append(cand)
    else:
        _log.warning("no stream found that runs beside the pipeline's other streams in %d tries (GPU_MAX_HW_QUEUES=%s?): "
                     "the side chain will run behind K2 instead of beside it", tries, os.environ.get("GPU_MAX_HW_QUEUES", "4"))
    del rejected
    return cand, ok


def stream_beside(against, device=None, priority: int = 0, tries: int = 8):
    """The stream of :func:`stream_beside_checked` alone."""
    return stream_beside_checked(against, device=device, priority=priority, tries=tries)[0]


def scan_workspace(nbytes: int) -> int:
    """Workspace reserved for the fused scan (gj_capture_scan_dev, gj_part_capture_scan_dev) over ``nbytes`` capture bytes:
    its onset scratch, per-tile amplitude records, per-chunk accumulators, per-512-sample counters and tail records
    (k_scan.hip) stay well below one byte in 48 plus 1 MiB.  Reserved at construction, so that no step allocates."""
    return nbytes // 48 + (1 << 20)


def side_context(dev, against, device=None, priority: int = 0, side_device=None):
    """(context, stream, overlaps): a gpsjam context on ``dev``'s GPU (new, or ``side_device``) -- the stream's own
    workspace -- bound to a new stream tested by :func:`stream_beside_checked` against every stream of ``against``."""
    sdev = side_device if side_device is not None else type(dev)(dev.index)
    stream, ok = stream_beside_checked(against, device=device, priority=priority)
    sdev.set_stream(stream.cuda_stream)
    return sdev, stream, ok


def pair_outputs(pairs, device):
    """K5's pair table and outputs for ``pairs``: (d_pairs int32 [i, j, ...], lags int32 = LAG_INVALID, peaks f32, margins
    f32), one entry at least, so that a rank without pairs still has buffers to pack from."""
    n = max(len(pairs), 1)
    return (torch.tensor([x for p in pairs for x in p] or [0, 0], dtype=torch.int32, device=device),
            torch.full((n,), GJ_LAG_INVALID, dtype=torch.int32, device=device),
            torch.zeros(n, dtype=torch.float32, device=device), torch.zeros(n, dtype=torch.float32, device=device))


class PsdPingPong:
    """K2 writes PSD buffer i on the main stream and the packing reads it on the side stream, i = 0, 1, 0, ... step by
    step: the main stream goes on to the next step's K2 (into the other buffer) while the side stream still packs from
    this one.  K2 waits until the packing of two steps ago has read its buffer, the packing until K2 has written it.
    ``on`` False: one buffer (index 0), no events."""

    def __init__(self, main, side, on: bool):
        self.main, self.side, self.on, self.i = main, side, bool(on), 0
        self._written = [torch.cuda.Event(), torch.cuda.Event()] if self.on else None   # main: K2 has written buffer i
        self._read = [None, None]                                                        # side: the packing has read it

    def before_k2(self) -> int:
        """The buffer this step's K2 writes."""
        if self.on:
            self.i ^= 1
            if self._read[self.i] is not None:
                self.main.wait_event(self._read[self.i])
        return self.i

    def after_k2(self):
        if self.on:
            self._written[self.i].record(self.main)

    def before_pack(self):
        self.side.wait_event(self._written[self.i])

    def after_pack(self):
        if self._read[self.i] is None:
            self._read[self.i] = torch.cuda.Event()
        self._read[self.i].record(self.side)


class StepStreams:
    """The main and side stream of a pipeline step and the events between them: the one definition of the protocol.

    K2 runs on the main stream (``dev`` bound to it).  With ``overlap`` the scan, slot and K5 chain runs beside it on a
    side stream (``side_context``) with a context of its own (``dev_side``); K2 is bound by VALU issue, the scan by HBM.
        side   begin_side (waits: free)  scan ... K5  end_side (records: side done)
        main   K2  begin_pack (waits: side done)  pack  end_pack (records: free, packed)
    ``free`` lets the next step's side chain overwrite what the packing read; a collective stream follows ``packed``
    (``wait_packed``).  ``pack_on_side`` (needs ``overlap``): the packing runs on the side stream behind K5 from one of two
    PSD buffers (``PsdPingPong``), so the main stream carries K2 alone.  Without ``overlap`` (or on the CPU, ``main``
    None) there is one stream, ``_side`` is ``_main``, and no event is made or used."""

    def __init__(self, dev, main, overlap: bool, *, device=None, priority: int = 0, side_device=None,
                 pack_on_side: bool = False):
        self.dev, self._main, self.overlap = dev, main, bool(overlap)
        if main is not None:
            dev.set_stream(main.cuda_stream)     # the pipeline's torch ops, its events and the gpsjam kernels share one stream
        self.dev_side, self._side, self._own_side = dev, main, False
        self.streams_overlap = None              # one stream: nothing to overlap
        if self.overlap:
            #: False: no stream could be found that runs beside the main one (results unaffected, chains serialised)
            self.dev_side, self._side, self.streams_overlap = side_context(dev, [(dev, main)], device, priority, side_device)
            self._own_side = side_device is None
            self._ev_free, self._ev_side, self._ev_packed = torch.cuda.Event(), torch.cuda.Event(), torch.cuda.Event()
            self._ev_free.record(main)
        self._pack_on_side = bool(pack_on_side) and self.overlap
        self._psd_turn = PsdPingPong(self._main, self._side, self._pack_on_side)

    def scan(self):
        """Everything that only needs this rank's own bytes: the side chain's scan, then K2 (no host synchronisation)."""
        self.stream_scan()
        self.welch()

    def step(self):
        """One pass of the hot path: scan, TDOA (slots, exchange, K5) on the side stream, packing and result gather."""
        self.scan()
        self.tdoa()
        return self.exchange(0)

    def on_side(self):
        """Context manager: torch's current stream = the side stream (no-op without overlap)."""
        return torch.cuda.stream(self._side) if self.overlap else contextlib.nullcontext()

    def reserve(self, ws_main: int, ws_side: int):
        """Both workspaces up front (nothing is allocated inside a step): one per context, or the larger in one."""
        if self.overlap:
            self.dev.reserve(ws_main)
            self.dev_side.reserve(ws_side)
        else:
            self.dev.reserve(max(ws_main, ws_side))

    def begin_side(self):
        if self.overlap:
            self._side.wait_event(self._ev_free)

    def end_side(self):
        if self.overlap:
            self._ev_side.record(self._side)

    def begin_pack(self):
        """(stream, context) of the packing, once what it reads is written."""
        if self._pack_on_side:
            self._psd_turn.before_pack()
            return self._side, self.dev_side
        if self.overlap:
            self._main.wait_event(self._ev_side)
        return self._main, self.dev

    def end_pack(self, stream):
        if self.overlap:
            self._ev_free.record(stream)
            self._ev_packed.record(stream)
        if self._pack_on_side:
            self._psd_turn.after_pack()

    def wait_packed(self, stream):
        if self.overlap:
            stream.wait_event(self._ev_packed)

    def close(self):
        if self.overlap and self._own_side and self.dev_side is not self.dev:
            self.dev_side.close()
