"""The part every host double of the library shares (tests/test_*_host.py): "device memory" that is numpy buffers, the
allocation bookkeeping the tests read, the status texts ``Device._check`` asks for, and a ``Device`` that holds such a
double in place of the library.  A test file subclasses ``HostLib`` with the kernel entry points its wrappers reach,
computed by the restatements under tests/.  No GPU call is made."""
import ctypes as C

import numpy as np
import pytest

import gpsjam

GJ_ERR_INVALID = -1          # include/gpsjam.h
STATUS_TEXT = {0: b"ok", GJ_ERR_INVALID: b"invalid argument"}          # gj_strerror (csrc/api.hip)


class HostLib:
    """A "device address" is the address of a numpy buffer this object keeps alive: ``mem`` holds every allocation that
    has not been freed, ``calls`` what the test wants to read back of the calls that were made."""

    log_malloc = True        # ("malloc", nbytes) goes into ``calls``

    def __init__(self):
        self.mem, self.calls, self.last_error = {}, [], b""

    def _new(self, nbytes):
        buf = np.zeros(max(int(nbytes), 1), np.uint8)
        self.mem[buf.ctypes.data] = buf
        return buf.ctypes.data

    @staticmethod
    def view(addr, count, dtype=np.uint8):
        addr = addr.value if isinstance(addr, C.c_void_p) else int(addr)
        dt = np.dtype(dtype)
        return np.frombuffer((C.c_uint8 * (count * dt.itemsize)).from_address(addr), dt)

    def gj_malloc(self, ctx, nbytes, ref):
        if self.log_malloc:
            self.calls.append(("malloc", int(nbytes)))
        ref._obj.value = self._new(nbytes)
        return 0

    def gj_upload(self, ctx, data, nbytes, ref):
        ref._obj.value = self._new(nbytes)
        if nbytes:
            C.memmove(ref._obj.value, data, nbytes)
        return 0

    def gj_free(self, ctx, ptr):
        self.mem.pop(int(ptr), None)
        return 0

    def gj_memcpy_h2d(self, ctx, dst, src, nbytes):
        C.memmove(dst, src, nbytes)
        return 0

    gj_memcpy_d2h = gj_memcpy_h2d

    @staticmethod
    def gj_strerror(status):
        return STATUS_TEXT.get(status, b"unknown status")

    def gj_last_error(self, ctx):
        return self.last_error

    def refuse(self, entry, status=GJ_ERR_INVALID, detail=b"refused by the double"):
        """From now on ``entry`` does nothing and returns ``status``, the way the library refuses an argument."""
        def refused(*args):
            self.calls.append(("refused", entry))
            self.last_error = detail
            return status
        setattr(self, entry, refused)


def host_device(lib):
    """A ``Device`` on the double ``lib``: no library is loaded and no context is created."""
    dev = object.__new__(gpsjam.Device)
    dev._lib, dev._ctx, dev.kernel_calls, dev.cache_hits, dev.last_kernel_ms = lib, C.c_void_p(1), {}, 0, 0.0
    return dev


REFUSED_TEXT = "gpsjam: invalid argument: refused by the double (status -1)"       # Device._check on HostLib.refuse


def mallocs(lib):
    return [c[1] for c in lib.calls if c[0] == "malloc"]


def sources(dev, raw):
    """The two forms a wrapper takes its capture in: host bytes, then a resident ``Capture`` (freed behind the loop's
    body).  Yields ``(source, held)``; ``held``: what ``lib.mem`` must hold behind the call besides the call's result."""
    before = set(dev._lib.mem)
    yield raw, before
    with gpsjam.Capture(dev, raw) as cap:
        yield cap, before | {cap.ptr}


def check_refused(dev, raw, call, error, text, counted=None):
    """``call(source)`` raises ``error`` with exactly ``text``, on host bytes and on a resident capture alike; behind it
    the double holds what it held before (and the caller's capture), and nothing has been counted.  ``counted``: the
    refusal is the library's own, so the wrapper named here HAS counted the call that reached it, once."""
    for source, held in sources(dev, raw):
        calls = dict(dev.kernel_calls)
        if counted:
            calls[counted] = calls.get(counted, 0) + 1
        with pytest.raises(error) as caught:
            call(source)
        assert str(caught.value) == text
        assert set(dev._lib.mem) == held, "nothing is leaked, and the caller's capture is left alone"
        assert dev.kernel_calls == calls, "a refused call counts nothing"


def check_freed(dev, raw, call):
    """``call(capture)`` on a capture that has been freed: the one ValueError, nothing allocated, nothing counted."""
    cap = gpsjam.Capture(dev, raw)
    cap.free()
    held, calls, before = set(dev._lib.mem), dict(dev.kernel_calls), len(dev._lib.calls)
    with pytest.raises(ValueError) as caught:
        call(cap)
    assert str(caught.value) == "the capture has been freed"
    assert set(dev._lib.mem) == held and dev.kernel_calls == calls and len(dev._lib.calls) == before
