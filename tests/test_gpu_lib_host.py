"""tests/gpu_lib.py on the host double of tests/host_lib.py: a guard that never fires is worth nothing, so every check the
GPU tests lean on -- the pads of a Guarded buffer, the refusal loop, the value cache, the run_<entry> functions -- is
shown to pass on a clean call and to FAIL on one stray byte, a wrong status or a call that went through.  No GPU call
is made."""
import numpy as np
import pytest

import gpsjam
import gpu_lib
from gpu_lib import GJ_ERR_INVALID, GJ_ERR_UNSUPPORTED, PAD, SENTINEL, Guarded, Resident, refused
from host_lib import HostLib, host_device, mallocs


class Lib(HostLib):
    """Kernel entry points that write exactly their outputs -- counting patterns, never the sentinel -- and, when
    ``stray`` names an output, one byte more: right behind it (+1) or right in front of it (-1)."""

    stray = None             # (index of the output among the call's outputs, +1 or -1)

    @staticmethod
    def gj_synchronize(ctx):
        return 0

    def _write(self, k, addr, values):
        data = np.ascontiguousarray(values).reshape(-1).view(np.uint8)
        assert not np.any(data == SENTINEL)
        self.view(addr, data.size)[:] = data
        if self.stray is not None and self.stray[0] == k:
            self.view(addr + (data.size if self.stray[1] > 0 else -1), 1)[0] = 0x11

    def gj_blank_dev(self, ctx, d_iq, nbytes, first, n_samples, window, guard, threshold, d_out, d_blocks):
        self._write(0, d_out, blank_bytes(n_samples))
        if d_blocks:
            self._write(1, d_blocks, blank_records(n_samples))
        return 0

    def gj_ridge_dev(self, ctx, d_iq, nbytes, first, nfft, hop, n_frames, guard, d_out):
        self._write(0, d_out, ridge_records(n_frames))
        return 0

    def gj_sk_dev(self, ctx, d_iq, nbytes, first, nfft, hop, m, n_rows, d_s1, d_s2, d_sk):
        for k, d in enumerate((d_s1, d_s2, d_sk)):
            if d:
                self._write(k, d, sk_plane(k, n_rows, nfft))
        return 0


def blank_bytes(n_samples):
    return (np.arange(2 * n_samples) % 100).astype(np.uint8)


def blank_records(n_samples):
    rec = np.zeros(gpsjam.blank_blocks(n_samples), gpsjam.BLANK_DTYPE)
    rec["total"], rec["removed"], rec["n_blanked"], rec["n_rising"] = 1000 + np.arange(rec.size), 7, 3, np.arange(rec.size)
    return rec


def ridge_records(n_frames):
    rec = np.zeros(n_frames, gpsjam.RIDGE_DTYPE)
    rec["total"], rec["peak"], rec["second"], rec["peak_bin"] = 4.0 + np.arange(n_frames), 2.0, 1.0, np.arange(n_frames)
    return rec


def sk_plane(k, n_rows, nfft):
    return (1.0 + k + np.arange(n_rows * nfft, dtype=np.float32)).reshape(n_rows, nfft)


@pytest.fixture
def lib():
    return Lib()


@pytest.fixture
def dev(lib):
    return host_device(lib)


def poke(lib, addr):
    lib.view(addr, 1)[0] = 0x11


# ------------------------------------------------------------------------------------------------ Guarded
@pytest.mark.parametrize("fill", [True, False])
@pytest.mark.parametrize("offset", [0, 3])
def test_guarded_catches_one_byte_on_either_side(lib, dev, offset, fill):
    n = 1000
    strays = {"ptr - 1": -1, "ptr + nbytes": n, "the front pad's far end": -PAD - offset, "the rear pad's far end": n + PAD - 1}
    for where, at in strays.items():
        g = Guarded(dev, n, offset, fill=fill)
        assert g.ptr == g.buf.ptr + PAD + offset and g.nbytes == n
        g.check_pads("a buffer nobody wrote")
        lib.view(g.ptr, n)[:] = 0x22                         # an exact fill of the payload passes
        g.check_pads("a payload filled to its last byte")
        assert np.all(g.read() == 0x22) and g.read(np.uint16, 2, 6).tolist() == [0x2222, 0x2222]
        poke(lib, g.ptr + at)
        with pytest.raises(AssertionError, match="outside the call's output"):
            g.check_pads("output")
        g.free()
    assert lib.mem == {}, "free() gives the whole allocation back"


def test_guarded_check_untouched_sees_one_payload_byte(lib, dev):
    for at in (0, 499, 999, -1, 1000):
        g = Guarded(dev, 1000, 3)
        g.check_untouched("nothing was written")
        poke(lib, g.ptr + at)
        with pytest.raises(AssertionError, match="refused calls: bytes were written"):
            g.check_untouched("refused calls")
        g.free()


def test_guarded_is_a_buffer_whose_address_is_the_payloads(lib, dev):
    g = Guarded(dev, 64)
    assert gpsjam._ptr(g) == g.ptr == g.buf.ptr + PAD
    g.upload(np.arange(8, dtype=np.uint8), offset=8)
    assert g.read(np.uint8, 8, 8).tolist() == list(range(8)) and g.download(np.uint8, 8, 8).tolist() == list(range(8))
    assert np.all(g.download(np.uint8, PAD, 64) == SENTINEL), "download counts from the payload: this is the rear pad"
    g.check_pads("an upload inside the payload")
    with g:
        pass
    assert g.ptr == 0 and lib.mem == {}


def test_guarded_refilled_for_a_shorter_payload(lib, dev):
    """floor_result's use: one buffer over many calls, the rear pad right behind each call's own length."""
    g = Guarded(dev, 64)
    lib.view(g.ptr, 64)[:] = 0x22
    g.refill(10)
    assert g.nbytes == 10 and np.all(g.read() == SENTINEL)
    lib.view(g.ptr, 10)[:] = 0x33
    g.check_pads("ten bytes")
    poke(lib, g.ptr + 10)
    with pytest.raises(AssertionError):
        g.check_pads("an eleventh byte")
    g.refill()
    assert g.nbytes == 64
    g.check_untouched("refilled whole")
    g.free()


# ------------------------------------------------------------------------------------------------ refused
def refusing(status, write_at=None):
    def launch(lib, *args):
        if write_at is not None:
            poke(lib, write_at)
        raise gpsjam.GpsJamError(status, "refused by the double")
    return launch


def test_refused_passes_on_clean_refusals_and_fails_on_anything_else(lib, dev):
    out, rec = Guarded(dev, 100), Guarded(dev, 48)
    cases = [((lib, 1), GJ_ERR_INVALID), ((lib, 2, 3), GJ_ERR_INVALID)]
    refused(dev, refusing(GJ_ERR_INVALID), cases, out, rec)
    refused(dev, refusing(GJ_ERR_UNSUPPORTED), [((lib,), GJ_ERR_UNSUPPORTED)], out, rec)
    with pytest.raises(pytest.fail.Exception, match="DID NOT RAISE"):
        refused(dev, lambda *args: None, cases, out, rec)                           # a call that went through
    with pytest.raises(AssertionError):
        refused(dev, refusing(GJ_ERR_UNSUPPORTED), cases, out, rec)                 # another status
    with pytest.raises(AssertionError):
        refused(dev, refusing(GJ_ERR_INVALID), cases[:1] + [((lib,), GJ_ERR_UNSUPPORTED)], out, rec)
    for g, at in ((out, 0), (out, 99), (out, -1), (out, 100), (rec, 17), (rec, 48 + PAD - 1)):
        with pytest.raises(AssertionError, match="refused calls: bytes were written"):
            refused(dev, refusing(GJ_ERR_INVALID, g.ptr + at), cases, out, rec)     # the right status, and one byte written
        g.refill()
    refused(dev, refusing(GJ_ERR_INVALID), cases, out, rec)


# ------------------------------------------------------------------------------------------------ the value cache
def test_resident_allocates_equal_values_once_per_dtype(lib, dev):
    res = Resident(dev)
    a = res(np.full(16, -1.0))
    assert res(np.full(16, -1.0)) is a and res([-1.0] * 16, np.float32) is a and mallocs(lib) == [64]
    assert a.download(np.float32).tolist() == [-1.0] * 16
    b = res(np.zeros(16), np.float32)
    c = res(np.zeros(16), np.int32)                         # the same bytes under another dtype: a second buffer
    assert b is not a and c is not b and mallocs(lib) == [64, 64, 64]
    assert res(np.zeros(16, np.int64), np.int32) is c and len(mallocs(lib)) == 3
    res.free()
    assert lib.mem == {}


# ------------------------------------------------------------------------------------------------ run_<entry>
N_BLANK = 2 * 4096 + 5


def test_run_blank_returns_the_bytes_and_the_records(lib, dev):
    got, rec = gpu_lib.run_blank(dev, 1 << 20, 2 * N_BLANK, 0, N_BLANK, 16, 8, 1.0)
    assert got.tobytes() == blank_bytes(N_BLANK).tobytes() and rec.tobytes() == blank_records(N_BLANK).tobytes()
    got, rec = gpu_lib.run_blank(dev, 1 << 20, 2 * N_BLANK, 0, N_BLANK, 16, 8, 1.0, want_blocks=False)
    assert got.tobytes() == blank_bytes(N_BLANK).tobytes() and rec.size == gpsjam.blank_blocks(N_BLANK)
    assert np.all(rec.view(np.uint8) == SENTINEL), "records that were not asked for come back as they were"
    assert lib.mem == {}


def test_run_ridge_returns_the_records(lib, dev):
    got = gpu_lib.run_ridge(dev, 1 << 20, 4096, 256, 128, 0, 9, 2)
    assert got.dtype == gpsjam.RIDGE_DTYPE and got.tobytes() == ridge_records(9).tobytes() and lib.mem == {}


def test_run_sk_returns_the_planes_and_none_for_the_one_not_asked_for(lib, dev):
    s1, s2, skv = gpu_lib.run_sk(dev, 1 << 20, 1 << 16, 64, 32, 0, 4, 5)
    for k, plane in enumerate((s1, s2, skv)):
        assert plane.shape == (5, 64) and plane.tobytes() == sk_plane(k, 5, 64).tobytes()
    s1, s2, none = gpu_lib.run_sk(dev, 1 << 20, 1 << 16, 64, 32, 0, 4, 5, want_sk=False)
    assert none is None and s1.tobytes() == sk_plane(0, 5, 64).tobytes() and s2.tobytes() == sk_plane(1, 5, 64).tobytes()
    assert lib.mem == {}


RUNS = {"blank": (lambda dev: gpu_lib.run_blank(dev, 1 << 20, 2 * N_BLANK, 0, N_BLANK, 16, 8, 1.0), 2),
        "ridge": (lambda dev: gpu_lib.run_ridge(dev, 1 << 20, 4096, 256, 128, 0, 9, 2), 1),
        "kurtosis": (lambda dev: gpu_lib.run_sk(dev, 1 << 20, 1 << 16, 64, 32, 0, 4, 5), 3)}


@pytest.mark.parametrize("side", [+1, -1], ids=["behind", "in_front"])
@pytest.mark.parametrize("name", list(RUNS))
def test_run_fails_on_one_byte_outside_any_output(lib, dev, name, side):
    run, n_outputs = RUNS[name]
    for k in range(n_outputs):
        lib.stray = (k, side)
        with pytest.raises(AssertionError, match="bytes were written outside the call's"):
            run(dev)
        assert lib.mem == {}, "every buffer is freed behind a failed check too"
    lib.stray = None
    run(dev)
