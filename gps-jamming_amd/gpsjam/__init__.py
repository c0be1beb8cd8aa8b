"""gpsjam -- host side of the MI355X jamming-detection DSP path.

``Device`` owns one ``gj_ctx`` (one GPU) and exposes the C-ABI of
``libgpsjam_hip.so`` in two flavours:

* host arrays in, numpy results out (``chunk_power``, ``welch``, ``amp_stats``,
  ``onset``, ``xcorr_lags``) -- what the drop-in modules under ``skrypty/`` and
  ``GpsJammerApp/app/`` call;
* device pointers in / out (``*_dev``) on a caller-supplied HIP stream -- what
  ``bench.py`` and the one-capture-per-GPU driver (``gpsjam.sharded``) call with torch
  tensors.

Nothing in this package computes on the CPU: without the HIP library every call
raises ``GpsJamLibraryError``.
"""
from __future__ import annotations

import contextlib
import ctypes as C
from typing import NamedTuple, Optional, Sequence

import numpy as np

from . import _bands, _ffi
from ._ffi import (AmpStats, GpsJamError, GpsJamLibraryError, Onset, SynthParams,  # noqa: F401
                   GJ_LAG_INVALID, GJ_MAX_ANTENNAS)

__all__ = ["Device", "DevBuf", "Capture", "GpsJamError", "GpsJamLibraryError", "device_count",
           "library_path", "as_u8", "default_device", "read_capture", "resident_capture",
           "release_resident", "CafPeak", "xcorr_fft_len", "xcorr_bin_hz", "caf_bin_range", "Ridge", "RIDGE_DTYPE",
           "ridge_frames", "EXCISE_DTYPE", "excise_frames", "SpectralKurtosis", "sk_rows", "ChirpScan", "CHIRP_DTYPE",
           "BLANK_DTYPE", "BLANK_BLOCK", "blank_blocks", "FINE_BLOCK", "FINE_MAX_HALF", "fine_blocks", "FineCorr",
           "CrossSpectrum", "csd_rows", "CANCEL_DTYPE", "CORR_MAX_BLOCK", "CORR_CHANNEL_DTYPE", "corr_blocks", "CorrBank",
           "ACQ_MAX_PEAKS", "ACQ_PEAK_DTYPE", "ACQ_FLOOR_DTYPE", "SUB_BLOCK", "SUB_DTYPE", "SUB_FRAC", "SUB_MAX_AMP",
           "subtract_blocks", "ALIGN_BLOCK", "ALIGN_DTYPE", "ALIGN_PHASES", "ALIGN_TAPS", "ALIGN_ROT_LEN", "AlignParams",
           "align_blocks", "TRACK_MAX_CHANNELS", "TRACK_MAX_EPOCHS", "TRACK_MAX_GAIN", "TRACK_STATE_DTYPE", "TRACK_EPOCH_DTYPE", "SUB_TRACK_CHANNEL_DTYPE",
           "TrackParams"]

_default = None
_default_lock = __import__("threading").Lock()


def default_device() -> "Device":
    """Process-wide context used by the drop-in modules (GPU index from GPSJAM_DEVICE,
    default 0).  Raises if the HIP library or the GPU is missing -- there is no CPU path."""
    global _default
    with _default_lock:
        if _default is None or _default._ctx is None:
            _default = Device(int(__import__("os").environ.get("GPSJAM_DEVICE", "0")))
        return _default


def read_capture(path) -> np.ndarray:
    """uint8 view of a capture file without copying it through Python (memory-mapped;
    empty files give an empty array)."""
    import os
    if os.path.getsize(path) == 0:
        return np.zeros(0, np.uint8)
    return np.memmap(path, dtype=np.uint8, mode="r")


_resident = {}            # (realpath, size, mtime_ns) -> Capture, insertion order = LRU order
_resident_loading = {}    # key -> (threading.Event, kernel thread id of the loading thread): an upload in flight
_resident_lock = __import__("threading").Lock()


def resident_capture(path, **ingest) -> "Capture":
    """The capture file ``path`` in HBM on the default device, uploaded on first use and kept
    (process-wide, least-recently-used eviction above GPSJAM_RESIDENT_GIB, default 64 of the
    288 GB; an evicted capture is freed once nobody holds it any more): the worker's power scan, the RSSI solver and the PSD script all read the same
    files (worker.py:209-217 -> :590-600 -> triangulateRSSI.py:29), and each used to pay its own
    host->device pass.  ``ingest`` (keyword arguments of ``Device.ingest``): what the caller is about to
    compute -- on the first use of a file it is computed WHILE the file uploads and rides on the Capture; a
    file that is already resident is returned as it is (the caller's call then runs on it as usual).
    Raises FileNotFoundError like open().

    The cache lock is held for dictionary operations only, never across an upload: two threads bringing in
    different files do not wait for each other, and a thread that is stopped inside its upload (the GUI ends an
    analysis with QThread.terminate(), ui_mainwindow.py:818-826) leaves nothing locked -- a second caller of the
    same file waits for the upload in flight only while the thread that started it is alive, then takes over."""
    import os
    import threading
    st = os.stat(path)
    key = (os.path.realpath(path), st.st_size, st.st_mtime_ns)
    dev = default_device()
    while True:
        with _resident_lock:
            cap = _resident.pop(key, None)
            if cap is not None and cap.ptr and cap.dev is dev:
                _resident[key] = cap                      # most recently used last
                return cap
            pending = _resident_loading.get(key)
            if pending is not None and not _thread_alive(pending[1]):
                pending[0].set()                          # its loader is gone: whoever waits may try again
                del _resident_loading[key]
                pending = None
            if pending is None:
                mine = threading.Event()
                _resident_loading[key] = (mine, threading.get_native_id())
                limit = int(float(os.environ.get("GPSJAM_RESIDENT_GIB", "64")) * (1 << 30))
                while _resident and sum(c.nbytes for c in _resident.values()) + st.st_size > limit:
                    # eviction only drops the cache's reference: a caller that still holds the Capture (a scan
                    # running in another thread) keeps it alive, and its memory is freed when that reference goes
                    _resident.pop(next(iter(_resident)))
                break
        pending[0].wait(0.05)                             # short waits: the loader's liveness is re-checked above
    try:
        cap = dev.ingest(path, **ingest) if ingest else dev.capture(path)
        with _resident_lock:
            _resident[key] = cap
        return cap
    finally:
        with _resident_lock:
            if _resident_loading.get(key, (None,))[0] is mine:
                del _resident_loading[key]
        mine.set()


def _thread_alive(native_id) -> bool:
    """Kernel thread ``native_id`` of this process still exists (works for threads Python did not start, such as
    a QThread: the threading module does not know when those end)."""
    import os
    return os.path.exists(f"/proc/self/task/{native_id}")


def release_resident():
    """Free every cached capture (tests; long-running hosts that switch file sets)."""
    with _resident_lock:
        caps = list(_resident.values())
        _resident.clear()
    for c in caps:
        c.free()


def library_path() -> str:
    return _ffi.LIB_PATH


def device_count() -> int:
    n = C.c_int(0)
    _ffi.load().gj_device_count(C.byref(n))
    return n.value


def xcorr_fft_len(n_samples: int) -> int:
    """FFT length L of K5 and of the cross-ambiguity search for a slice of n_samples (gj_xcorr_fft_len)."""
    return int(_ffi.load().gj_xcorr_fft_len(int(n_samples)))


def xcorr_bin_hz(n_samples: int, fs: float = 2.048e6) -> float:
    """Width of one frequency bin of ``Device.xcorr_caf`` for slices of n_samples: fs / L."""
    return float(fs) / xcorr_fft_len(n_samples)


def caf_bin_range(n_samples: int, max_offset_hz: float, fs: float = 2.048e6):
    """(bin_first, n_bins) of the symmetric bin range that covers +-max_offset_hz."""
    k = int(np.ceil(abs(float(max_offset_hz)) / xcorr_bin_hz(n_samples, fs) - 1e-9))
    return -k, 2 * k + 1


class CafPeak(NamedTuple):
    """One pair of ``Device.xcorr_caf``: the maximum of |correlate(slice_j rotated by -bin, slice_i)| over lag and bin
    (gj_caf_result, include/gpsjam.h).  ``offset_hz`` = bin * fs / L: receiver j sees the source that much higher."""
    lag: int
    bin: int
    offset_hz: float
    peak: float
    margin_lag: float
    margin_bin: float


RIDGE_DTYPE = np.dtype([("total", np.float32), ("peak", np.float32), ("second", np.float32), ("peak_bin", np.int32)])


def ridge_frames(nbytes: int, first_sample: int, nfft: int, hop: int) -> int:
    """Whole frames of nfft points that fit from first_sample at the given hop (gj_ridge_frames); 0 when none do."""
    if min(int(nbytes), int(first_sample), int(hop)) < 0 or not -2 ** 31 <= int(nfft) < 2 ** 31:
        return 0
    return int(_ffi.load().gj_ridge_frames(int(nbytes), int(first_sample), int(nfft), int(hop)))


EXCISE_DTYPE = np.dtype([("total", np.float32), ("removed", np.float32), ("n_excised", np.int32), ("reserved", np.int32)])

# gj_cancel_frame: one frame of the two-antenna canceller
CANCEL_DTYPE = np.dtype([("total_in", np.float32), ("total", np.float32), ("removed", np.float32), ("n_excised", np.int32)])


def excise_frames(n_samples: int, nfft: int) -> int:
    """Frames of the excisor over n_samples at nfft points, hop nfft // 2 (gj_excise_frames); 0 when none fits."""
    if int(n_samples) < 0 or not -2 ** 31 <= int(nfft) < 2 ** 31:
        return 0
    return int(_ffi.load().gj_excise_frames(int(n_samples), int(nfft)))


BLANK_BLOCK = _ffi.GJ_BLANK_BLOCK
BLANK_DTYPE = np.dtype([("total", np.uint64), ("removed", np.uint64), ("n_blanked", np.int32), ("n_rising", np.int32)])


def blank_blocks(n_samples: int) -> int:
    """Records of the pulse blanker over n_samples: one per BLANK_BLOCK samples, the last one ragged (gj_blank_blocks)."""
    if not 0 <= int(n_samples) < 2 ** 64:
        return 0
    return int(_ffi.load().gj_blank_blocks(int(n_samples)))


FINE_BLOCK = _ffi.GJ_FINE_BLOCK
FINE_MAX_HALF = _ffi.GJ_FINE_MAX_HALF


def fine_blocks(n_samples: int) -> int:
    """Block records of the lag-window correlation over n_samples: one per FINE_BLOCK samples, the last one ragged
    (gj_fine_blocks)."""
    if not 0 <= int(n_samples) < 2 ** 64:
        return 0
    return int(_ffi.load().gj_fine_blocks(int(n_samples)))


class FineCorr(NamedTuple):
    """``Device.xcorr_fine``: correlate(x_b, x_a, 'full') at the lags ``lags`` in K5's unpacking, from the exact integers
    of gj_xcorr_fine_dev (c = C4 / 4: exact in complex128 up to 2^53 / 4 per part).  ``blocks[m]`` is the same over the
    m-th FINE_BLOCK samples of a alone (None unless asked for); the rows sum to ``c``."""
    lags: np.ndarray        # int64[2R+1]
    c: np.ndarray           # complex128[2R+1]
    blocks: Optional[np.ndarray]   # complex128[blocks][2R+1] or None
    n_samples: int


CORR_MAX_BLOCK = _ffi.GJ_CORR_MAX_BLOCK
CORR_CHANNEL_DTYPE = np.dtype([("code_phase", np.uint64), ("code_step", np.uint64), ("carr_phase", np.uint32),
                               ("carr_step", np.uint32), ("code_row", np.int32), ("reserved", np.int32)])


def corr_blocks(n_samples: int, block_samples: int) -> int:
    """Block records of the correlator bank over n_samples: one per block_samples samples, the last one ragged
    (gj_corr_blocks)."""
    if not 0 <= int(n_samples) < 2 ** 64 or not 1 <= int(block_samples) < 2 ** 31:
        return 0
    return int(_ffi.load().gj_corr_blocks(int(n_samples), int(block_samples)))


class CorrBank(NamedTuple):
    """``Device.corr_bank``: the exact integers of gj_corr_bank_dev.  ``iq[ch, m, j]`` = (I, Q) of channel ch, block m
    (``block_samples`` samples, the last one ragged) and tap ``taps[j]`` (whole samples; 0 is the prompt)."""
    iq: np.ndarray          # int32[n_channels][n_blocks][n_taps][2]
    taps: tuple
    block_samples: int
    n_samples: int

    def tap(self, offset: int = 0) -> np.ndarray:
        """complex128[n_channels][n_blocks]: I + jQ of the tap at ``offset`` samples (default: the prompt)."""
        j = self.taps.index(int(offset))
        return self.iq[:, :, j, 0].astype(np.float64) + 1j * self.iq[:, :, j, 1].astype(np.float64)


SUB_BLOCK = _ffi.GJ_SUB_BLOCK
SUB_FRAC = _ffi.GJ_SUB_FRAC
SUB_MAX_AMP = _ffi.GJ_SUB_MAX_AMP
SUB_DTYPE = np.dtype([("total", np.uint64), ("removed", np.uint64), ("n_clipped", np.int32), ("reserved", np.int32)])


def subtract_blocks(n_samples: int) -> int:
    """Records of the counterfeit-signal subtraction over n_samples: one per SUB_BLOCK samples, the last one ragged
    (gj_subtract_blocks)."""
    if not 0 <= int(n_samples) < 2 ** 64:
        return 0
    return int(_ffi.load().gj_subtract_blocks(int(n_samples)))


ALIGN_BLOCK = _ffi.GJ_ALIGN_BLOCK
ALIGN_PHASES = _ffi.GJ_ALIGN_PHASES
ALIGN_TAPS = _ffi.GJ_ALIGN_TAPS
ALIGN_ROT_LEN = _ffi.GJ_ALIGN_ROT_LEN
ALIGN_DTYPE = np.dtype([("power_out", np.uint64), ("n_clipped", np.int32), ("n_edge", np.int32)])
AlignParams = _ffi.AlignParams


def align_blocks(n_out: int) -> int:
    """Records of the pair alignment over n_out output samples: one per ALIGN_BLOCK samples, the last one ragged
    (gj_align_blocks)."""
    if not 0 <= int(n_out) < 2 ** 64:
        return 0
    return int(_ffi.load().gj_align_blocks(int(n_out)))


def _align_params(params) -> "_ffi.AlignParams":
    """An ``AlignParams`` as it is; ``(pos0, pos_step, rot_phase, rot_step)`` made into one (the phases modulo 2^32)."""
    if isinstance(params, _ffi.AlignParams):
        return params
    pos0, pos_step, rot_phase, rot_step = (int(v) for v in params)
    if not -2 ** 63 <= pos0 < 2 ** 63 or not 0 <= pos_step < 2 ** 64:
        raise GpsJamError(-5, "unsupported: a position outside 64 bits")
    return _ffi.AlignParams(pos0, pos_step, rot_phase & 0xFFFFFFFF, rot_step & 0xFFFFFFFF, 0)


TRACK_MAX_CHANNELS = _ffi.GJ_TRACK_MAX_CHANNELS
TRACK_MAX_EPOCHS = _ffi.GJ_TRACK_MAX_EPOCHS
TRACK_MAX_GAIN = _ffi.GJ_TRACK_MAX_GAIN
TRACK_STATE_DTYPE = np.dtype([("ch", CORR_CHANNEL_DTYPE), ("carr_nco", np.int64), ("start", np.uint32), ("e_prev", np.int32),
                              ("c_prev", np.int32), ("primed", np.int32), ("reserved", np.int32, (2,))])      # gj_track_state
TRACK_EPOCH_DTYPE = np.dtype([("early", np.int32, (2,)), ("prompt", np.int32, (2,)), ("late", np.int32, (2,)),
                              ("carr_phase", np.uint32), ("carr_step", np.uint32), ("code_phase", np.uint64),
                              ("code_step", np.uint64), ("e", np.int32), ("c", np.int32)])                     # gj_track_epoch
TrackParams = _ffi.TrackParams


def _track_params(params) -> "_ffi.TrackParams":
    """A ``TrackParams`` as it is; ``(spacing, aid_div, pll_p, pll_i, fll, dll_p, dll_i)`` made into one."""
    if isinstance(params, _ffi.TrackParams):
        return params
    v = [int(x) for x in params]
    if len(v) != 7 or any(not -2 ** 31 <= x < 2 ** 31 for x in v):
        raise GpsJamError(-5, "unsupported: params are (spacing, aid_div, pll_p, pll_i, fll, dll_p, dll_i) in int32")
    return _ffi.TrackParams(*v, 0)


def _track_states(states) -> np.ndarray:
    """The states of ``Device.track`` as TRACK_STATE_DTYPE records: such records as they are, or rows of thirteen integers
    in the struct's order (code_phase, code_step, carr_phase, carr_step, code_row, 0, carr_nco, start, e_prev, c_prev,
    primed, 0, 0)."""
    if isinstance(states, np.ndarray) and states.dtype == TRACK_STATE_DTYPE:
        return np.ascontiguousarray(states).reshape(-1).copy()
    rows = [tuple(int(v) for v in s) for s in states]
    lo = (0, 0, 0, 0, -2 ** 31, -2 ** 31, -2 ** 63, 0, -2 ** 31, -2 ** 31, -2 ** 31, -2 ** 31, -2 ** 31)
    hi = (2 ** 64, 2 ** 64, 2 ** 32, 2 ** 32, 2 ** 31, 2 ** 31, 2 ** 63, 2 ** 32, 2 ** 31, 2 ** 31, 2 ** 31, 2 ** 31, 2 ** 31)
    rec = np.zeros(len(rows), TRACK_STATE_DTYPE)
    for k, r in enumerate(rows):
        if len(r) != 13 or any(not a <= v < b for v, a, b in zip(r, lo, hi)):
            raise GpsJamError(-1, f"invalid argument: a state is thirteen integers in the order of gj_track_state, not {r}")
        rec[k] = (r[:6], r[6], r[7], r[8], r[9], r[10], r[11:13])
    return rec


SUB_TRACK_CHANNEL_DTYPE = np.dtype([("start", np.uint32), ("code_row", np.int32)])          # gj_subtract_track_channel


def _subtract_track_channels(channels, n_code_rows: int, n_epochs: int, block_samples: int, n_samples: int) -> np.ndarray:
    """The channel table of ``Device.subtract_tracked`` as SUB_TRACK_CHANNEL_DTYPE records, checked on the host: it lives
    in device memory once uploaded, where gj_subtract_track_dev cannot answer for it with a status."""
    if isinstance(channels, np.ndarray) and channels.dtype == SUB_TRACK_CHANNEL_DTYPE:
        rec = np.ascontiguousarray(channels).reshape(-1)
    else:
        rows = [tuple(int(v) for v in c) for c in channels]
        for r in rows:
            if len(r) != 2 or not (0 <= r[0] < 2 ** 32 and -2 ** 31 <= r[1] < 2 ** 31):
                raise GpsJamError(-1, f"invalid argument: a channel is (start, code_row), not {r}")
        rec = np.array(rows, SUB_TRACK_CHANNEL_DTYPE).reshape(-1)
    for k, c in enumerate(rec):
        if not 0 <= int(c["code_row"]) < n_code_rows:
            raise GpsJamError(-1, f"invalid argument: channel {k}: code_row {int(c['code_row'])} outside the {n_code_rows} rows")
        if int(c["start"]) + n_epochs * block_samples > n_samples:
            raise GpsJamError(-1, f"invalid argument: channel {k}: {n_epochs} epochs of {block_samples} samples from start "
                                  f"{int(c['start'])} run past the range's {n_samples}")
    return rec


ACQ_MAX_PEAKS = _ffi.GJ_ACQ_MAX_PEAKS
ACQ_PEAK_DTYPE = np.dtype([("power", np.float64), ("code_index", np.int32), ("freq_index", np.int32)])        # gj_acq_peak
ACQ_FLOOR_DTYPE = np.dtype([("mean_power", np.float64), ("kept_columns", np.int32), ("reserved", np.int32)])  # gj_acq_floor


def _corr_channels(channels, n_code_rows: int) -> np.ndarray:
    """The channel table of ``Device.corr_bank`` as CORR_CHANNEL_DTYPE records, its fields checked on the host: they
    live in device memory once uploaded, where gj_corr_bank_dev cannot answer for them with a status."""
    if isinstance(channels, np.ndarray) and channels.dtype == CORR_CHANNEL_DTYPE:
        rec = np.ascontiguousarray(channels).reshape(-1)
    else:
        rows = [tuple(int(v) for v in c) for c in channels]
        for r in rows:
            if len(r) != 6 or not (0 <= r[0] < 2 ** 64 and 0 <= r[1] < 2 ** 64 and 0 <= r[2] < 2 ** 32 and 0 <= r[3] < 2 ** 32
                                   and -2 ** 31 <= r[4] < 2 ** 31 and -2 ** 31 <= r[5] < 2 ** 31):
                raise GpsJamError(-1, f"invalid argument: a channel is (code_phase, code_step, carr_phase, carr_step, code_row, 0), not {r}")
        rec = np.array(rows, CORR_CHANNEL_DTYPE).reshape(-1)
    for k, c in enumerate(rec):
        what = None
        if int(c["reserved"]) != 0:
            what = "reserved must be 0"
        elif not 0 <= int(c["code_row"]) < n_code_rows:
            what = f"code_row {int(c['code_row'])} outside the {n_code_rows} rows"
        elif int(c["code_phase"]) >= _ffi.GJ_CORR_CODE_LEN << 32:
            what = "code_phase is not below 1023 * 2^32"
        elif int(c["code_step"]) >= _ffi.GJ_CORR_MAX_CODE_STEP:
            what = "code_step is not below 2^34"
        if what:
            raise GpsJamError(-1, f"invalid argument: channel {k}: {what}")
    return rec


class _FrameRecords:
    """What ``Ridge`` and ``ChirpScan`` share: the records, the frames' geometry, slicing by frame and the ridge's four
    numbers.  A subclass names its dtype and the word of its slicing errors (``_as``) and builds a slice (``_sliced``)."""

    def __init__(self, records, nfft: int, hop: int, first_sample: int = 0, guard: int = 2):
        self.records = np.ascontiguousarray(records, dtype=self._dtype).reshape(-1)
        self.nfft, self.hop, self.first_sample, self.guard = int(nfft), int(hop), int(first_sample), int(guard)

    def __len__(self) -> int:
        return self.records.size

    def __getitem__(self, key):
        if not isinstance(key, slice):
            raise TypeError(f"a {type(self).__name__} is sliced by frame: {self._as}[a:b]")
        start, _, step = key.indices(len(self))
        if step != 1:
            raise ValueError(f"a {type(self).__name__} keeps consecutive frames: the step must be 1")
        return self._sliced(key, self.first_sample + start * self.hop)

    total = property(lambda self: self.records["total"])
    peak = property(lambda self: self.records["peak"])
    second = property(lambda self: self.records["second"])
    peak_bin = property(lambda self: self.records["peak_bin"])

    @property
    def concentration(self) -> np.ndarray:
        """peak / total: the share of each frame's power in its peak bin (0 for an empty frame); for a ChirpScan at the
        best rate, in its de-chirped peak bin."""
        t = self.total.astype(np.float64)
        return np.divide(self.peak, t, out=np.zeros(t.shape), where=t > 0)


class Ridge(_FrameRecords):
    """The short-time spectral ridge of a capture (``Device.ridge``; gj_ridge_frame, include/gpsjam.h): per frame the
    total power, the peak |X[k]|^2, the largest value outside the guard band around the peak and the peak's bin, as
    the numpy structured array ``records`` (RIDGE_DTYPE) plus the geometry they were computed with.  Frame f starts
    at sample ``first_sample + f * hop``.  ``ridge[a:b]`` is the Ridge of those frames."""
    _dtype, _as = RIDGE_DTYPE, "ridge"

    def _sliced(self, key, first_sample) -> "Ridge":
        return Ridge(self.records[key], self.nfft, self.hop, first_sample, self.guard)

    def freq_hz(self, fs: float = 2.048e6) -> np.ndarray:
        """Signed frequency of peak_bin: bins from nfft/2 on are negative frequencies."""
        return _bands.signed_bins(self.nfft, self.peak_bin.astype(np.int64)) * (float(fs) / self.nfft)


CHIRP_DTYPE = np.dtype([("total", np.float32), ("peak", np.float32), ("second", np.float32), ("peak_bin", np.int32),
                        ("rate_index", np.int32), ("reserved", np.int32)])


class ChirpScan(_FrameRecords):
    """The chirp-rate search of a capture (``Device.chirp``; gj_chirp_frame, include/gpsjam.h): per frame the ridge's four
    numbers behind the de-chirp that concentrates the frame best, and which rate that was, as the numpy structured array
    ``records`` (CHIRP_DTYPE) plus the geometry and the rate grid ``rates = (first, step, n)`` they were computed with.
    Rates count bins per frame length: one unit is fs^2 / nfft^2 Hz/s.  ``peaks``: the peak of every frame at every
    rate, ``[frames, n]``, or None.  Frame f starts at sample ``first_sample + f * hop``; ``scan[a:b]`` is the
    ChirpScan of those frames."""
    _dtype, _as = CHIRP_DTYPE, "scan"

    def __init__(self, records, nfft: int, hop: int, rates, first_sample: int = 0, guard: int = 2, peaks=None):
        super().__init__(records, nfft, hop, first_sample, guard)
        self.rates = tuple(int(v) for v in rates)
        if len(self.rates) != 3:
            raise ValueError("rates is (first, step, n)")
        self.peaks = None if peaks is None else np.ascontiguousarray(peaks, dtype=np.float32).reshape(self.records.size, self.rates[2])

    def _sliced(self, key, first_sample) -> "ChirpScan":
        return ChirpScan(self.records[key], self.nfft, self.hop, self.rates, first_sample, self.guard,
                         None if self.peaks is None else self.peaks[key])

    rate_index = property(lambda self: self.records["rate_index"])

    @property
    def rate(self) -> np.ndarray:
        """The q of each frame's rate_index, in bins per frame length."""
        return self.rates[0] + self.rates[1] * self.rate_index.astype(np.int64)

    def sweep_hz_per_s(self, fs: float = 2.048e6) -> np.ndarray:
        """Each frame's best rate in Hz/s: q fs^2 / nfft^2."""
        return self.rate * (float(fs) / self.nfft) ** 2

    def centre_freq_hz(self, fs: float = 2.048e6) -> np.ndarray:
        """Signed frequency of the de-chirped line at the CENTRE of each frame: bin + q / 2, wrapped to [-fs/2, fs/2)."""
        k = self.peak_bin.astype(np.float64) + 0.5 * self.rate
        return ((k + self.nfft / 2.0) % self.nfft - self.nfft / 2.0) * (float(fs) / self.nfft)


def _frames_to_compute(n_frames: Optional[int], nbytes: int, first_sample: int, nfft: int, hop: int):
    """(n_frames, empty): a given frame count as it is, None means all that fit (``ridge_frames``).  ``empty``: none does
    although the library takes nfft and hop, so the answer is the result without frames and nothing is launched."""
    if n_frames is not None:
        return n_frames, False
    n_frames = ridge_frames(nbytes, first_sample, nfft, hop)
    return n_frames, n_frames == 0 and 16 <= int(nfft) <= 4096 and hop >= 1


def _row_args_fit(nfft: int, frames_per_row: int, *sizes: int) -> bool:
    """Whether gj_sk_rows / gj_csd_rows can be asked at all: ``sizes`` go into size_t, the other two into int."""
    return min(int(v) for v in sizes) >= 0 and all(-2 ** 31 <= int(v) < 2 ** 31 for v in (nfft, frames_per_row))


def sk_rows(nbytes: int, first_sample: int, nfft: int, hop: int, frames_per_row: int) -> int:
    """Whole rows of frames_per_row frames of nfft points that fit from first_sample at the given hop (gj_sk_rows);
    0 when none do."""
    if not _row_args_fit(nfft, frames_per_row, nbytes, first_sample, hop):
        return 0
    return int(_ffi.load().gj_sk_rows(int(nbytes), int(first_sample), int(nfft), int(hop), int(frames_per_row)))


def _rows_to_compute(n_rows: Optional[int], fit, ranges, nfft: int, hop: int, frames_per_row: int):
    """(n_rows, empty): a given row count as it is, None means all that fit (``sk_rows`` / ``csd_rows`` on ``ranges``).
    ``empty``: the float32[0, nfft] to answer with when none does although the library takes the geometry, else None."""
    if n_rows is not None:
        return int(n_rows), None
    n_rows = fit(*ranges, nfft, hop, frames_per_row)
    legal = 16 <= nfft <= 4096 and hop >= 1 and 2 <= frames_per_row <= 65536
    return n_rows, np.empty((0, nfft), np.float32) if n_rows == 0 and legal else None


class _RowSums:
    """What ``SpectralKurtosis`` and ``CrossSpectrum`` share: arrays [rows, nfft] in FFT order and the rows' geometry."""

    def __init__(self, lead, nfft: int, hop: int, frames_per_row: int):
        self.nfft, self.hop, self.frames_per_row = int(nfft), int(hop), int(frames_per_row)
        self._lead = self._rows(lead)

    def _rows(self, values, dtype=np.float32) -> np.ndarray:
        return np.ascontiguousarray(values, dtype=dtype).reshape(-1, self.nfft)

    def __len__(self) -> int:
        return self._lead.shape[0]

    def freq_hz(self, fs: float = 2.048e6) -> np.ndarray:
        """Signed frequency of every bin in FFT order: bins from nfft/2 on are negative frequencies."""
        return _bands.signed_bins(self.nfft) * (float(fs) / self.nfft)


def _sk_estimate(s1, s2, frames: int) -> np.ndarray:
    """(M+1)/(M-1) * (M * S2 / S1^2 - 1) in float64 with M = frames; NaN where S1 == 0 (include/gpsjam.h)."""
    s1, s2, m = np.asarray(s1, np.float64), np.asarray(s2, np.float64), float(frames)
    with np.errstate(divide="ignore", invalid="ignore"):
        sk = (m + 1.0) / (m - 1.0) * (m * s2 / (s1 * s1) - 1.0)
    return np.where(s1 == 0, np.nan, sk)


class SpectralKurtosis(_RowSums):
    """Spectral kurtosis of a capture (``Device.spectral_kurtosis``; gj_sk_dev, include/gpsjam.h): per row of
    ``frames_per_row`` frames and per bin the sums ``s1`` of P and ``s2`` of P^2 and the estimator ``sk``, each
    float32[rows, nfft] in FFT order, plus the geometry they were computed with.  Row r starts at sample
    ``first_sample + r * frames_per_row * hop``.  Noise gives sk = 1 with standard deviation 2 / sqrt(frames_per_row)."""

    def __init__(self, s1, s2, sk, nfft: int, hop: int, frames_per_row: int, first_sample: int = 0):
        super().__init__(s1, nfft, hop, frames_per_row)
        self.first_sample = int(first_sample)
        self.s1, self.s2, self.sk = self._lead, self._rows(s2), self._rows(sk)

    def merged(self) -> np.ndarray:
        """SK of all rows together, float64[nfft]: the estimator on the summed sums with M = frames_per_row * rows."""
        if len(self) == 0:
            return np.full(self.nfft, np.nan)
        return _sk_estimate(self.s1.astype(np.float64).sum(axis=0), self.s2.astype(np.float64).sum(axis=0), self.frames_per_row * len(self))


def csd_rows(nbytes_a: int, first_a: int, nbytes_b: int, first_b: int, nfft: int, hop: int, frames_per_row: int) -> int:
    """Whole rows of frames_per_row frame pairs of nfft points that fit BOTH captures from first_a / first_b at the given
    hop (gj_csd_rows); 0 when none do."""
    if not _row_args_fit(nfft, frames_per_row, nbytes_a, first_a, nbytes_b, first_b, hop):
        return 0
    return int(_ffi.load().gj_csd_rows(int(nbytes_a), int(first_a), int(nbytes_b), int(first_b), int(nfft), int(hop),
                                       int(frames_per_row)))


def _msc(saa, sbb, sab) -> np.ndarray:
    """|Sab|^2 / (Saa Sbb) in float64; NaN where Saa Sbb == 0 (include/gpsjam.h)."""
    saa, sbb, sab = np.asarray(saa, np.float64), np.asarray(sbb, np.float64), np.asarray(sab, np.complex128)
    den = saa * sbb
    with np.errstate(divide="ignore", invalid="ignore"):
        v = (sab.real * sab.real + sab.imag * sab.imag) / den
    return np.where(den == 0, np.nan, v)


class CrossSpectrum(_RowSums):
    """Cross-spectral density of a capture pair (``Device.cross_spectrum``; gj_csd_dev, include/gpsjam.h): per row of
    ``frames_per_row`` frame pairs and per bin the auto-spectra ``saa`` and ``sbb`` (float32), the cross-spectrum ``sab``
    (complex64, sum of B conj(A): its phase falls with frequency when b is delayed) and the magnitude-squared coherence
    ``msc`` (float32), each [rows, nfft] in FFT order, plus the geometry they were computed with.  Row r starts at
    samples ``first_a + r * frames_per_row * hop`` of a and ``first_b + ...`` of b."""

    def __init__(self, saa, sbb, sab, msc, nfft: int, hop: int, frames_per_row: int, first_a: int = 0, first_b: int = 0):
        super().__init__(saa, nfft, hop, frames_per_row)
        self.first_a, self.first_b = int(first_a), int(first_b)
        self.saa, self.sbb, self.sab, self.msc = self._lead, self._rows(sbb), self._rows(sab, np.complex64), self._rows(msc)

    def merged(self) -> np.ndarray:
        """MSC of all rows together, float64[nfft]: the formula on the summed sums (M = frames_per_row * rows)."""
        if len(self) == 0:
            return np.full(self.nfft, np.nan)
        return _msc(self.saa.astype(np.float64).sum(axis=0), self.sbb.astype(np.float64).sum(axis=0),
                    self.sab.astype(np.complex128).sum(axis=0))


def as_u8(raw) -> np.ndarray:
    """Contiguous uint8 view of bytes / bytearray / memoryview / ndarray."""
    if isinstance(raw, np.ndarray):
        if raw.dtype != np.uint8:
            raise TypeError("raw I/Q must be uint8")
        return np.ascontiguousarray(raw).reshape(-1)
    return np.frombuffer(raw, dtype=np.uint8)


def _ptr(x) -> int:
    """Device address of a torch tensor / DevBuf / int."""
    if x is None:
        return 0
    if isinstance(x, int):
        return x
    if isinstance(x, (DevBuf, Capture)):
        return x.ptr
    if hasattr(x, "data_ptr"):
        return int(x.data_ptr())
    raise TypeError(f"not a device buffer: {type(x)!r}")


class DevBuf:
    """Device allocation owned by a Device (for callers without torch)."""

    def __init__(self, dev: "Device", nbytes: int):
        self.dev, self.nbytes = dev, int(nbytes)
        p = C.c_void_p()
        dev._check(dev._lib.gj_malloc(dev._ctx, self.nbytes, C.byref(p)))
        self.ptr = p.value or 0

    def upload(self, host: np.ndarray, offset: int = 0):
        host = np.ascontiguousarray(host)
        if offset + host.nbytes > self.nbytes:
            raise ValueError("upload exceeds the device buffer")
        self.dev._check(self.dev._lib.gj_memcpy_h2d(self.dev._ctx, self.ptr + offset,
                                                    host.ctypes.data, host.nbytes))
        return self

    def download(self, dtype=np.uint8, count: Optional[int] = None, offset: int = 0) -> np.ndarray:
        dt = np.dtype(dtype)
        if count is None:
            count = (self.nbytes - offset) // dt.itemsize
        out = np.empty(count, dt)
        self.dev._check(self.dev._lib.gj_memcpy_d2h(self.dev._ctx, out.ctypes.data,
                                                    self.ptr + offset, out.nbytes))
        return out

    def free(self):
        if self.ptr:
            self.dev._lib.gj_free(self.dev._ctx, self.ptr)
            self.ptr = 0

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.free()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Capture:
    """One capture resident in HBM: uploaded ONCE (file -> pinned bounce buffers -> HBM, or from
    a uint8 array), then handed to ``Device.chunk_power / welch / amp_stats / onset /
    byte_histogram / xcorr_lags_at`` any number of times.  The array-taking forms of those calls
    stage their input on every call (21 ms per GiB of PCIe against 0.2-1.3 ms of kernel time), so
    a caller that runs scan + PSD + RSSI on one file (widmo_plot, the worker's scan ->
    triangulation flow) uses this instead.  The library's ``*_u8`` entry points take the device
    address as it is, so a call on a Capture works in a lane of its own like any other: several
    host threads may use one Capture (and one Device) at once.  ``uploads`` counts host->device
    passes (tests)."""

    uploads = 0
    _count_lock = __import__("threading").Lock()

    @classmethod
    def _count(cls):
        with cls._count_lock:                                # several host threads may upload at once (one lane each)
            cls.uploads += 1

    @classmethod
    def _adopt(cls, dev: "Device", ptr: int, nbytes: int, path=None) -> "Capture":
        """A Capture around a device pointer the library has just handed out (gj_ingest_*)."""
        self = cls.__new__(cls)
        self.dev, self.ptr, self.nbytes, self.path = dev, int(ptr or 0), int(nbytes), path
        self.results, self.ingest_ms, self.results_unpack = {}, None, None
        Capture._count()
        return self

    @classmethod
    def from_device(cls, dev: "Device", buf: "DevBuf", nbytes: Optional[int] = None) -> "Capture":
        """A Capture that takes over a device allocation a kernel has filled (``Device.excise``): no host->device pass,
        so ``uploads`` does not count it.  ``buf`` gives its memory up; the Capture frees it."""
        self = cls.__new__(cls)
        self.dev, self.ptr, self.path = dev, int(buf.ptr), None
        self.nbytes = int(buf.nbytes if nbytes is None else nbytes)
        self.results, self.ingest_ms, self.results_unpack = {}, None, None
        buf.ptr = 0
        return self

    def __init__(self, dev: "Device", source, offset: int = 0, max_bytes: int = 0):
        import os
        self.dev = dev
        # results computed while the capture was uploaded (Device.ingest), keyed by the call that would recompute
        # them: ("chunk_power", chunk_bytes, eps, odd_chunk_zero), ("amp_stats", threshold), ("onset", noise_samples,
        # window, factor), ("welch", chunk_samples, nperseg, fs, shift)
        self.results, self.ingest_ms, self.results_unpack = {}, None, None
        p, n = C.c_void_p(), C.c_size_t(0)
        if isinstance(source, (str, bytes, os.PathLike)):
            self.path = os.fspath(source)
            dev._check(dev._lib.gj_upload_file(dev._ctx, os.fsencode(self.path), int(offset), int(max_bytes),
                                               C.byref(p), C.byref(n)))
            self.nbytes = n.value
        else:
            self.path = None
            raw = as_u8(source)
            if offset or max_bytes:
                raw = raw[offset:offset + max_bytes] if max_bytes else raw[offset:]
            dev._check(dev._lib.gj_upload(dev._ctx, raw.ctypes.data if raw.size else None, raw.size, C.byref(p)))
            self.nbytes = int(raw.size)
        self.ptr = p.value or 0
        Capture._count()

    @property
    def nsamples(self) -> int:
        return self.nbytes // 2

    def download(self, offset: int = 0, count: Optional[int] = None) -> np.ndarray:
        """Bytes [offset, offset + count) back on the host (tests, near-tie re-evaluation)."""
        if count is None:
            count = self.nbytes - offset
        count = max(0, min(count, self.nbytes - offset))
        out = np.empty(count, np.uint8)
        if count:
            self.dev._check(self.dev._lib.gj_memcpy_d2h(self.dev._ctx, out.ctypes.data, self.ptr + offset, count))
        return out

    def free(self):
        if getattr(self, "ptr", 0) and getattr(self.dev, "_ctx", None):
            self.dev._lib.gj_free(self.dev._ctx, self.ptr)
        self.ptr = 0

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.free()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Device:
    def __init__(self, index: int = 0):
        self._lib = _ffi.load()
        ctx = C.c_void_p()
        rc = self._lib.gj_create(int(index), C.byref(ctx))
        if rc != 0:
            raise GpsJamError(rc, f"gj_create({index}): " + self._lib.gj_strerror(rc).decode())
        self._ctx = ctx
        self.index = int(index)
        self.last_kernel_ms = 0.0
        self.cache_hits = 0        # calls answered from a Capture's ride-along results (no kernel ran)
        self.kernel_calls = {}     # name -> host-array / resident-capture calls that DID reach the library

    # ------------------------------------------------------------------ plumbing
    def _check(self, rc: int):
        if rc != 0:
            detail = self._lib.gj_last_error(self._ctx).decode(errors="replace")
            raise GpsJamError(rc, f"{self._lib.gj_strerror(rc).decode()}: {detail}")

    def capture(self, source, offset: int = 0, max_bytes: int = 0) -> Capture:
        """Upload a capture file (path) or a uint8 array once; see ``Capture``."""
        return Capture(self, source, offset, max_bytes)

    def ingest(self, source, *, chunk_bytes: int = 65536, eps: float = 1e-10, odd_chunk_zero: bool = False,
               rssi_threshold: float = 0.0, noise_samples: int = 200000, window: int = 1000, factor: float = 50.0,
               welch=None, fs: float = 2.048e6, shift: bool = True, want_db: bool = False, offset: int = 0,
               max_bytes: int = 0) -> Capture:
        """Upload a capture file (path) or uint8 array AND analyse it while it uploads (gj_ingest_*: the kernels run
        on the pieces that have landed: 1-16 MiB each, by capture size).  ``chunk_bytes`` != 0: the fused scan (K1 power map, K3 amplitude
        statistics at ``rssi_threshold``, K4 onset); ``welch=(chunk_samples, nperseg)``: the PSD waterfall.  The
        results ride on the returned Capture (``.results``) and are handed out by ``chunk_power`` / ``amp_stats`` /
        ``onset`` / ``welch`` when these are called on it with the same parameters -- bit-identical to what those
        calls compute on an uploaded capture, without a second pass."""
        import os
        kw = dict(chunk_bytes=chunk_bytes, eps=eps, odd_chunk_zero=odd_chunk_zero, rssi_threshold=rssi_threshold,
                  noise_samples=noise_samples, window=window, factor=factor, welch=welch, fs=fs, shift=shift, want_db=want_db)
        plan = self._ingest_plan(**kw)
        is_path = isinstance(source, (str, bytes, os.PathLike))
        if is_path:
            path = os.fspath(source)
            size = os.stat(path).st_size                     # FileNotFoundError like open()
            nbytes = max(0, size - int(offset))
            if max_bytes:
                nbytes = min(nbytes, int(max_bytes))
        else:
            path = None
            raw = as_u8(source)
            if offset or max_bytes:
                raw = raw[offset:offset + max_bytes] if max_bytes else raw[offset:]
            nbytes = int(raw.size)
        power, psd, db = self._ingest_buffers(nbytes, chunk_bytes, welch, want_db)
        res, p = _ffi.IngestResult(), C.c_void_p()
        args = (C.byref(plan), power.ctypes.data, power.size, psd.ctypes.data, db.ctypes.data if db is not None else None,
                psd.size, C.byref(res), C.byref(p))
        if is_path:
            self._check(self._lib.gj_ingest_file(self._ctx, os.fsencode(path), int(offset), int(max_bytes), *args))
        else:
            self._check(self._lib.gj_ingest_u8(self._ctx, raw.ctypes.data if raw.size else None, raw.size, *args))
        return self._ingest_adopt(p.value, res, path, power, psd, db, **kw)

    def ingest_many(self, paths, *, chunk_bytes: int = 65536, eps: float = 1e-10, odd_chunk_zero: bool = False,
                    rssi_threshold: float = 0.0, noise_samples: int = 200000, window: int = 1000, factor: float = 50.0,
                    welch=None, fs: float = 2.048e6, shift: bool = True, want_db: bool = False):
        """``ingest`` for several capture FILES at once (gj_ingest_files: one host thread of the library and one lane per
        file, the copies sharing the cores) -- the recordings of a deployment.  Returns the Captures in the order of
        ``paths``, each with the same ride-along results ``ingest`` would have left on it.  A file that cannot be read
        raises (FileNotFoundError from the stat here, GpsJamError from the library); captures that did come in are freed."""
        import os
        paths = [os.fspath(p) for p in paths]
        kw = dict(chunk_bytes=chunk_bytes, eps=eps, odd_chunk_zero=odd_chunk_zero, rssi_threshold=rssi_threshold,
                  noise_samples=noise_samples, window=window, factor=factor, welch=welch, fs=fs, shift=shift, want_db=want_db)
        if not paths:
            return []
        plan = self._ingest_plan(**kw)
        jobs = (_ffi.IngestJob * len(paths))()
        bufs = []
        for k, path in enumerate(paths):
            nbytes = os.stat(path).st_size                   # FileNotFoundError like open()
            power, psd, db = self._ingest_buffers(nbytes, chunk_bytes, welch, want_db)
            bufs.append((power, psd, db))
            j = jobs[k]
            j.path, j.offset, j.max_bytes = os.fsencode(path), 0, 0
            j.power, j.power_cap = power.ctypes.data, power.size
            j.psd, j.psd_db, j.psd_cap_floats = psd.ctypes.data, (db.ctypes.data if db is not None else None), psd.size
        rc = self._lib.gj_ingest_files(self._ctx, jobs, len(paths), C.byref(plan))
        if rc:
            for j in jobs:
                if j.status == 0 and j.dptr:
                    self._lib.gj_free(self._ctx, j.dptr)
            self._check(rc)
        return [self._ingest_adopt(jobs[k].dptr, jobs[k].result, paths[k], *bufs[k], **kw) for k in range(len(paths))]

    @staticmethod
    def _ingest_plan(*, chunk_bytes, eps, odd_chunk_zero, rssi_threshold, noise_samples, window, factor, welch, fs, shift, want_db):
        return _ffi.IngestPlan(int(chunk_bytes), float(eps), _ffi.GJ_CP_ODD_CHUNK_ZERO if odd_chunk_zero else 0,
                               float(rssi_threshold), int(noise_samples), int(window), float(factor),
                               int(welch[0]) if welch else 0, int(welch[1]) if welch else 0,
                               _ffi.GJ_WELCH_SHIFT if shift else 0, float(fs))

    def _ingest_buffers(self, nbytes, chunk_bytes, welch, want_db):
        n_chunks = self._lib.gj_chunk_count(nbytes, chunk_bytes) if chunk_bytes else 0
        rows = self._lib.gj_welch_rows(nbytes, welch[0], welch[1]) if welch else 0
        nper = int(welch[1]) if welch else 0
        power = np.empty(n_chunks, np.float32)
        psd = np.empty((rows, nper), np.float32)
        db = np.empty((rows, nper), np.float32) if (welch and want_db) else None
        return power, psd, db

    def _ingest_adopt(self, ptr, res, path, power, psd, db, *, chunk_bytes, eps, odd_chunk_zero, rssi_threshold, noise_samples,
                      window, factor, welch, fs, shift, want_db):
        cap = Capture._adopt(self, ptr, res.nbytes, path)
        cap.ingest_ms = (float(res.upload_ms), float(res.total_ms))
        cap.results_unpack = self.get_unpack()               # the convention the ride-along results were computed under
        for a in (power, psd, db):
            if a is not None:
                a.flags.writeable = False                    # handed out as they are on every matching call
        if chunk_bytes and power.size:
            cap.results[("chunk_power", int(chunk_bytes), float(np.float32(eps)), bool(odd_chunk_zero))] = power
            cap.results[("amp_stats", float(np.float32(rssi_threshold)))] = AmpStats.from_buffer_copy(bytes(res.amp))
            cap.results[("onset", int(noise_samples), int(window), float(np.float32(factor)))] = Onset.from_buffer_copy(bytes(res.onset))
        if welch and psd.shape[0]:
            cap.results[("welch", int(welch[0]), int(welch[1]), float(fs), bool(shift))] = (psd, db)
        return cap

    def _cached(self, raw, key):
        """Ride-along result of ``Device.ingest`` for this call, or None.  The results were computed under the unpack
        convention in force at ingest time: after a ``set_unpack`` to anything else they are dropped (gj_set_unpack
        promises to affect every later call on the context), and the call recomputes.  A hit ran no kernel:
        ``last_kernel_ms`` says so."""
        if not isinstance(raw, Capture) or not raw.results:
            return None
        if raw.results_unpack is not None and raw.results_unpack != self.get_unpack():
            if raw.dev is self:                              # this context's convention has changed: they are stale for good
                raw.results.clear()
            return None                                      # (another context with another convention: just not served)
        hit = raw.results.get(key)
        if hit is not None:
            self.last_kernel_ms = 0.0
            self.cache_hits += 1
        return hit

    def _count(self, name):
        self.kernel_calls[name] = self.kernel_calls.get(name, 0) + 1

    @staticmethod
    def _input(raw):
        """(address, nbytes, keep-alive) of a call's input: a resident Capture goes in by its device
        address (the library uses it in place), anything else as a host uint8 buffer (staged)."""
        if isinstance(raw, Capture):
            if not raw.ptr and raw.nbytes:
                raise ValueError("the capture has been freed")
            return raw.ptr, raw.nbytes, raw
        arr = as_u8(raw)
        return (arr.ctypes.data if arr.size else None), int(arr.size), arr

    @contextlib.contextmanager
    def _resident(self, raw):
        """A live ``Capture`` for the length of a ``with``: ``raw`` itself when it is one (it is left alone on the way out),
        else host bytes, uploaded once and freed on the way out."""
        if isinstance(raw, Capture):
            if not raw.ptr and raw.nbytes:
                raise ValueError("the capture has been freed")
            yield raw
        else:
            with Capture(self, raw) as cap:
                yield cap

    def _residents(self, temps, *raws):
        """``_resident`` of every input in order, entered into the ExitStack ``temps``: the list of their ``Capture``s.  An
        input that IS an earlier one (the same object) gets that one's, so host bytes given twice are uploaded once."""
        caps = []
        for k, raw in enumerate(raws):
            earlier = next((caps[j] for j in range(k) if raws[j] is raw), None)
            caps.append(temps.enter_context(self._resident(raw)) if earlier is None else earlier)
        return caps

    def _on_device(self, temps, values, dtype, count: int, name: str, expected: str):
        """``values`` on the device: a device buffer (DevBuf, address, torch tensor) as it is, whatever it holds, or a host
        array of exactly ``count`` values, uploaded as ``dtype`` into a buffer that the ExitStack ``temps`` frees."""
        if isinstance(values, (DevBuf, int)) or hasattr(values, "data_ptr"):
            return values
        host, dtype = np.asarray(values).reshape(-1), np.dtype(dtype)
        if host.size != count:
            raise ValueError(f"{name} holds {host.size} values, {expected}")
        if host.size and dtype.kind == "i" and not np.issubdtype(host.dtype, np.integer):
            raise TypeError(f"{name} must be integers")
        return temps.enter_context(DevBuf(self, max(count, 1) * dtype.itemsize)).upload(host.astype(dtype))

    def _cleaned(self, n_samples: int, n_records: int, dtype, launch):
        """The tail the cleaners share: 2 * n_samples output bytes and n_records records of ``dtype`` (neither buffer is
        ever empty), ``launch(d_out, d_rec)``, the records brought back and the output handed over to a ``Capture`` of
        its own, which empties ``d_out``: ``(cleaned, records)``.  Whatever fails, both buffers are freed."""
        with DevBuf(self, max(2 * n_samples, 1)) as d_out, DevBuf(self, max(n_records, 1) * dtype.itemsize) as d_rec:
            launch(d_out, d_rec)
            rec = d_rec.download(dtype, n_records)
            return Capture.from_device(self, d_out, 2 * n_samples), rec

    def _replica_inputs(self, temps, capture, channels, codes, first_sample: int, n_samples, block_samples: int):
        """What ``corr_bank`` and ``subtract`` do before they part: the capture resident, ``n_samples`` defaulted to the
        rest of it, the code rows on the device (``(buffer, rows)`` as it is, a host int16[rows][1023] uploaded into a buffer
        that the ExitStack ``temps`` frees), the channels checked on the host as CORR_CHANNEL_DTYPE records, and the count of
        their blocks: ``(cap, n_samples, d_codes, n_rows, rec, blocks)``.  The records are NOT uploaded here: the
        subtraction puts its amplitudes on the device first, whose size it learns from these."""
        cap = temps.enter_context(self._resident(capture))
        n_samples = max(0, cap.nsamples - first_sample) if n_samples is None else int(n_samples)
        if isinstance(codes, tuple):
            d_codes, n_rows = codes[0], int(codes[1])
        else:
            host = np.ascontiguousarray(codes, np.int16)
            if host.ndim != 2 or host.shape[1] != _ffi.GJ_CORR_CODE_LEN:
                raise ValueError(f"codes must be int16[rows][{_ffi.GJ_CORR_CODE_LEN}]")
            n_rows = int(host.shape[0])
            d_codes = temps.enter_context(DevBuf(self, max(host.nbytes, 2))).upload(host)
        rec = _corr_channels(channels, n_rows)
        return cap, n_samples, d_codes, n_rows, rec, corr_blocks(n_samples, block_samples)

    def probe_busy_dev(self, milliseconds: float):
        """Keep this context's stream (and its hardware queue) busy for a while with one spinning wave (gj_probe_busy_dev):
        the stream-overlap probe of gpsjam/streams.py."""
        self._check(self._lib.gj_probe_busy_dev(self._ctx, float(milliseconds)))

    def debug_inject(self, what: int, count: int = 1):
        """Fault injection for tests (gj_debug_inject; GJ_INJECT_OWNER_ALIVE = 1; GJ_INJECT_FILL_WORKSPACE = 2 with the
        fill byte as ``count``)."""
        self._check(self._lib.gj_debug_inject(self._ctx, int(what), int(count)))

    def debug_counters(self):
        """Lanes made / in use / taken back from dead callers, dead-owner recoveries of the mutex."""
        v = [C.c_int(0) for _ in range(4)]
        self._check(self._lib.gj_debug_counters(self._ctx, *[C.byref(x) for x in v]))
        return dict(zip(("lanes", "lanes_busy", "lanes_reclaimed", "owner_deaths"), (x.value for x in v)))

    def close(self):
        if getattr(self, "_ctx", None):
            self._lib.gj_destroy(self._ctx)
            self._ctx = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self):
        name = C.create_string_buffer(256)
        cus, mem = C.c_int(0), C.c_uint64(0)
        self._check(self._lib.gj_device_info(self._ctx, name, 256, C.byref(cus), C.byref(mem)))
        return {"name": name.value.decode(), "compute_units": cus.value, "hbm_bytes": mem.value}

    def identity(self) -> str:
        """Which physical GPU this context runs on: ``pci=<bus id> uuid=<hex> hip=<index>`` (gj_device_identity)."""
        buf = C.create_string_buffer(160)
        self._check(self._lib.gj_device_identity(self._ctx, buf, 160))
        return buf.value.decode()

    def set_stream(self, stream_handle: Optional[int], external: bool = True):
        """Run on an external HIP stream (``torch.cuda.current_stream().cuda_stream``; 0 is
        the legacy default stream).  ``external=False`` returns to the context's own stream."""
        self._check(self._lib.gj_set_stream(self._ctx, stream_handle or None, 1 if external else 0))

    def synchronize(self):
        self._check(self._lib.gj_synchronize(self._ctx))

    def set_unpack(self, offset: float = 127.5, scale: float = 1.0 / 127.5):
        """sample = (u8 - offset) * scale for every later call on this context (gj_set_unpack):
        (127.5, 1/127.5) is the Python reference's convention, (128, 1/128) gnssdec's."""
        self._check(self._lib.gj_set_unpack(self._ctx, float(offset), float(scale)))

    def set_fill_threads(self, n: int = 0):
        """Host threads per staged copy (gj_set_fill_threads): 0 = by capture size, 1..16 = that many."""
        self._check(self._lib.gj_set_fill_threads(self._ctx, int(n)))

    def get_unpack(self):
        o, s = C.c_double(0), C.c_double(0)
        self._check(self._lib.gj_get_unpack(self._ctx, C.byref(o), C.byref(s)))
        return o.value, s.value

    def reserve(self, nbytes: int):
        self._check(self._lib.gj_reserve(self._ctx, int(nbytes)))

    def alloc(self, nbytes: int) -> DevBuf:
        return DevBuf(self, nbytes)

    def timer_start(self):
        self._check(self._lib.gj_timer_start(self._ctx))

    def timer_stop(self) -> float:
        ms = C.c_float(0)
        self._check(self._lib.gj_timer_stop(self._ctx, C.byref(ms)))
        return ms.value

    # ------------------------------------------------------------------ host arrays
    def chunk_power(self, raw, chunk_bytes: int = 65536, eps: float = 1e-10,
                    odd_chunk_zero: bool = False) -> np.ndarray:
        hit = self._cached(raw, ("chunk_power", int(chunk_bytes), float(np.float32(eps)), bool(odd_chunk_zero)))
        if hit is not None:
            return hit                                       # read-only array computed while the capture uploaded
        self._count("chunk_power")
        ptr, nbytes, _keep = self._input(raw)
        n = self._lib.gj_chunk_count(nbytes, chunk_bytes)
        out = np.empty(n, np.float32)
        n_out, ms = C.c_size_t(0), C.c_float(0)
        self._check(self._lib.gj_chunk_power_u8(
            self._ctx, ptr, nbytes, chunk_bytes, eps,
            _ffi.GJ_CP_ODD_CHUNK_ZERO if odd_chunk_zero else 0, out.ctypes.data, out.size,
            C.byref(n_out), C.byref(ms)))
        self.last_kernel_ms = ms.value
        return out[:n_out.value]

    def welch(self, raw, chunk_samples: int = 2048000, nperseg: int = 1024, fs: float = 2.048e6,
              shift: bool = True, want_db: bool = True):
        """(psd[rows, nperseg], psd_db[rows, nperseg] | None), float32."""
        key = ("welch", int(chunk_samples), int(nperseg), float(fs), bool(shift))
        if isinstance(raw, Capture) and raw.results.get(key) is not None and (raw.results[key][1] is not None or not want_db):
            hit = self._cached(raw, key)
            if hit is not None:
                return hit[0], (hit[1] if want_db else None)   # read-only arrays computed while the capture uploaded
        self._count("welch")
        ptr, nbytes, _keep = self._input(raw)
        rows = self._lib.gj_welch_rows(nbytes, chunk_samples, nperseg)
        psd = np.empty((rows, nperseg), np.float32)
        db = np.empty((rows, nperseg), np.float32) if want_db else None
        rows_out, ms = C.c_size_t(0), C.c_float(0)
        self._check(self._lib.gj_welch_u8(
            self._ctx, ptr, nbytes, chunk_samples, nperseg, fs,
            _ffi.GJ_WELCH_SHIFT if shift else 0, psd.ctypes.data,
            db.ctypes.data if want_db else None, psd.size, C.byref(rows_out), C.byref(ms)))
        self.last_kernel_ms = ms.value
        return psd, db

    def amp_stats(self, raw, threshold: float) -> AmpStats:
        hit = self._cached(raw, ("amp_stats", float(np.float32(threshold))))
        if hit is not None:
            return AmpStats.from_buffer_copy(bytes(hit))
        self._count("amp_stats")
        ptr, nbytes, _keep = self._input(raw)
        out, ms = AmpStats(), C.c_float(0)
        self._check(self._lib.gj_amp_stats_u8(self._ctx, ptr, nbytes, threshold,
                                              C.byref(out), C.byref(ms)))
        self.last_kernel_ms = ms.value
        return out

    def onset(self, raw, noise_samples: int = 200000, window: int = 1000,
              factor: float = 50.0) -> Onset:
        hit = self._cached(raw, ("onset", int(noise_samples), int(window), float(np.float32(factor))))
        if hit is not None:
            return Onset.from_buffer_copy(bytes(hit))
        self._count("onset")
        ptr, nbytes, _keep = self._input(raw)
        out, ms = Onset(), C.c_float(0)
        self._check(self._lib.gj_onset_u8(self._ctx, ptr, nbytes, noise_samples,
                                          window, factor, C.byref(out), C.byref(ms)))
        self.last_kernel_ms = ms.value
        return out

    def xcorr_lags_at(self, captures: Sequence["Capture"], starts: Sequence[int], n_samples: int,
                      pairs: Sequence[Sequence[int]], want_margins: bool = False):
        """Lags between resident captures: slice a = n_samples I/Q pairs of captures[a] from
        starts[a] (negative / out of range -> GJ_LAG_INVALID for its pairs).  No slice ever
        leaves HBM: the slices go to the library as device addresses inside the captures."""
        prs = [tuple(int(x) for x in p) for p in np.asarray(pairs, np.int64).reshape(-1, 2)]
        ok = [0 <= int(st) and 2 * (int(st) + n_samples) <= c.nbytes for c, st in zip(captures, starts)]
        lags = np.full(len(prs), GJ_LAG_INVALID, np.int32)
        peaks = np.zeros(len(prs), np.float32)
        margins = np.zeros(len(prs), np.float32)
        live = [k for k, (i, j) in enumerate(prs) if ok[i] and ok[j]]
        if live and n_samples > 0:
            used = sorted({a for k in live for a in prs[k]})
            local = {a: n for n, a in enumerate(used)}
            ptrs = (C.c_void_p * len(used))(*[captures[a].ptr + 2 * int(starts[a]) for a in used])
            flat = np.ascontiguousarray(np.array([[local[prs[k][0]], local[prs[k][1]]] for k in live], np.int32).reshape(-1))
            l2, p2, m2 = (np.empty(len(live), np.int32), np.empty(len(live), np.float32), np.empty(len(live), np.float32))
            ms = C.c_float(0)
            self._check(self._lib.gj_xcorr_lags_u8(
                self._ctx, ptrs, len(used), n_samples, flat.ctypes.data_as(C.POINTER(C.c_int32)), len(live),
                l2.ctypes.data_as(C.POINTER(C.c_int32)), p2.ctypes.data_as(C.POINTER(C.c_float)),
                m2.ctypes.data_as(C.POINTER(C.c_float)), C.byref(ms)))
            self.last_kernel_ms = ms.value
            lags[live], peaks[live], margins[live] = l2, p2, m2
        if want_margins:
            return lags, peaks, margins
        return lags, peaks

    def byte_histogram(self, cap: "Capture", chunk_samples: int = 2048000, nperseg: int = 1024,
                       stride: int = 100) -> np.ndarray:
        """256-bin histogram of raw_chunk[::stride] over the chunks the waterfall keeps
        (widmo_plot.py:35,85)."""
        with DevBuf(self, 8 * 256) as d:   # a buffer of this call's own: several threads may histogram at once
            self.byte_histogram_dev(cap, cap.nbytes, chunk_samples, nperseg, stride, d)
            return d.download(np.uint64, 256)

    def xcorr_lags(self, slices: Sequence, pairs: Sequence[Sequence[int]], want_margins: bool = False):
        """lags[p], peaks[p] (, margins[p]) for pairs (i, j): lag of slice j relative to slice i
        (= argmax|correlate(slice_j, slice_i, 'full')| - (N-1))."""
        arrs = [as_u8(s) for s in slices]
        n = arrs[0].size // 2
        if any(a.size != 2 * n for a in arrs):
            raise ValueError("slices must have equal length")
        ptrs = (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
        flat = np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(-1))
        npairs = flat.size // 2
        lags = np.empty(npairs, np.int32)
        peaks = np.empty(npairs, np.float32)
        margins = np.empty(npairs, np.float32)
        ms = C.c_float(0)
        self._check(self._lib.gj_xcorr_lags_u8(
            self._ctx, ptrs, len(arrs), n, flat.ctypes.data_as(C.POINTER(C.c_int32)), npairs,
            lags.ctypes.data_as(C.POINTER(C.c_int32)), peaks.ctypes.data_as(C.POINTER(C.c_float)),
            margins.ctypes.data_as(C.POINTER(C.c_float)), C.byref(ms)))
        self.last_kernel_ms = ms.value
        if want_margins:
            return lags, peaks, margins
        return lags, peaks

    def xcorr_caf(self, slices: Sequence, pairs: Sequence[Sequence[int]], max_offset_hz: Optional[float] = None,
                  bins: Optional[Sequence[int]] = None, fs: float = 2.048e6, want_ridge: bool = False):
        """Lag AND frequency offset of slice j relative to slice i, for receivers on separate oscillators
        (gj_xcorr_caf_u8): a list of ``CafPeak``, one per pair.  ``slices``: equal-length uint8 arrays or resident
        ``Capture``s.  The bins searched: ``bins = (bin_first, n_bins)``, or the symmetric range that covers
        ``max_offset_hz``; neither: bin 0 alone (= ``xcorr_lags``).  ``want_ridge``: also the best lag and its peak
        of every bin, two arrays [n_pairs][n_bins]."""
        ins = [self._input(s) for s in slices]
        n = ins[0][1] // 2
        if any(nb != 2 * n for _, nb, _ in ins):
            raise ValueError("slices must have equal, even length")
        if bins is not None and max_offset_hz is not None:
            raise ValueError("give max_offset_hz or bins, not both")
        if bins is not None:
            bin_first, n_bins = int(bins[0]), int(bins[1])
        elif max_offset_hz is not None:
            bin_first, n_bins = caf_bin_range(n, max_offset_hz, fs)
        else:
            bin_first, n_bins = 0, 1
        ptrs = (C.c_void_p * len(ins))(*[p for p, _, _ in ins])
        flat = np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(-1))
        npairs = flat.size // 2
        out = (_ffi.CafResult * max(npairs, 1))()
        cells = max(npairs * max(n_bins, 0), 1)
        ridge_lags = np.empty(cells, np.int32) if want_ridge else None
        ridge_peaks = np.empty(cells, np.float32) if want_ridge else None
        ms = C.c_float(0)
        self._count("xcorr_caf")
        self._check(self._lib.gj_xcorr_caf_u8(
            self._ctx, ptrs, len(ins), n, flat.ctypes.data_as(C.POINTER(C.c_int32)), npairs, bin_first, n_bins, out,
            ridge_lags.ctypes.data_as(C.POINTER(C.c_int32)) if want_ridge else None,
            ridge_peaks.ctypes.data_as(C.POINTER(C.c_float)) if want_ridge else None, C.byref(ms)))
        self.last_kernel_ms = ms.value
        hz = xcorr_bin_hz(n, fs)
        res = [CafPeak(int(r.lag), int(r.bin), r.bin * hz, float(r.peak), float(r.margin_lag), float(r.margin_bin))
               for r in out[:npairs]]
        if want_ridge:
            return res, ridge_lags.reshape(npairs, n_bins), ridge_peaks.reshape(npairs, n_bins)
        return res

    def ridge(self, raw, nfft: int = 256, hop: Optional[int] = None, first_sample: int = 0,
              n_frames: Optional[int] = None, guard: int = 2) -> Ridge:
        """Short-time spectral ridge (gj_ridge_dev): per frame of nfft points, hop samples apart (default nfft // 2),
        where the spectral peak is and how much of the frame's power it holds; n_frames defaults to all that fit.
        ``raw``: host bytes (uploaded once, like a ``Capture``) or a resident ``Capture``.  16 bytes per frame come back."""
        hop = int(nfft) // 2 if hop is None else int(hop)
        with self._resident(raw) as cap:
            n_frames, empty = _frames_to_compute(n_frames, cap.nbytes, first_sample, nfft, hop)
            if empty:
                return Ridge(np.empty(0, RIDGE_DTYPE), nfft, hop, first_sample, guard)
            self._count("ridge")
            with DevBuf(self, max(int(n_frames), 1) * RIDGE_DTYPE.itemsize) as out:
                self.ridge_dev(cap, cap.nbytes, first_sample, nfft, hop, n_frames, guard, out)
                rec = out.download(RIDGE_DTYPE, int(n_frames))
        return Ridge(rec, nfft, hop, first_sample, guard)

    def chirp(self, raw, nfft: int = 256, hop: Optional[int] = None, rates=(0, 1, 1), first_sample: int = 0,
              n_frames: Optional[int] = None, guard: int = 2, want_peaks: bool = False) -> ChirpScan:
        """Chirp-rate search (gj_chirp_dev): the ridge of every frame behind a de-chirp at each of the rates
        ``first + r * step``, r < n, of ``rates = (first, step, n)`` (bins per frame length, at most 256 per call); per
        frame the rate that concentrates it best and the ridge's numbers there.  ``raw``: host bytes (uploaded once) or a
        resident ``Capture``; n_frames defaults to all that fit.  ``want_peaks``: also every frame's peak at every rate."""
        nfft, first_sample, guard = int(nfft), int(first_sample), int(guard)
        hop = nfft // 2 if hop is None else int(hop)
        first, step, n = (int(v) for v in rates)
        with self._resident(raw) as cap:
            n_frames, empty = _frames_to_compute(n_frames, cap.nbytes, first_sample, nfft, hop)
            if empty and 1 <= n <= _ffi.GJ_CHIRP_MAX_RATES:
                return ChirpScan(np.empty(0, CHIRP_DTYPE), nfft, hop, (first, step, n), first_sample, guard,
                                 np.empty((0, n), np.float32) if want_peaks else None)
            n_frames = int(n_frames)
            self._count("chirp")
            with DevBuf(self, max(n_frames, 1) * CHIRP_DTYPE.itemsize) as out, \
                    (DevBuf(self, max(n_frames, 1) * max(n, 1) * 4) if want_peaks else contextlib.nullcontext()) as pk:
                self.chirp_dev(cap, cap.nbytes, first_sample, nfft, hop, n_frames, guard, first, step, n, out, pk)
                rec = out.download(CHIRP_DTYPE, n_frames)
                peaks = pk.download(np.float32, n_frames * n).reshape(n_frames, n) if want_peaks else None
        return ChirpScan(rec, nfft, hop, (first, step, n), first_sample, guard, peaks)

    def spectral_kurtosis(self, capture, nfft: int = 256, hop: Optional[int] = None, frames_per_row: int = 256,
                          first_sample: int = 0, n_rows: Optional[int] = None) -> SpectralKurtosis:
        """Spectral kurtosis (gj_sk_dev): per row of frames_per_row frames of nfft points, hop samples apart (default
        nfft: independent frames), the per-bin sums of P and P^2 and the estimator; n_rows defaults to all that fit.
        ``capture``: host bytes (uploaded once, like a ``Capture``) or a resident ``Capture``."""
        nfft, frames_per_row, first_sample = int(nfft), int(frames_per_row), int(first_sample)
        hop = nfft if hop is None else int(hop)
        with self._resident(capture) as cap:
            n_rows, empty = _rows_to_compute(n_rows, sk_rows, (cap.nbytes, first_sample), nfft, hop, frames_per_row)
            if empty is not None:
                return SpectralKurtosis(empty, empty, empty, nfft, hop, frames_per_row, first_sample)
            self._count("spectral_kurtosis")
            cells = max(n_rows, 1) * max(nfft, 1)
            with DevBuf(self, 3 * 4 * cells) as out:
                self.spectral_kurtosis_dev(cap, cap.nbytes, first_sample, nfft, hop, frames_per_row, n_rows, out.ptr,
                                           out.ptr + 4 * cells, out.ptr + 8 * cells)
                got = out.download(np.float32, 3 * cells).reshape(3, cells)[:, :n_rows * nfft]
        return SpectralKurtosis(got[0], got[1], got[2], nfft, hop, frames_per_row, first_sample)

    def cross_spectrum(self, a, b, nfft: int = 256, hop: Optional[int] = None, frames_per_row: int = 1024,
                       first_a: int = 0, first_b: int = 0, n_rows: Optional[int] = None) -> CrossSpectrum:
        """Cross-spectral density and coherence of a capture pair (gj_csd_dev): per row of frames_per_row frame pairs of
        nfft points, hop samples apart (default nfft: independent frames), the per-bin sums of |A|^2, |B|^2 and
        B conj(A) and the magnitude-squared coherence; n_rows defaults to all that fit both.  ``a`` and ``b``: host bytes
        (uploaded once each) or resident ``Capture``s.  ``last_kernel_ms`` is the time of the two launches."""
        nfft, frames_per_row, first_a, first_b = int(nfft), int(frames_per_row), int(first_a), int(first_b)
        hop = nfft if hop is None else int(hop)
        with contextlib.ExitStack() as temps:
            cap_a, cap_b = self._residents(temps, a, b)
            n_rows, empty = _rows_to_compute(n_rows, csd_rows, (cap_a.nbytes, first_a, cap_b.nbytes, first_b), nfft, hop, frames_per_row)
            if empty is not None:
                return CrossSpectrum(empty, empty, empty, empty, nfft, hop, frames_per_row, first_a, first_b)
            self._count("cross_spectrum")
            cells = max(n_rows, 1) * max(nfft, 1)
            out = temps.enter_context(DevBuf(self, 5 * 4 * cells))       # sab (8-byte aligned) in front, then saa, sbb, msc
            self.timer_start()
            self.cross_spectrum_dev(cap_a, cap_a.nbytes, first_a, cap_b, cap_b.nbytes, first_b, nfft, hop, frames_per_row,
                                    n_rows, out.ptr + 8 * cells, out.ptr + 12 * cells, out.ptr, out.ptr + 16 * cells)
            self.last_kernel_ms = self.timer_stop()
            got = out.download(np.float32, 5 * cells)
        n = n_rows * nfft
        sab = got[:2 * cells][:2 * n].view(np.complex64)
        saa, sbb, msc = (got[k * cells:k * cells + n] for k in (2, 3, 4))
        return CrossSpectrum(saa, sbb, sab, msc, nfft, hop, frames_per_row, first_a, first_b)

    def excise(self, raw, threshold, nfft: int = 1024, first_sample: int = 0, n_samples: Optional[int] = None):
        """Frequency-domain excision (gj_excise_dev): samples first_sample .. + n_samples of ``raw`` (default: to the
        end) with every bin of every nfft-point frame whose power exceeds ``threshold[k]`` taken out.  ``raw``: host
        bytes (uploaded once) or a resident ``Capture``; ``threshold``: nfft floats in FFT order, in the units of
        ``ridge`` (+inf: never, negative: always), or a device buffer that holds them.  Returns
        ``(cleaned, records)``: the cleaned range as a resident ``Capture`` of its own (the caller frees it) and one
        EXCISE_DTYPE record per frame."""
        nfft, first_sample = int(nfft), int(first_sample)
        with contextlib.ExitStack() as temps:
            cap = temps.enter_context(self._resident(raw))
            n_samples = max(0, cap.nsamples - first_sample) if n_samples is None else int(n_samples)
            frames = excise_frames(n_samples, nfft)
            thr = self._on_device(temps, threshold, np.float32, nfft, "threshold", f"nfft is {nfft}")
            self._count("excise")
            return self._cleaned(n_samples, frames, EXCISE_DTYPE, lambda d_out, d_rec: self.excise_dev(
                cap, cap.nbytes, first_sample, n_samples, nfft, thr, d_out, d_rec))

    def excise_chirp(self, raw, threshold, rates, nfft: int = 1024, first_sample: int = 0, n_samples: Optional[int] = None):
        """Chirp-domain excision (gj_excise_chirp_dev): ``excise`` with every frame de-chirped by its own rate in front
        of the mask and re-chirped behind it, so that a sweep which crosses many bins inside a frame is cut as the few
        bins of its de-chirped line.  ``rates``: one integer per frame (bins per frame length, the unit of ``chirp``; 0
        leaves the frame to the plain excisor), a host array whose length must be the frame count, or a device buffer
        of int32.  ``raw``, ``threshold`` and the result ``(cleaned, records)`` as ``excise``; the records are taken
        behind the de-chirp."""
        nfft, first_sample = int(nfft), int(first_sample)
        with contextlib.ExitStack() as temps:
            cap = temps.enter_context(self._resident(raw))
            n_samples = max(0, cap.nsamples - first_sample) if n_samples is None else int(n_samples)
            frames = excise_frames(n_samples, nfft)
            thr = self._on_device(temps, threshold, np.float32, nfft, "threshold", f"nfft is {nfft}")
            rate = self._on_device(temps, rates, np.int32, frames, "rates", f"the range has {frames} frames of {nfft} points")
            self._count("excise_chirp")
            return self._cleaned(n_samples, frames, EXCISE_DTYPE, lambda d_out, d_rec: self.excise_chirp_dev(
                cap, cap.nbytes, first_sample, n_samples, nfft, rate, thr, d_out, d_rec))

    def cancel(self, a, b, weights, threshold=None, nfft: int = 1024, first_a: int = 0, first_b: int = 0,
               n_samples: Optional[int] = None, frames_per_set: Optional[int] = None):
        """Two-antenna per-bin cancellation (gj_cancel_dev): samples first_a .. + n_samples of ``a`` (default: as many as
        both captures hold) with ``W[k] * B_f[k]`` subtracted from every bin of every nfft-point frame, B_f being the frame
        of ``b`` at first_b, and every bin whose remaining power exceeds ``threshold[k]`` taken out.  ``a`` and ``b``:
        host bytes (uploaded once each) or resident ``Capture``s.  ``weights``: complex64[nfft] (one set) or
        complex64[n_sets][nfft] in FFT order (``gpsjam.coherence.cancel_weights`` builds them); frame f uses set
        ``min(f // frames_per_set, n_sets - 1)``, and ``frames_per_set`` defaults to all frames (needed only with more
        than one set).  ``threshold``: as ``excise``; None never excises.  Returns ``(cleaned, records)``: the cleaned
        range as a resident ``Capture`` of its own (the caller frees it) and one CANCEL_DTYPE record per frame."""
        nfft, first_a, first_b = int(nfft), int(first_a), int(first_b)
        w = np.asarray(weights)
        if w.ndim not in (1, 2) or w.shape[-1] != nfft or w.size == 0:
            raise ValueError(f"weights must be complex64[{nfft}] or [n_sets][{nfft}], not {w.shape}")
        return self._cancel("cancel", (a, b), (first_a, first_b), w.reshape(-1, nfft), threshold, nfft, n_samples, frames_per_set,
                            self.cancel_dev)

    def _cancel(self, name, raws, firsts, weights, threshold, nfft: int, n_samples, frames_per_set, launch):
        """The one body of ``cancel`` and ``cancel2`` behind their weights' shape check: main and its auxiliaries ``raws``
        resident, n_samples and frames_per_set defaulted, the threshold and ``weights`` ([n_sets][...], one row per set)
        on the device, and ``launch`` -- the caller's ``*_dev`` -- on (capture, nbytes, first) of every input and the
        arguments the two entry points share.  Device memory is taken in the order threshold, weights, output, records."""
        w = np.ascontiguousarray(weights, np.complex64)
        n_sets = w.shape[0]
        with contextlib.ExitStack() as temps:
            caps = self._residents(temps, *raws)
            if n_samples is None:
                n_samples = max(0, min(cap.nsamples - first for cap, first in zip(caps, firsts)))
            n_samples = int(n_samples)
            frames = excise_frames(n_samples, nfft)
            if frames_per_set is None:
                if n_sets > 1:
                    raise ValueError(f"{n_sets} weight sets need frames_per_set")
                frames_per_set = max(frames, 1)
            thr = np.full(nfft, np.inf, np.float32) if threshold is None else threshold
            thr = self._on_device(temps, thr, np.float32, nfft, "threshold", f"nfft is {nfft}")
            d_w = self._on_device(temps, w.view(np.float32), np.float32, 2 * w.size, "weights", "")
            self._count(name)
            inputs = [v for cap, first in zip(caps, firsts) for v in (cap, cap.nbytes, first)]
            return self._cleaned(n_samples, frames, CANCEL_DTYPE, lambda d_out, d_rec: launch(
                *inputs, n_samples, nfft, d_w, frames_per_set, n_sets, thr, d_out, d_rec))

    def cancel2(self, a, b, c, weights, threshold=None, nfft: int = 1024, first_a: int = 0, first_b: int = 0,
                first_c: int = 0, n_samples: Optional[int] = None, frames_per_set: Optional[int] = None):
        """Three-antenna per-bin cancellation (gj_cancel2_dev): ``cancel`` with two auxiliaries.  From every bin of every
        nfft-point frame of ``a`` at first_a, ``W1[k] * B_f[k]`` and then ``W2[k] * C_f[k]`` are subtracted, B_f and C_f
        being the frames of ``b`` at first_b and of ``c`` at first_c; n_samples defaults to as many as all three captures
        hold.  ``a``, ``b`` and ``c``: host bytes (uploaded once each) or resident ``Capture``s.  ``weights``:
        complex64[2][nfft] (one set: W1, W2) or complex64[n_sets][2][nfft] in FFT order
        (``gpsjam.coherence.cancel_weights2`` builds them); sets, ``frames_per_set``, ``threshold`` and the result
        ``(cleaned, records)`` as ``cancel``."""
        nfft, first_a, first_b, first_c = int(nfft), int(first_a), int(first_b), int(first_c)
        w = np.asarray(weights)
        if w.ndim not in (2, 3) or w.shape[-2:] != (2, nfft) or w.size == 0:
            raise ValueError(f"weights must be complex64[2][{nfft}] or [n_sets][2][{nfft}], not {w.shape}")
        return self._cancel("cancel2", (a, b, c), (first_a, first_b, first_c), w.reshape(-1, 2 * nfft), threshold, nfft, n_samples,
                            frames_per_set, self.cancel2_dev)

    def blank(self, raw, threshold: float, window: int = 16, guard: int = 8, first_sample: int = 0,
              n_samples: Optional[int] = None):
        """Time-domain pulse blanking (gj_blank_dev): samples first_sample .. + n_samples of ``raw`` (default: to the
        end) with every sample within ``guard`` of a ``window``-sample stretch whose mean power exceeds ``threshold``
        put to mid-level.  ``raw``: host bytes (uploaded once) or a resident ``Capture``; ``threshold``: a mean power per
        sample in LSB^2, the unit of ``onset(...).noise_power`` (+inf: never).  Returns ``(cleaned, records)``: the
        cleaned range as a resident ``Capture`` of its own (the caller frees it) and one BLANK_DTYPE record per
        BLANK_BLOCK samples."""
        first_sample = int(first_sample)
        with self._resident(raw) as cap:
            n_samples = max(0, cap.nsamples - first_sample) if n_samples is None else int(n_samples)
            blocks = blank_blocks(n_samples)
            self._count("blank")
            return self._cleaned(n_samples, blocks, BLANK_DTYPE, lambda d_out, d_rec: self.blank_dev(
                cap, cap.nbytes, first_sample, n_samples, window, guard, threshold, d_out, d_rec))

    def xcorr_fine(self, a, b, lag_center: int = 0, half_width: int = 16, first_a: int = 0, first_b: int = 0,
                   n_samples: Optional[int] = None, want_blocks: bool = False) -> FineCorr:
        """The exact correlation of two ranges at the 2 * half_width + 1 lags around ``lag_center``
        (gj_xcorr_fine_dev): ``c[k] = correlate(x_b, x_a, 'full')`` at lag ``lags[k]``, positive lags when b is delayed,
        over ``n_samples`` samples from ``first_a`` of a and ``first_b`` of b (default: as many as both hold).  ``a``
        and ``b``: host bytes (uploaded once each) or resident ``Capture``s; ``want_blocks``: also the sum of every
        FINE_BLOCK samples alone.  What a sub-sample delay is estimated from: ``gpsjam.tdoa.fine_lag``."""
        lag_center, half_width, first_a, first_b = int(lag_center), int(half_width), int(first_a), int(first_b)
        with contextlib.ExitStack() as temps:
            cap_a, cap_b = self._residents(temps, a, b)
            if n_samples is None:
                n_samples = max(0, min(cap_a.nsamples - first_a, cap_b.nsamples - first_b))
            n_samples, n_lags = int(n_samples), 2 * max(half_width, 0) + 1
            blocks = fine_blocks(n_samples) if want_blocks else 0
            d_total = temps.enter_context(DevBuf(self, 16 * n_lags))
            d_blocks = temps.enter_context(DevBuf(self, 8 * n_lags * max(blocks, 1))) if want_blocks else None
            self._count("xcorr_fine")
            self.xcorr_fine_dev(cap_a, cap_a.nbytes, first_a, cap_b, cap_b.nbytes, first_b, n_samples, lag_center,
                                half_width, d_total, d_blocks)
            total = d_total.download(np.int64, 2 * n_lags).reshape(n_lags, 2)
            rec = d_blocks.download(np.int32, 2 * n_lags * blocks).reshape(blocks, n_lags, 2) if want_blocks else None
        lags = lag_center - half_width + np.arange(n_lags, dtype=np.int64)
        c = (total[:, 0] + 1j * total[:, 1]) / 4.0
        return FineCorr(lags, c, None if rec is None else (rec[..., 0] + 1j * rec[..., 1]) / 4.0, n_samples)

    def corr_bank(self, capture, channels, codes, first_sample: int = 0, n_samples: Optional[int] = None,
                  block_samples: int = 2048, taps=(0, -1, 1)) -> CorrBank:
        """The correlator bank (gj_corr_bank_dev): every channel of ``channels`` mixed with its carrier, multiplied with
        its code row at every tap and summed per ``block_samples`` samples, over ``n_samples`` samples from
        ``first_sample`` (default: to the end).  ``capture``: host bytes (uploaded once) or a resident ``Capture``;
        ``channels``: CORR_CHANNEL_DTYPE records or (code_phase, code_step, carr_phase, carr_step, code_row, 0) rows,
        what ``gpsjam.postcorr.channel`` makes; ``codes``: int16[rows][1023] of +-1 on the host, or a device buffer
        ``(buffer, rows)``; ``taps``: whole-sample offsets.  The channel fields are checked HERE, on the host, before
        they are uploaded (GJ_ERR_INVALID): the library cannot answer for device memory with a status."""
        first_sample, block_samples = int(first_sample), int(block_samples)
        taps = tuple(int(d) for d in taps)
        with contextlib.ExitStack() as temps:
            cap, n_samples, d_codes, n_rows, rec, blocks = self._replica_inputs(temps, capture, channels, codes, first_sample,
                                                                                n_samples, block_samples)
            d_ch = temps.enter_context(DevBuf(self, max(rec.nbytes, 32))).upload(rec)
            d_out = temps.enter_context(DevBuf(self, 8 * max(rec.size * blocks * len(taps), 1)))
            self._count("corr_bank")
            self.corr_bank_dev(cap, cap.nbytes, first_sample, n_samples, block_samples, d_codes, n_rows, d_ch, rec.size, taps, d_out)
            iq = d_out.download(np.int32, 2 * rec.size * blocks * len(taps)).reshape(rec.size, blocks, len(taps), 2)
        return CorrBank(iq, taps, block_samples, n_samples)

    def subtract(self, capture, channels, codes, amplitudes, first_sample: int = 0, n_samples: Optional[int] = None,
                 block_samples: int = 256, dither: bool = True, seed: int = 0):
        """Counterfeit-signal subtraction (gj_subtract_dev): the replicas of ``channels`` -- each its code times its
        carrier times one complex amplitude per ``block_samples`` samples -- taken off samples first_sample ..
        + n_samples of ``capture`` (default: to the end).  ``capture``, ``channels`` and ``codes`` as in ``corr_bank``;
        ``amplitudes``: int32[n_channels][corr_blocks(n_samples, block_samples)][2] (aI, aQ) in units of 2^-SUB_FRAC,
        what ``gpsjam.postcorr.amplitudes`` makes of a bank's prompts, on the host or in a device buffer; ``dither``:
        the replica is brought down to whole LSB by a dithered floor (seeded by ``seed``) instead of rounding.  The
        channel fields are checked HERE, on the host (GJ_ERR_INVALID), as in ``corr_bank``.  Returns
        ``(cleaned, records)``: the cleaned range as a resident ``Capture`` of its own (the caller frees it) and one
        SUB_DTYPE record per SUB_BLOCK samples."""
        first_sample, block_samples = int(first_sample), int(block_samples)
        with contextlib.ExitStack() as temps:
            cap, n_samples, d_codes, n_rows, rec, blocks = self._replica_inputs(temps, capture, channels, codes, first_sample,
                                                                                n_samples, block_samples)
            d_amp = self._on_device(temps, amplitudes, np.int32, 2 * rec.size * blocks, "amplitudes",
                                    f"{rec.size} channels of {blocks} blocks take {2 * rec.size * blocks}")
            d_ch = temps.enter_context(DevBuf(self, max(rec.nbytes, 32))).upload(rec)
            self._count("subtract")
            return self._cleaned(n_samples, subtract_blocks(n_samples), SUB_DTYPE, lambda d_out, d_rec: self.subtract_dev(
                cap, cap.nbytes, first_sample, n_samples, block_samples, d_codes, n_rows, d_ch, rec.size, d_amp,
                _ffi.GJ_SUB_DITHER if dither else 0, seed, d_out, d_rec))

    def track(self, capture, states, codes, params, first_sample: int = 0, n_samples: Optional[int] = None,
              block_samples: int = 2048, n_epochs: Optional[int] = None):
        """Closed-loop tracking (gj_track_dev): every channel of ``states`` runs its DLL / FLL / PLL over ``n_epochs``
        epochs of ``block_samples`` samples inside samples first_sample .. + n_samples of ``capture`` (default: to the
        end), one workgroup per channel, one launch.  ``capture`` and ``codes`` as in ``corr_bank``; ``states``:
        TRACK_STATE_DTYPE records or rows of thirteen integers in that order, what ``gpsjam.track.states`` makes of an
        acquisition; ``params``: a ``TrackParams`` or (spacing, aid_div, pll_p, pll_i, fll, dll_p, dll_i), what
        ``gpsjam.track.gains`` makes of loop bandwidths; ``n_epochs``: default the most that every channel's ``start``
        leaves room for.  The states are checked HERE, on the host, before they are uploaded (GJ_ERR_INVALID), as the
        bank's channels are.  Returns ``(records, states)``: TRACK_EPOCH_DTYPE[n_channels][n_epochs] and the states
        behind the last epoch, with which a next call goes on."""
        first_sample, block_samples = int(first_sample), int(block_samples)
        params = _track_params(params)
        rec = _track_states(states)
        with contextlib.ExitStack() as temps:
            cap, n_samples, d_codes, n_rows, _, _ = self._replica_inputs(temps, capture, rec["ch"], codes, first_sample,
                                                                         n_samples, block_samples)
            if n_epochs is None:
                room = n_samples - (int(rec["start"].max()) if rec.size else 0)
                n_epochs = min(max(room, 0) // block_samples, TRACK_MAX_EPOCHS) if block_samples > 0 else 0
            n_epochs = int(n_epochs)
            for k, s in enumerate(rec):
                what = None
                if s["reserved"].any():
                    what = "reserved must be 0"
                elif int(s["primed"]) not in (0, 1):
                    what = f"primed {int(s['primed'])} is neither 0 nor 1"
                elif int(s["start"]) + n_epochs * block_samples > n_samples:
                    what = f"{n_epochs} epochs of {block_samples} samples from start {int(s['start'])} run past the range's {n_samples}"
                if what:
                    raise GpsJamError(-1, f"invalid argument: state {k}: {what}")
            d_st = temps.enter_context(DevBuf(self, max(rec.nbytes, 64))).upload(rec)
            d_out = temps.enter_context(DevBuf(self, TRACK_EPOCH_DTYPE.itemsize * max(rec.size * max(n_epochs, 0), 1)))
            self._count("track")
            self.track_dev(cap, cap.nbytes, first_sample, n_samples, block_samples, n_epochs, d_codes, n_rows, d_st, rec.size,
                           params, d_out)
            out = d_out.download(TRACK_EPOCH_DTYPE, rec.size * n_epochs).reshape(rec.size, n_epochs)
            return out, d_st.download(TRACK_STATE_DTYPE, rec.size)

    def subtract_tracked(self, capture, channels, codes, records, amplitudes, first_sample: int = 0,
                         n_samples: Optional[int] = None, block_samples: int = 2048, dither: bool = True, seed: int = 0,
                         n_epochs: Optional[int] = None):
        """Subtraction of tracked signals (gj_subtract_track_dev): ``subtract`` with the replica's NCOs taken per epoch
        from the records ``track`` returned.  ``channels``: SUB_TRACK_CHANNEL_DTYPE records or (start, code_row) rows, one
        per tracked channel, ``start`` being its state's; ``records``: TRACK_EPOCH_DTYPE[n_channels][n_epochs], on the
        host or in a device buffer (the one gj_track_dev wrote, as it is); ``amplitudes``: int32[n_channels][n_epochs][2]
        in units of 2^-SUB_FRAC, what ``gpsjam.track.amplitudes`` makes of the records' prompts, on the host or in a
        device buffer; ``n_epochs``: needed only where neither of the two is on the host.  ``capture``, ``codes``,
        ``dither`` and ``seed`` as in ``subtract``.  The channel table is checked HERE, on the host (GJ_ERR_INVALID); a
        record whose code NCO is out of bounds is not an error: by the definition its epoch is left alone.  Samples in
        front of a channel's ``start`` and behind its last whole epoch keep that channel's signal.  Returns
        ``(cleaned, records)`` as ``subtract`` does."""
        first_sample, block_samples = int(first_sample), int(block_samples)
        with contextlib.ExitStack() as temps:
            cap, n_samples, d_codes, n_rows, _, _ = self._replica_inputs(temps, capture, (), codes, first_sample, n_samples,
                                                                         block_samples)
            n_ch = len(channels)
            on_device = lambda v: isinstance(v, (DevBuf, int)) or hasattr(v, "data_ptr")
            if n_epochs is None:
                host = next((np.asarray(v) for v in (records, amplitudes) if not on_device(v)), None)
                if host is None:
                    raise ValueError("records and amplitudes are both on the device: n_epochs must be given")
                per = 1 if host.dtype == TRACK_EPOCH_DTYPE else 2
                n_epochs = host.size // (per * n_ch) if n_ch else 0
            n_epochs = int(n_epochs)
            rec = _subtract_track_channels(channels, n_rows, n_epochs, block_samples, n_samples)
            if not on_device(records):
                host = np.ascontiguousarray(records)
                if host.dtype != TRACK_EPOCH_DTYPE or host.size != rec.size * n_epochs:
                    raise ValueError(f"records must be TRACK_EPOCH_DTYPE[{rec.size}][{n_epochs}]")
                records = temps.enter_context(DevBuf(self, max(host.nbytes, 8))).upload(host.reshape(-1))
            d_amp = self._on_device(temps, amplitudes, np.int32, 2 * rec.size * n_epochs, "amplitudes",
                                    f"{rec.size} channels of {n_epochs} epochs take {2 * rec.size * n_epochs}")
            d_ch = temps.enter_context(DevBuf(self, max(rec.nbytes, 8))).upload(rec)
            self._count("subtract_tracked")
            return self._cleaned(n_samples, subtract_blocks(n_samples), SUB_DTYPE, lambda d_out, d_rec: self.subtract_track_dev(
                cap, cap.nbytes, first_sample, n_samples, block_samples, n_epochs, d_codes, n_rows, d_ch, rec.size, records, d_amp,
                _ffi.GJ_SUB_DITHER if dither else 0, seed, d_out, d_rec))

    def align(self, capture, params, taps, rot, n_out: Optional[int] = None):
        """Pair alignment (gj_align_dev): ``n_out`` samples (default: as many as ``capture`` holds) read from ``capture``
        along the time base and the phase of ``params`` -- an ``AlignParams`` or ``(pos0, pos_step, rot_phase, rot_step)``,
        what ``gpsjam.align.params`` makes of a lag, a drift and an offset -- through the polyphase rows ``taps``
        (int16[ALIGN_PHASES][ALIGN_TAPS], ``gpsjam.align.taps``) and the turn ``rot`` (int16[ALIGN_ROT_LEN],
        ``gpsjam.align.rot_table``), each on the host (uploaded) or in a device buffer.  ``capture``: host bytes
        (uploaded once) or a resident ``Capture``.  Returns ``(aligned, records)``: a resident ``Capture`` of its own
        (the caller frees it) and one ALIGN_DTYPE record per ALIGN_BLOCK samples.  The arguments are checked by the
        library: a refusal raises ``GpsJamError``."""
        params = _align_params(params)
        with contextlib.ExitStack() as temps:
            cap = temps.enter_context(self._resident(capture))
            n_out = cap.nsamples if n_out is None else int(n_out)
            d_taps = self._on_device(temps, taps, np.int16, ALIGN_PHASES * ALIGN_TAPS, "taps",
                                     f"{ALIGN_PHASES} rows of {ALIGN_TAPS} take {ALIGN_PHASES * ALIGN_TAPS}")
            d_rot = self._on_device(temps, rot, np.int16, ALIGN_ROT_LEN, "rot", f"one turn takes {ALIGN_ROT_LEN}")
            self._count("align")
            return self._cleaned(max(n_out, 0), align_blocks(max(n_out, 0)), ALIGN_DTYPE, lambda d_out, d_rec: self.align_dev(
                cap, cap.nbytes, params, d_taps, d_rot, n_out, d_out, d_rec))

    def acq_peaks(self, power, k: int = 2, guard: int = 4, shape=None):
        """The K-peak search (gj_acq_peaks_dev) over power surfaces double[n_prn][n_freq][nsamp]: per PRN the ``k``
        largest peaks under successive exclusion of the columns within ``guard`` (circular) of a peak already taken, and
        the mean of the columns left.  ``power``: a float64 array of that shape on the host (uploaded), or a device
        buffer with ``shape = (n_prn, n_freq, nsamp)``.  Returns ``(peaks, floor)``: ACQ_PEAK_DTYPE[n_prn][k] and
        ACQ_FLOOR_DTYPE[n_prn].  The arguments are checked by the library: a refusal raises ``GpsJamError``."""
        k, guard = int(k), int(guard)
        with contextlib.ExitStack() as temps:
            if isinstance(power, (DevBuf, int)) or hasattr(power, "data_ptr"):
                if shape is None or len(shape) != 3:
                    raise ValueError("a device surface needs shape = (n_prn, n_freq, nsamp)")
                d_power = power
            else:
                host = np.ascontiguousarray(power, np.float64)
                if host.ndim != 3:
                    raise ValueError("power must be float64[n_prn][n_freq][nsamp]")
                shape = host.shape
                d_power = temps.enter_context(DevBuf(self, max(host.nbytes, 8))).upload(host)
            n_prn, n_freq, nsamp = (int(v) for v in shape)
            records = max(n_prn, 1) * min(max(k, 1), ACQ_MAX_PEAKS)
            d_peaks = temps.enter_context(DevBuf(self, ACQ_PEAK_DTYPE.itemsize * records))
            d_floor = temps.enter_context(DevBuf(self, ACQ_FLOOR_DTYPE.itemsize * max(n_prn, 1)))
            self._count("acq_peaks")
            self.acq_peaks_dev(d_power, n_prn, n_freq, nsamp, k, guard, d_peaks, d_floor)
            return d_peaks.download(ACQ_PEAK_DTYPE, n_prn * k).reshape(n_prn, k), d_floor.download(ACQ_FLOOR_DTYPE, n_prn)

    # ------------------------------------------------------------------ device pointers
    def acq_peaks_workspace(self, nsamp: int, n_prn: int) -> int:
        return int(self._lib.gj_acq_peaks_workspace(self._ctx, int(nsamp), int(n_prn)))

    def acq_peaks_dev(self, d_power, n_prn, n_freq, nsamp, k, guard, d_peaks, d_floor):
        """gj_acq_peaks_dev: gj_acq_peak[n_prn][k] into d_peaks and gj_acq_floor[n_prn] into d_floor, on the context's
        stream."""
        args = [int(v) for v in (n_prn, n_freq, nsamp, k, guard)]
        if any(not -2 ** 31 <= v < 2 ** 31 for v in args):
            raise GpsJamError(-5, "unsupported: an argument outside int32")
        self._check(self._lib.gj_acq_peaks_dev(self._ctx, _ptr(d_power) or None, *args, _ptr(d_peaks) or None, _ptr(d_floor) or None))

    def corr_bank_dev(self, d_iq, nbytes, first_sample, n_samples, block_samples, d_codes, n_code_rows, d_channels, n_channels,
                      taps, d_out):
        """gj_corr_bank_dev: int32 (I, Q) of every channel, block and tap into d_out, on the context's stream; ``taps`` is a
        host sequence of whole-sample offsets."""
        taps = [int(d) for d in taps]
        if any(not -2 ** 31 <= d < 2 ** 31 for d in taps):
            raise GpsJamError(-5, "unsupported: a tap offset outside int32")
        arr = (C.c_int32 * max(len(taps), 1))(*taps)
        self._check(self._lib.gj_corr_bank_dev(self._ctx, _ptr(d_iq), int(nbytes), int(first_sample), int(n_samples),
                                               int(block_samples), _ptr(d_codes), int(n_code_rows), _ptr(d_channels),
                                               int(n_channels), arr, len(taps), _ptr(d_out)))

    def track_dev(self, d_iq, nbytes, first_sample, n_samples, block_samples, n_epochs, d_codes, n_code_rows, d_states,
                  n_channels, params, d_out):
        """gj_track_dev: one 56-byte record (TRACK_EPOCH_DTYPE) per channel and epoch into d_out and the 64-byte states
        (TRACK_STATE_DTYPE) in d_states advanced in place, on the context's stream."""
        args = [int(v) for v in (block_samples, n_epochs, n_code_rows, n_channels)]
        if any(not -2 ** 31 <= v < 2 ** 31 for v in args):
            raise GpsJamError(-5, "unsupported: an argument outside int32")
        self._check(self._lib.gj_track_dev(self._ctx, _ptr(d_iq), int(nbytes), int(first_sample), int(n_samples), args[0], args[1],
                                           _ptr(d_codes), args[2], _ptr(d_states), args[3], _track_params(params), _ptr(d_out)))

    def subtract_dev(self, d_iq, nbytes, first_sample, n_samples, block_samples, d_codes, n_code_rows, d_channels, n_channels,
                     d_amp, flags, seed, d_out, d_blocks=None):
        """gj_subtract_dev: 2 * n_samples cleaned bytes into d_out and, if asked for, one 24-byte record (SUB_DTYPE) per
        SUB_BLOCK samples into d_blocks, on the context's stream; ``seed`` is taken modulo 2^32."""
        self._check(self._lib.gj_subtract_dev(self._ctx, _ptr(d_iq), int(nbytes), int(first_sample), int(n_samples),
                                              int(block_samples), _ptr(d_codes), int(n_code_rows), _ptr(d_channels),
                                              int(n_channels), _ptr(d_amp), int(flags), int(seed) & 0xFFFFFFFF, _ptr(d_out),
                                              _ptr(d_blocks) or None))

    def subtract_track_dev(self, d_iq, nbytes, first_sample, n_samples, block_samples, n_epochs, d_codes, n_code_rows, d_channels,
                           n_channels, d_epochs, d_amp, flags, seed, d_out, d_blocks=None):
        """gj_subtract_track_dev: 2 * n_samples cleaned bytes into d_out and, if asked for, one 24-byte record (SUB_DTYPE)
        per SUB_BLOCK samples into d_blocks, on the context's stream; ``d_epochs``: the 56-byte records gj_track_dev wrote;
        ``seed`` is taken modulo 2^32."""
        args = [int(v) for v in (block_samples, n_epochs, n_code_rows, n_channels, flags)]
        if any(not -2 ** 31 <= v < 2 ** 31 for v in args):
            raise GpsJamError(-5, "unsupported: an argument outside int32")
        self._check(self._lib.gj_subtract_track_dev(self._ctx, _ptr(d_iq), int(nbytes), int(first_sample), int(n_samples), args[0],
                                                    args[1], _ptr(d_codes), args[2], _ptr(d_channels), args[3], _ptr(d_epochs),
                                                    _ptr(d_amp), args[4], int(seed) & 0xFFFFFFFF, _ptr(d_out), _ptr(d_blocks) or None))

    def align_dev(self, d_iq, nbytes, params, d_taps, d_rot, n_out, d_out, d_blocks=None):
        """gj_align_dev: 2 * n_out aligned bytes into d_out and, if asked for, one 16-byte record (ALIGN_DTYPE) per
        ALIGN_BLOCK samples into d_blocks, on the context's stream."""
        if not 0 <= int(n_out) < 2 ** 64 or not 0 <= int(nbytes) < 2 ** 64:
            raise GpsJamError(-5, "unsupported: a size outside 64 bits")
        self._check(self._lib.gj_align_dev(self._ctx, _ptr(d_iq), int(nbytes), _align_params(params), _ptr(d_taps), _ptr(d_rot),
                                           int(n_out), _ptr(d_out), _ptr(d_blocks) or None))

    def xcorr_fine_dev(self, d_a, nbytes_a, first_a, d_b, nbytes_b, first_b, n_samples, lag_center, half_width, d_total,
                       d_blocks=None):
        """gj_xcorr_fine_dev: int64 (re, im) of the 2 * half_width + 1 lags into d_total and, if asked for, the int32
        (re, im) of every FINE_BLOCK samples into d_blocks, on the context's stream."""
        self._check(self._lib.gj_xcorr_fine_dev(self._ctx, _ptr(d_a), int(nbytes_a), int(first_a), _ptr(d_b), int(nbytes_b),
                                                int(first_b), int(n_samples), int(lag_center), int(half_width),
                                                _ptr(d_total), _ptr(d_blocks) or None))

    def blank_dev(self, d_iq, nbytes, first_sample, n_samples, window, guard, threshold, d_out, d_blocks=None):
        """gj_blank_dev: 2 * n_samples cleaned bytes into d_out and, if asked for, one 24-byte record (BLANK_DTYPE) per
        BLANK_BLOCK samples into d_blocks, on the context's stream."""
        self._check(self._lib.gj_blank_dev(self._ctx, _ptr(d_iq), int(nbytes), int(first_sample), int(n_samples), int(window),
                                           int(guard), float(threshold), _ptr(d_out), _ptr(d_blocks) or None))

    def excise_chirp_dev(self, d_iq, nbytes, first_sample, n_samples, nfft, d_rate, d_threshold, d_out, d_frames=None):
        """gj_excise_chirp_dev: gj_excise_dev with the int32 rate of every frame in d_rate, on the context's stream."""
        self._check(self._lib.gj_excise_chirp_dev(self._ctx, _ptr(d_iq), int(nbytes), int(first_sample), int(n_samples),
                                                  int(nfft), _ptr(d_rate), _ptr(d_threshold), _ptr(d_out),
                                                  _ptr(d_frames) or None))

    def chirp_rates_dev(self, d_scan, n_frames, rate_first, rate_step, min_concentration, d_rate):
        """gj_chirp_rates_dev: the int32 rate of every frame of a gj_chirp_dev scan (0 where peak < min_concentration *
        total) into d_rate, on the context's stream."""
        self._check(self._lib.gj_chirp_rates_dev(self._ctx, _ptr(d_scan), int(n_frames), int(rate_first), int(rate_step),
                                                 float(min_concentration), _ptr(d_rate)))

    def cancel_dev(self, d_a, nbytes_a, first_a, d_b, nbytes_b, first_b, n_samples, nfft, d_weights, frames_per_set, n_sets,
                   d_threshold, d_out, d_frames=None):
        """gj_cancel_dev: 2 * n_samples cleaned bytes into d_out and, if asked for, one 16-byte record (CANCEL_DTYPE) per
        frame into d_frames, with the float32[n_sets][nfft][2] weights in d_weights, on the context's stream."""
        self._check(self._lib.gj_cancel_dev(self._ctx, _ptr(d_a), int(nbytes_a), int(first_a), _ptr(d_b), int(nbytes_b),
                                            int(first_b), int(n_samples), int(nfft), _ptr(d_weights), int(frames_per_set),
                                            int(n_sets), _ptr(d_threshold), _ptr(d_out), _ptr(d_frames) or None))

    def cancel2_dev(self, d_a, nbytes_a, first_a, d_b, nbytes_b, first_b, d_c, nbytes_c, first_c, n_samples, nfft, d_weights,
                    frames_per_set, n_sets, d_threshold, d_out, d_frames=None):
        """gj_cancel2_dev: gj_cancel_dev with a third capture and the float32[n_sets][2][nfft][2] weights (W1, then W2, of
        every set) in d_weights, on the context's stream."""
        self._check(self._lib.gj_cancel2_dev(self._ctx, _ptr(d_a), int(nbytes_a), int(first_a), _ptr(d_b), int(nbytes_b),
                                             int(first_b), _ptr(d_c), int(nbytes_c), int(first_c), int(n_samples), int(nfft),
                                             _ptr(d_weights), int(frames_per_set), int(n_sets), _ptr(d_threshold), _ptr(d_out),
                                             _ptr(d_frames) or None))

    def excise_dev(self, d_iq, nbytes, first_sample, n_samples, nfft, d_threshold, d_out, d_frames=None):
        """gj_excise_dev: 2 * n_samples cleaned bytes into d_out and, if asked for, one 16-byte record (EXCISE_DTYPE) per
        frame into d_frames, on the context's stream."""
        self._check(self._lib.gj_excise_dev(self._ctx, _ptr(d_iq), int(nbytes), int(first_sample), int(n_samples), int(nfft),
                                            _ptr(d_threshold), _ptr(d_out), _ptr(d_frames) or None))

    def spectral_kurtosis_dev(self, d_iq, nbytes, first_sample, nfft, hop, frames_per_row, n_rows, d_s1, d_s2, d_sk=None):
        """gj_sk_dev: float32[n_rows][nfft] sums of P into d_s1 and of P^2 into d_s2 and, if asked for, the estimator
        into d_sk, on the context's stream."""
        self._check(self._lib.gj_sk_dev(self._ctx, _ptr(d_iq), int(nbytes), int(first_sample), int(nfft), int(hop),
                                        int(frames_per_row), int(n_rows), _ptr(d_s1), _ptr(d_s2), _ptr(d_sk) or None))

    def sk_workspace(self, nfft: int, frames_per_row: int, n_rows: int) -> int:
        return self._lib.gj_sk_workspace(self._ctx, int(nfft), int(frames_per_row), int(n_rows))

    def cross_spectrum_dev(self, d_a, nbytes_a, first_a, d_b, nbytes_b, first_b, nfft, hop, frames_per_row, n_rows, d_saa,
                           d_sbb, d_sab, d_msc=None):
        """gj_csd_dev: float32[n_rows][nfft] sums of |A|^2 into d_saa and of |B|^2 into d_sbb, float32[n_rows][nfft][2]
        (re, im) sums of B conj(A) into d_sab and, if asked for, the coherence into d_msc, on the context's stream."""
        self._check(self._lib.gj_csd_dev(self._ctx, _ptr(d_a), int(nbytes_a), int(first_a), _ptr(d_b), int(nbytes_b),
                                         int(first_b), int(nfft), int(hop), int(frames_per_row), int(n_rows), _ptr(d_saa),
                                         _ptr(d_sbb), _ptr(d_sab), _ptr(d_msc) or None))

    def csd_workspace(self, nfft: int, frames_per_row: int, n_rows: int) -> int:
        return self._lib.gj_csd_workspace(self._ctx, int(nfft), int(frames_per_row), int(n_rows))

    def ridge_dev(self, d_iq, nbytes, first_sample, nfft, hop, n_frames, guard, d_out):
        """gj_ridge_dev: n_frames records of 16 bytes (RIDGE_DTYPE) into d_out, on the context's stream."""
        self._check(self._lib.gj_ridge_dev(self._ctx, _ptr(d_iq), int(nbytes), int(first_sample), int(nfft), int(hop),
                                           int(n_frames), int(guard), _ptr(d_out)))

    def chirp_dev(self, d_iq, nbytes, first_sample, nfft, hop, n_frames, guard, rate_first, rate_step, n_rates, d_out, d_peaks=None):
        """gj_chirp_dev: n_frames records of 24 bytes (CHIRP_DTYPE) into d_out and, if asked for, float32[n_frames][n_rates]
        peaks into d_peaks, on the context's stream."""
        self._check(self._lib.gj_chirp_dev(self._ctx, _ptr(d_iq), int(nbytes), int(first_sample), int(nfft), int(hop),
                                           int(n_frames), int(guard), int(rate_first), int(rate_step), int(n_rates),
                                           _ptr(d_out), _ptr(d_peaks) or None))

    def chunk_count(self, nbytes: int, chunk_bytes: int) -> int:
        return self._lib.gj_chunk_count(nbytes, chunk_bytes)

    def welch_rows(self, nbytes: int, chunk_samples: int, nperseg: int) -> int:
        return self._lib.gj_welch_rows(nbytes, chunk_samples, nperseg)

    def welch_workspace(self, nbytes: int, chunk_samples: int, nperseg: int) -> int:
        return self._lib.gj_welch_workspace(self._ctx, nbytes, chunk_samples, nperseg)

    def xcorr_workspace(self, n_ant: int, n_samples: int, n_pairs: int) -> int:
        return self._lib.gj_xcorr_workspace(self._ctx, n_ant, n_samples, n_pairs)

    def chunk_power_dev(self, d_iq, nbytes, chunk_bytes, d_power, eps=1e-10, flags=0):
        self._check(self._lib.gj_chunk_power_dev(self._ctx, _ptr(d_iq), nbytes, chunk_bytes, eps,
                                                 flags, _ptr(d_power)))

    def power_threshold_dev(self, d_power, n, d_stats, d_mask=None, pct=5.0, rise_db=6.0):
        self._check(self._lib.gj_power_threshold_dev(self._ctx, _ptr(d_power), n, pct, rise_db,
                                                     _ptr(d_stats), _ptr(d_mask) or None))

    def welch_dev(self, d_iq, nbytes, chunk_samples, nperseg, fs, d_psd, d_psd_db=None, shift=True):
        self._check(self._lib.gj_welch_dev(self._ctx, _ptr(d_iq), nbytes, chunk_samples, nperseg,
                                           fs, _ffi.GJ_WELCH_SHIFT if shift else 0, _ptr(d_psd),
                                           _ptr(d_psd_db) or None))

    def welch_batch_dev(self, d_iqs, nbytes_each, chunk_samples, nperseg, fs, d_psds, shift=True):
        """K2 of several captures of ONE length in one launch + one finalize (gj_welch_batch_dev); same bits per capture
        as welch_dev."""
        n = len(d_iqs)
        iq = (C.c_void_p * n)(*[_ptr(p) for p in d_iqs])
        out = (C.c_void_p * n)(*[_ptr(p) for p in d_psds])
        self._check(self._lib.gj_welch_batch_dev(self._ctx, iq, n, int(nbytes_each), chunk_samples, nperseg, fs,
                                                 _ffi.GJ_WELCH_SHIFT if shift else 0, out))

    def pack_results_dev(self, captures, nperseg, d_pairs=None, d_lags=None, d_peaks=None, d_margins=None):
        """One result vector per capture in ONE launch (gj_pack_results_dev); ``captures``: list of _ffi.CombineCapture."""
        ca = (_ffi.CombineCapture * len(captures))(*captures)
        self._check(self._lib.gj_pack_results_dev(self._ctx, ca, len(captures), nperseg, _ptr(d_pairs) or None, _ptr(d_lags) or None,
                                                  _ptr(d_peaks) or None, _ptr(d_margins) or None))

    def welch_timed_dev(self, d_iq, nbytes, chunk_samples, nperseg, fs, d_psd, d_psd_db=None, shift=True):
        """welch_dev with events around the transform kernel and around the finalize launch; synchronises.
        Returns (kernel_ms, finalize_ms) (gj_welch_timed_dev)."""
        k, f = C.c_float(0), C.c_float(0)
        self._check(self._lib.gj_welch_timed_dev(self._ctx, _ptr(d_iq), nbytes, chunk_samples, nperseg, fs,
                                                 _ffi.GJ_WELCH_SHIFT if shift else 0, _ptr(d_psd), _ptr(d_psd_db) or None,
                                                 C.byref(k), C.byref(f)))
        return float(k.value), float(f.value)

    def byte_histogram_dev(self, d_iq, nbytes, chunk_samples, nperseg, stride, d_hist):
        self._check(self._lib.gj_byte_histogram_dev(self._ctx, _ptr(d_iq), nbytes, chunk_samples,
                                                    nperseg, stride, _ptr(d_hist)))

    def amp_stats_dev(self, d_iq, nbytes, threshold, d_out):
        self._check(self._lib.gj_amp_stats_dev(self._ctx, _ptr(d_iq), nbytes, threshold, _ptr(d_out)))

    def onset_dev(self, d_iq, nbytes, noise_samples, window, factor, d_out):
        self._check(self._lib.gj_onset_dev(self._ctx, _ptr(d_iq), nbytes, noise_samples, window,
                                           factor, _ptr(d_out)))

    def stream_scan_dev(self, d_iq, nbytes, chunk_bytes, d_power, rssi_threshold, d_amp, noise_samples, window,
                        factor, d_onset, eps=1e-10, flags=0):
        """K1 + K3 + K4 in one pass over the capture (gj_stream_scan_dev)."""
        self._check(self._lib.gj_stream_scan_dev(self._ctx, _ptr(d_iq), nbytes, chunk_bytes, eps, flags,
                                                 _ptr(d_power), rssi_threshold, _ptr(d_amp), noise_samples,
                                                 window, factor, _ptr(d_onset)))

    @staticmethod
    def _scan_extra(d_stats, d_mask, pct, rise_db, slice_samples, d_slot):
        return _ffi.ScanExtra(float(pct), float(rise_db), _ptr(d_stats) or None, _ptr(d_mask) or None,
                              int(slice_samples) if d_slot is not None else 0, _ptr(d_slot) or None)

    def capture_scan_dev(self, d_iq, nbytes, chunk_bytes, d_power, rssi_threshold, d_amp, noise_samples, window,
                         factor, d_onset, *, d_stats=None, d_mask=None, pct=5.0, rise_db=6.0, slice_samples=0, d_slot=None,
                         eps=1e-10, flags=0):
        """The per-capture side chain in two launches (gj_capture_scan_dev): the fused pass, then one tail launch with
        the noise-floor threshold (``d_stats`` / ``d_mask``), the amplitude totals, the onset record and the TDOA slot cut
        at that onset (``d_slot``, ``slice_samples``).  Same results as stream_scan_dev + power_threshold_dev +
        tdoa_slot_dev."""
        x = self._scan_extra(d_stats, d_mask, pct, rise_db, slice_samples, d_slot)
        self._check(self._lib.gj_capture_scan_dev(self._ctx, _ptr(d_iq), nbytes, chunk_bytes, eps, flags,
                                                  _ptr(d_power), rssi_threshold, _ptr(d_amp), noise_samples,
                                                  window, factor, _ptr(d_onset), C.byref(x)))

    def tdoa_slot_bytes(self, n_samples: int) -> int:
        return self._lib.gj_tdoa_slot_bytes(n_samples)

    def tdoa_slot_dev(self, d_iq, nbytes, d_start, n_samples, d_slot):
        """Cut the slice that starts at the DEVICE scalar *d_start into a TDOA slot."""
        self._check(self._lib.gj_tdoa_slot_dev(self._ctx, _ptr(d_iq), nbytes, _ptr(d_start), n_samples, _ptr(d_slot)))

    def xcorr_slots_dev(self, d_slots, slot_stride, n_ant, n_samples, pairs, d_lags, d_peaks, d_margins=None):
        flat = np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(-1))
        self._check(self._lib.gj_xcorr_slots_dev(
            self._ctx, _ptr(d_slots), slot_stride, n_ant, n_samples,
            flat.ctypes.data_as(C.POINTER(C.c_int32)), flat.size // 2, _ptr(d_lags), _ptr(d_peaks),
            _ptr(d_margins) or None))

    def xcorr_lags_dev(self, d_iqs, nbytes_list, d_starts, n_samples, pairs, d_lags, d_peaks, d_margins=None):
        n_ant = len(d_iqs)
        ptrs = (C.c_void_p * n_ant)(*[_ptr(p) for p in d_iqs])
        sizes = (C.c_size_t * n_ant)(*[int(b) for b in nbytes_list])
        flat = np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(-1))
        self._check(self._lib.gj_xcorr_lags_dev(
            self._ctx, ptrs, sizes, n_ant, _ptr(d_starts), n_samples,
            flat.ctypes.data_as(C.POINTER(C.c_int32)), flat.size // 2, _ptr(d_lags), _ptr(d_peaks),
            _ptr(d_margins) or None))

    def xcorr_caf_workspace(self, n_ant: int, n_samples: int, n_pairs: int, n_bins: int, bins_per_launch: int = 0) -> int:
        return self._lib.gj_xcorr_caf_workspace(self._ctx, n_ant, n_samples, n_pairs, n_bins, bins_per_launch)

    def xcorr_caf_dev(self, d_iqs, nbytes_list, d_starts, n_samples, pairs, bin_first, n_bins, d_out, d_bin_lags=None,
                      d_bin_peaks=None, bins_per_launch=0):
        """gj_xcorr_caf_dev: ``d_out`` receives one gj_caf_result (24 bytes) per pair, the optional ridge arrays
        [n_pairs][n_bins] int32 / float32.  Enqueues and returns."""
        n_ant = len(d_iqs)
        ptrs = (C.c_void_p * n_ant)(*[_ptr(p) for p in d_iqs])
        sizes = (C.c_size_t * n_ant)(*[int(b) for b in nbytes_list])
        flat = np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(-1))
        self._check(self._lib.gj_xcorr_caf_dev(
            self._ctx, ptrs, sizes, n_ant, _ptr(d_starts), n_samples, flat.ctypes.data_as(C.POINTER(C.c_int32)),
            flat.size // 2, int(bin_first), int(n_bins), int(bins_per_launch), _ptr(d_out), _ptr(d_bin_lags) or None,
            _ptr(d_bin_peaks) or None))

    def xcorr_caf_slots_dev(self, d_slots, slot_stride, n_ant, n_samples, pairs, bin_first, n_bins, d_out, d_bin_lags=None,
                            d_bin_peaks=None, bins_per_launch=0):
        """gj_xcorr_caf_slots_dev: the same over an array of TDOA slots."""
        flat = np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(-1))
        self._check(self._lib.gj_xcorr_caf_slots_dev(
            self._ctx, _ptr(d_slots), slot_stride, n_ant, n_samples, flat.ctypes.data_as(C.POINTER(C.c_int32)),
            flat.size // 2, int(bin_first), int(n_bins), int(bins_per_launch), _ptr(d_out), _ptr(d_bin_lags) or None,
            _ptr(d_bin_peaks) or None))

    def pack_result_dev(self, n_chunks, d_power, d_stats, d_amp, d_onset, d_psd, rows, nperseg, rank, n_pairs,
                        pair_capacity, d_pairs, d_lags, d_peaks, d_margins, d_out):
        self._check(self._lib.gj_pack_result_dev(self._ctx, n_chunks, _ptr(d_power), _ptr(d_stats), _ptr(d_amp),
                                                 _ptr(d_onset), _ptr(d_psd), rows, nperseg, rank, n_pairs, pair_capacity,
                                                 _ptr(d_pairs) or None, _ptr(d_lags) or None, _ptr(d_peaks) or None,
                                                 _ptr(d_margins) or None, _ptr(d_out)))

    # ------------------------------------------------------------------ one capture over several GPUs
    def amp_tile_count(self, nbytes: int) -> int:
        return self._lib.gj_amp_tile_count(int(nbytes))

    def part_scan_dev(self, view, chunk_bytes, d_power, rssi_threshold, d_tiles, d_amp, noise_samples, window, factor,
                      d_onset, eps=1e-10, flags=0):
        """K1 + K3 + K4 of one part (gj_part_scan_dev); ``view`` is a _ffi.PartView."""
        self._check(self._lib.gj_part_scan_dev(self._ctx, C.byref(view), chunk_bytes, eps, flags, _ptr(d_power),
                                               rssi_threshold, _ptr(d_tiles), _ptr(d_amp), noise_samples, window, factor,
                                               _ptr(d_onset)))

    def part_capture_scan_dev(self, view, chunk_bytes, d_power, rssi_threshold, d_tiles, d_amp, noise_samples, window,
                              factor, d_onset, *, slice_samples=0, d_slot=None, eps=1e-10, flags=0):
        """part_scan_dev + part_slot_dev (at the part's own onset) in two launches (gj_part_capture_scan_dev)."""
        x = self._scan_extra(None, None, 5.0, 6.0, slice_samples, d_slot)
        self._check(self._lib.gj_part_capture_scan_dev(self._ctx, C.byref(view), chunk_bytes, eps, flags, _ptr(d_power),
                                                       rssi_threshold, _ptr(d_tiles), _ptr(d_amp), noise_samples, window,
                                                       factor, _ptr(d_onset), C.byref(x)))

    def part_welch_dev(self, view, chunk_samples, nperseg, fs, d_psd, d_psd_db=None, shift=True):
        self._check(self._lib.gj_part_welch_dev(self._ctx, C.byref(view), chunk_samples, nperseg, fs,
                                                _ffi.GJ_WELCH_SHIFT if shift else 0, _ptr(d_psd), _ptr(d_psd_db) or None))

    def part_welch_workspace(self, view, chunk_samples, nperseg) -> int:
        return self._lib.gj_part_welch_workspace(self._ctx, C.byref(view), chunk_samples, nperseg)

    def part_slot_dev(self, view, d_start, n_samples, d_slot):
        self._check(self._lib.gj_part_slot_dev(self._ctx, C.byref(view), _ptr(d_start), n_samples, _ptr(d_slot)))

    def slots_pick_dev(self, d_slots, slot_stride, d_offsets, d_members, n_groups, d_out):
        self._check(self._lib.gj_slots_pick_dev(self._ctx, _ptr(d_slots), slot_stride, _ptr(d_offsets), _ptr(d_members),
                                                n_groups, _ptr(d_out)))

    def amp_combine_dev(self, d_tiles, n_tiles, d_parts, n_parts, total_bytes, d_out):
        self._check(self._lib.gj_amp_combine_dev(self._ctx, _ptr(d_tiles), n_tiles, _ptr(d_parts), n_parts, total_bytes,
                                                 _ptr(d_out)))

    def onset_combine_dev(self, d_parts, n_parts, d_out):
        self._check(self._lib.gj_onset_combine_dev(self._ctx, _ptr(d_parts), n_parts, _ptr(d_out)))

    def part_result_len(self, chunk_cap, tile_cap, rows_cap, nperseg, pair_cap) -> int:
        return self._lib.gj_part_result_len(chunk_cap, tile_cap, rows_cap, nperseg, pair_cap)

    def pack_part_dev(self, args, d_out):
        self._check(self._lib.gj_pack_part_dev(self._ctx, C.byref(args), _ptr(d_out)))

    def combine_plan(self, copies, captures, rows_bytes, arena, nperseg, d_pairs, d_lags, d_peaks, d_margins,
                     pct=5.0, rise_db=6.0):
        """gj_combine_plan_create: ``copies`` / ``captures`` are lists of _ffi.CombineCopy / _ffi.CombineCapture; ``arena``
        the one device allocation (torch uint8 tensor or DevBuf) every destination lies in.  Returns the plan handle."""
        cs = (_ffi.CombineCopy * len(copies))(*copies)
        ca = (_ffi.CombineCapture * len(captures))(*captures)
        nbytes = arena.numel() if hasattr(arena, "numel") else arena.nbytes
        h = C.c_void_p()
        self._check(self._lib.gj_combine_plan_create(self._ctx, cs, len(copies), ca, len(captures), int(rows_bytes), _ptr(arena),
                                                     int(nbytes), int(nperseg), pct, rise_db, _ptr(d_pairs), _ptr(d_lags),
                                                     _ptr(d_peaks), _ptr(d_margins), C.byref(h)))
        return h

    def split_combine_dev(self, plan, d_rows):
        """Every capture of a split run rebuilt and finished in three launches (gj_split_combine_dev)."""
        self._check(self._lib.gj_split_combine_dev(self._ctx, plan, _ptr(d_rows)))

    def combine_plan_destroy(self, plan):
        if getattr(self, "_ctx", None):
            self._lib.gj_combine_plan_destroy(self._ctx, plan)

    def synth_dev(self, spec, n_samples: int, d_out, first_sample: int = 0):
        """Fill d_out[2*n_samples] with the capture described by a synth.StreamSpec."""
        p = SynthParams(spec.key_noise, spec.key_common, spec.delay, spec.jam_start,
                        min(spec.jam_end, (1 << 62)), spec.noise_k, spec.jam_k, spec.dc_i_q8,
                        spec.dc_q_q8)
        self._check(self._lib.gj_synth_u8_dev(self._ctx, C.byref(p), first_sample, n_samples,
                                              _ptr(d_out)))
