"""The part every GPU test shares (tests/*/test_round6_gpu.py and the top-level test_*_gpu.py): the ``gj_status`` values,
sentinel-guarded device buffers, resident values, the refusal loop, and one ``run_<entry>`` per entry point under test.
Everything here touches a ``Device`` or gpsjam's dtypes; comparisons that take arrays only live with the restatement
they compare against (tests/<name>_restatement.py, tests/<name>_inputs.py).  tests/test_gpu_lib_host.py holds this
module to the host double of tests/host_lib.py: a guard that never fires is worth nothing.

No test module imports another (tests/test_suite_order.py holds that): what two of them need stands here or beside a
restatement."""
import ctypes as C

import numpy as np
import pytest

import align_restatement as ar
import corr_restatement as cr
import gpsjam
import subtract_restatement as sr
import track_restatement as tr
from gpsjam import _ffi

GJ_ERR_INVALID, GJ_ERR_UNSUPPORTED = -1, -5     # include/gpsjam.h gj_status
SENTINEL = 0xA5
PAD = 256                                       # sentinel bytes on either side of a guarded payload
CAF_REC = C.sizeof(_ffi.CafResult)
LAG_INVALID = _ffi.GJ_LAG_INVALID


class Guarded(gpsjam.DevBuf):
    """``nbytes`` of device memory between two runs of ``pad`` sentinel bytes, ``offset`` bytes off its 256-byte aligned
    place; filled with the sentinel too unless the test never reads what the call leaves unwritten.  A ``DevBuf`` whose
    ``ptr`` is the payload's: it goes wherever a buffer goes, ``ptr + k`` addresses the payload's byte k, and ``upload``
    and ``download`` count from there."""

    def __init__(self, dev, nbytes, offset=0, fill=True, pad=PAD):
        self.dev, self.nbytes, self.capacity, self.pad, self.lo, self.ptr = dev, int(nbytes), int(nbytes), int(pad), int(pad) + int(offset), 0
        self.buf = dev.alloc(self.lo + self.nbytes + self.pad)
        self.ptr = self.buf.ptr + self.lo
        if fill:
            self.refill()
        else:
            self.buf.upload(np.full(self.lo, SENTINEL, np.uint8))
            self.buf.upload(np.full(self.pad, SENTINEL, np.uint8), offset=self.lo + self.nbytes)

    def refill(self, nbytes=None):
        """Sentinel everywhere again, for another call into the same buffer; ``nbytes``: that call's (shorter) payload,
        the rear pad right behind it."""
        self.nbytes = self.capacity if nbytes is None else int(nbytes)
        assert 0 <= self.nbytes <= self.capacity
        self.buf.upload(np.full(self.lo + self.nbytes + self.pad, SENTINEL, np.uint8))

    def read(self, dtype=np.uint8, count=None, offset=0):
        if count is None:
            count = (self.nbytes - offset) // np.dtype(dtype).itemsize
        assert 0 <= offset and offset + count * np.dtype(dtype).itemsize <= self.nbytes
        return self.buf.download(dtype, count, self.lo + offset)

    def check_pads(self, what):
        front, back = self.buf.download(np.uint8, self.lo, 0), self.buf.download(np.uint8, self.pad, self.lo + self.nbytes)
        assert np.all(front == SENTINEL) and np.all(back == SENTINEL), f"bytes were written outside the call's {what}"

    def check_untouched(self, what):
        assert np.all(self.buf.download(np.uint8, self.lo + self.nbytes + self.pad) == SENTINEL), f"{what}: bytes were written"

    def free(self):
        if getattr(self, "buf", None) is not None:
            self.buf.free()
        self.ptr = 0


class Resident:
    """Arrays resident once per (dtype, values)."""

    def __init__(self, dev):
        self.dev, self.bufs = dev, {}

    def __call__(self, values, dtype=np.float32):
        values = np.ascontiguousarray(values, dtype)
        key = (np.dtype(dtype).str, values.tobytes())
        if key not in self.bufs:
            self.bufs[key] = self.dev.alloc(max(values.nbytes, 1)).upload(values.reshape(-1).view(np.uint8))
        return self.bufs[key]

    def free(self):
        for b in self.bufs.values():
            b.free()


class Convention:
    """offset and scale for the body, the default convention afterwards."""

    def __init__(self, dev, offset, scale):
        self.dev, self.offset, self.scale = dev, offset, scale

    def __enter__(self):
        self.dev.set_unpack(self.offset, self.scale)

    def __exit__(self, *exc):
        self.dev.set_unpack()
        assert self.dev.get_unpack() == (127.5, 1.0 / 127.5)


def freed(*bufs):
    for b in bufs:
        if b is not None:
            b.free()


def refused(dev, launch, cases, *guarded):
    """Every ``(args, status)`` of ``cases``: ``launch(*args)`` raises gpsjam.GpsJamError with exactly that status.
    Behind all of them, one synchronize(): no byte of a ``guarded`` buffer, payload or pads, has been written."""
    for args, status in cases:
        with pytest.raises(gpsjam.GpsJamError) as e:
            launch(*args)
        assert e.value.status == status, (args, e.value)
    dev.synchronize()
    for g in guarded:
        g.check_untouched("refused calls")


# ------------------------------------------------------------------------------------------------ the calls
def _checked(*outputs):
    """``outputs``: (Guarded, what, asked for).  An output that was asked for keeps both pads; one that was not keeps
    every byte."""
    for g, what, asked in outputs:
        if asked:
            g.check_pads(what)
        else:
            g.check_untouched(f"no {what} were asked for")


def _bytes_and_records(dev, n_samples, n_records, dtype, want_records, launch, out_offset=0):
    """(bytes[2 n_samples], dtype[n_records]) of ``launch(d_out, d_records or None)``, the shape of every cleaner's call.
    Records that were not asked for come back as the sentinel bytes they still are."""
    out, rec = Guarded(dev, 2 * n_samples, out_offset), Guarded(dev, n_records * np.dtype(dtype).itemsize)
    try:
        launch(out.ptr, rec.ptr if want_records else None)
        _checked((out, "output", True), (rec, "records", want_records))
        return out.read(), rec.read(dtype)
    finally:
        freed(out, rec)


def run_ridge(dev, d_iq, nbytes, nfft, hop, first, n_frames, guard):
    """n_frames records through gj_ridge_dev; 64 sentinel records on either side of them."""
    rec = gpsjam.RIDGE_DTYPE.itemsize
    out = Guarded(dev, n_frames * rec, pad=64 * rec)
    try:
        dev.ridge_dev(d_iq, nbytes, first, nfft, hop, n_frames, guard, out.ptr)
        out.check_pads("records")
        return out.read(gpsjam.RIDGE_DTYPE)
    finally:
        out.free()


def run_chirp(dev, d_iq, nbytes, nfft, hop, first, n_frames, rates, guard=2, want_peaks=True):
    """(records, peaks or None) of one gj_chirp_dev call; 64 sentinel records on either side of the records."""
    n_rates, rec = rates[2], gpsjam.CHIRP_DTYPE.itemsize
    out, pk = Guarded(dev, n_frames * rec, pad=64 * rec), Guarded(dev, n_frames * n_rates * 4)
    try:
        dev.chirp_dev(d_iq, nbytes, first, nfft, hop, n_frames, guard, rates[0], rates[1], n_rates, out.ptr, pk.ptr if want_peaks else None)
        _checked((out, "records", True), (pk, "peaks", want_peaks))
        got = out.read(gpsjam.CHIRP_DTYPE)
        assert not got["reserved"].any()
        return got, pk.read(np.float32).reshape(n_frames, n_rates) if want_peaks else None
    finally:
        freed(out, pk)


def run_sk(dev, d_iq, nbytes, nfft, hop, first, m, n_rows, want_sk=True):
    """(S1, S2, SK | None) as float32[n_rows][nfft] through gj_sk_dev."""
    bufs = [Guarded(dev, 4 * n_rows * nfft) for _ in range(3)]
    try:
        dev.spectral_kurtosis_dev(d_iq, nbytes, first, nfft, hop, m, n_rows, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr if want_sk else None)
        _checked((bufs[0], "S1", True), (bufs[1], "S2", True), (bufs[2], "SK", want_sk))
        out = [b.read(np.float32).reshape(n_rows, nfft) for b in bufs]
        return out[0], out[1], (out[2] if want_sk else None)
    finally:
        freed(*bufs)


def run_csd(dev, d_a, nbytes_a, first_a, d_b, nbytes_b, first_b, nfft, hop, m, n_rows, want_msc=True):
    """(Saa, Sbb, Sab, MSC | None) through gj_csd_dev."""
    cells = n_rows * nfft
    bufs = [Guarded(dev, s) for s in (4 * cells, 4 * cells, 8 * cells, 4 * cells)]
    try:
        dev.cross_spectrum_dev(d_a, nbytes_a, first_a, d_b, nbytes_b, first_b, nfft, hop, m, n_rows, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr,
                               bufs[3].ptr if want_msc else None)
        _checked((bufs[0], "Saa", True), (bufs[1], "Sbb", True), (bufs[2], "Sab", True), (bufs[3], "MSC", want_msc))
        saa, sbb = (bufs[k].read(np.float32).reshape(n_rows, nfft) for k in (0, 1))
        sab = bufs[2].read(np.complex64).reshape(n_rows, nfft)
        return saa, sbb, sab, (bufs[3].read(np.float32).reshape(n_rows, nfft) if want_msc else None)
    finally:
        freed(*bufs)


def run_excise(dev, d_iq, nbytes, first, n_samples, nfft, d_thr, want_frames=True):
    """(bytes[2 n_samples], records[F]) through gj_excise_dev."""
    return _bytes_and_records(dev, n_samples, gpsjam.excise_frames(n_samples, nfft), gpsjam.EXCISE_DTYPE, want_frames,
                              lambda d_out, d_rec: dev.excise_dev(d_iq, nbytes, first, n_samples, nfft, d_thr, d_out, d_rec))


def run_excise_chirp(dev, d_iq, nbytes, first, n_samples, nfft, d_rate, d_thr, want_frames=True, plain=False):
    """(bytes[2 n_samples], records[F]) through gj_excise_chirp_dev (plain: gj_excise_dev)."""
    if plain:
        return run_excise(dev, d_iq, nbytes, first, n_samples, nfft, d_thr, want_frames)
    return _bytes_and_records(dev, n_samples, gpsjam.excise_frames(n_samples, nfft), gpsjam.EXCISE_DTYPE, want_frames,
                              lambda d_out, d_rec: dev.excise_chirp_dev(d_iq, nbytes, first, n_samples, nfft, d_rate, d_thr, d_out, d_rec))


def run_cancel(dev, d_a, nbytes_a, first_a, d_b, nbytes_b, first_b, n_samples, nfft, d_w, frames_per_set, n_sets, d_thr, want_frames=True):
    """(bytes[2 n_samples], records[F]) through gj_cancel_dev."""
    return _bytes_and_records(dev, n_samples, gpsjam.excise_frames(n_samples, nfft), gpsjam.CANCEL_DTYPE, want_frames,
                              lambda d_out, d_rec: dev.cancel_dev(d_a, nbytes_a, first_a, d_b, nbytes_b, first_b, n_samples, nfft, d_w,
                                                                  frames_per_set, n_sets, d_thr, d_out, d_rec))


def run_cancel2(dev, caps, firsts, n_samples, nfft, d_w, frames_per_set, n_sets, d_thr, want_frames=True):
    """(bytes[2 n_samples], records[F]) through gj_cancel2_dev.  caps: the three captures."""
    (a, b, c), (fa, fb, fc) = caps, firsts
    return _bytes_and_records(dev, n_samples, gpsjam.excise_frames(n_samples, nfft), gpsjam.CANCEL_DTYPE, want_frames,
                              lambda d_out, d_rec: dev.cancel2_dev(a, a.nbytes, fa, b, b.nbytes, fb, c, c.nbytes, fc, n_samples, nfft, d_w,
                                                                   frames_per_set, n_sets, d_thr, d_out, d_rec))


def run_blank(dev, d_iq, nbytes, first, n_samples, window, guard, threshold, want_blocks=True):
    """(bytes[2 n_samples], records[blocks]) through gj_blank_dev."""
    return _bytes_and_records(dev, n_samples, gpsjam.blank_blocks(n_samples), gpsjam.BLANK_DTYPE, want_blocks,
                              lambda d_out, d_rec: dev.blank_dev(d_iq, nbytes, first, n_samples, window, guard, threshold, d_out, d_rec))


def run_align(dev, d_iq, nbytes, case, d_taps, d_rot, n_out, records=True, out_offset=0):
    """(uint8[2 n_out], ALIGN_DTYPE[blocks] or None) through gj_align_dev; ``out_offset``: bytes by which d_out is moved
    off its 256-byte aligned place."""
    got, rec = _bytes_and_records(dev, n_out, ar.blocks(n_out), gpsjam.ALIGN_DTYPE, records,
                                  lambda d_out, d_rec: dev.align_dev(d_iq, nbytes, case, d_taps, d_rot, n_out, d_out, d_rec), out_offset)
    return got, rec if records else None


def run_subtract(dev, capture, first, n, B, d_rows, n_rows, channels, amps, flags, seed, records=True, out_offset=0, nbytes=None):
    """(uint8[2 n], SUB_DTYPE[blocks] or None) through gj_subtract_dev; ``out_offset`` as in run_align, ``nbytes``: of
    the capture, where it is not ``capture.nbytes``."""
    table = np.array(channels, gpsjam.CORR_CHANNEL_DTYPE)
    amps = np.ascontiguousarray(amps, np.int32)
    assert amps.shape == (len(channels), cr.blocks(n, B), 2)
    d_ch, d_amp = dev.alloc(table.nbytes).upload(table), dev.alloc(amps.nbytes).upload(amps)
    try:
        got, rec = _bytes_and_records(dev, n, sr.blocks(n), gpsjam.SUB_DTYPE, records,
                                      lambda d_out, d_rec: dev.subtract_dev(capture, capture.nbytes if nbytes is None else nbytes, first, n, B,
                                                                            d_rows, n_rows, d_ch, len(channels), d_amp, flags, seed, d_out, d_rec),
                                      out_offset)
        return got, rec if records else None
    finally:
        freed(d_ch, d_amp)


def run_corr(dev, capture, first, n, B, d_rows, n_rows, channels, taps, nbytes=None):
    """int32[n_channels][blocks][n_taps][2] through gj_corr_bank_dev."""
    table = np.array(channels, gpsjam.CORR_CHANNEL_DTYPE)
    out = Guarded(dev, 8 * len(channels) * gpsjam.corr_blocks(n, B) * len(taps))
    d_ch = dev.alloc(table.nbytes).upload(table)
    try:
        dev.corr_bank_dev(capture, capture.nbytes if nbytes is None else nbytes, first, n, B, d_rows, n_rows, d_ch, len(channels), taps, out.ptr)
        out.check_pads("records")
        return out.read(np.int32).reshape(len(channels), -1, len(taps), 2)
    finally:
        freed(out, d_ch)


def run_fine(dev, a, b, first_a, first_b, n, centre, half, want_blocks=True, nbytes_a=None, nbytes_b=None):
    """(total int64[2R+1][2], blocks int32[nb][2R+1][2] or None) through gj_xcorr_fine_dev."""
    nl, nb = 2 * half + 1, gpsjam.fine_blocks(n)
    tot, rec = Guarded(dev, 16 * nl), Guarded(dev, 8 * nl * nb)
    try:
        dev.xcorr_fine_dev(a, a.nbytes if nbytes_a is None else nbytes_a, first_a, b, b.nbytes if nbytes_b is None else nbytes_b,
                           first_b, n, centre, half, tot.ptr, rec.ptr if want_blocks else None)
        _checked((tot, "totals", True), (rec, "records", want_blocks))
        return tot.read(np.int64).reshape(nl, 2), rec.read(np.int32).reshape(nb, nl, 2) if want_blocks else None
    finally:
        freed(tot, rec)


def track_state_records(states):
    rec = np.zeros(len(states), gpsjam.TRACK_STATE_DTYPE)
    for k, s in enumerate(states):
        rec[k] = (tuple(s[:6]), s[6], s[7], s[8], s[9], s[10], tuple(s[11:13]))
    return rec


def run_track(dev, capture, first, n, B, n_epochs, d_rows, n_rows, states, params):
    """(record bytes uint8[n_channels][n_epochs * 56], states after as tuples) through gj_track_dev; the states are read
    and written in place."""
    rec = track_state_records(states)
    out, d_st = Guarded(dev, gpsjam.TRACK_EPOCH_DTYPE.itemsize * len(states) * n_epochs), Guarded(dev, rec.nbytes)
    try:
        d_st.upload(rec)
        dev.track_dev(capture, capture.nbytes, first, n, B, n_epochs, d_rows, n_rows, d_st.ptr, len(states), params, out.ptr)
        _checked((out, "records", True), (d_st, "states", True))
        return out.read().reshape(len(states), -1), tr.states_as_tuples(d_st.read(gpsjam.TRACK_STATE_DTYPE))
    finally:
        freed(out, d_st)


def run_peaks(dev, P, k, guard):
    """(peaks ACQ_PEAK_DTYPE[n_prn][k], floor ACQ_FLOOR_DTYPE[n_prn]) through gj_acq_peaks_dev."""
    P = np.ascontiguousarray(P, np.float64)
    n_prn, n_freq, nsamp = P.shape
    d_power, d_peaks, d_floor = dev.alloc(P.nbytes), Guarded(dev, 16 * n_prn * k), Guarded(dev, 16 * n_prn)
    try:
        d_power.upload(P)
        dev.acq_peaks_dev(d_power, n_prn, n_freq, nsamp, k, guard, d_peaks.ptr, d_floor.ptr)
        _checked((d_peaks, "peaks", True), (d_floor, "floor", True))
        return d_peaks.read(gpsjam.ACQ_PEAK_DTYPE).reshape(n_prn, k), d_floor.read(gpsjam.ACQ_FLOOR_DTYPE)
    finally:
        freed(d_power, d_peaks, d_floor)


# ------------------------------------------------------------------------------------------------ the cross-ambiguity search
def caf_records(raw: bytes):
    return [_ffi.CafResult.from_buffer_copy(raw[k:k + CAF_REC]) for k in range(0, len(raw), CAF_REC)]


class ResidentSlices:
    """Slices resident in HBM with their start words and output buffers for one shape of call."""

    def __init__(self, dev, raws, n, n_pairs, n_bins, starts=None):
        self.dev, self.n, self.n_pairs, self.n_bins = dev, n, n_pairs, n_bins
        self.caps = [dev.capture(r) for r in raws]
        st = np.zeros(len(raws), np.int64) if starts is None else np.asarray(starts, np.int64)
        self.d_starts = dev.alloc(8 * len(raws)).upload(st)
        self.sizes = [(CAF_REC * n_pairs, np.uint8), (4 * n_pairs * n_bins, np.uint8), (4 * n_pairs * n_bins, np.uint8)]
        self.bufs = [dev.alloc(s) for s, _ in self.sizes]
        self.k5 = [dev.alloc(4 * n_pairs) for _ in range(3)]

    def fill(self, byte=SENTINEL):
        for b in self.bufs:
            b.upload(np.full(b.nbytes, byte, np.uint8))

    def read(self):
        self.dev.synchronize()
        return tuple(b.download(np.uint8).tobytes() for b in self.bufs)

    def caf(self, pairs, bin_first, n_bins, bpl=0, bufs=None):
        d_out, d_bl, d_bp = bufs or self.bufs
        self.dev.xcorr_caf_dev(self.caps, [c.nbytes for c in self.caps], self.d_starts, self.n, pairs, bin_first, n_bins, d_out,
                               d_bl, d_bp, bins_per_launch=bpl)

    def lags(self, pairs):
        self.dev.xcorr_lags_dev(self.caps, [c.nbytes for c in self.caps], self.d_starts, self.n, pairs, *self.k5)
        self.dev.synchronize()
        return tuple(b.download(np.uint8, 4 * len(pairs)).tobytes() for b in self.k5)

    def close(self):
        for x in self.caps + self.bufs + self.k5 + [self.d_starts]:
            x.free()


def make_slots(dev, raws, n, flags=None):
    sb = dev.tdoa_slot_bytes(n)
    host = np.zeros(len(raws) * sb, np.uint8)
    for a, r in enumerate(raws):
        head = np.array([0 if flags is None else flags[a], 0], np.int64)
        host[a * sb:a * sb + 16] = head.view(np.uint8)
        host[a * sb + 16:a * sb + 16 + 2 * n] = r[:2 * n]
    return dev.alloc(host.nbytes).upload(host), sb


def as_k5(raw_out: bytes):
    """lag | peak | margin_lag of the records, as the three byte strings K5 writes."""
    rs = caf_records(raw_out)
    return (np.array([r.lag for r in rs], np.int32).tobytes(), np.array([r.peak for r in rs], np.float32).tobytes(),
            np.array([r.margin_lag for r in rs], np.float32).tobytes())
