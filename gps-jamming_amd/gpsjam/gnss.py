"""Host side of the batched GNSS acquisition search (``gj_acq_search_dev``).

The search itself -- carrier wipe-off, 2*nsamp-point FFT, product with the code spectrum, inverse
FFT, |.|^2 accumulation over up to ``intg`` milliseconds, peak test -- runs on the GPU for every PRN
and every Doppler bin at once.  What stays on the host is what the reference receiver computes once
at start-up, in a few microseconds per channel (GpsJammerApp/backend/):

* the spreading code of each PRN         sdrcode.c:102-149 (gencode_L1CA; IS-GPS-200 G1/G2 generators)
* its resampling to the sampling rate    sdrcmn.c:527-579  (rescode, the fixed-point SSE2 form) via sdrinit.c:439
* the Doppler bin list                   sdrinit.c:184,409-412 (+-7 kHz in 200 Hz steps: 71 bins)
* the mixer's phase index per sample     sdrcmn.c:618-659,676-684 (mixcarr, SSE2 form: 16-entry table,
                                         phases accumulated in doubles in ITS order, truncated toward zero)

``AcqSearch.series`` runs the search epoch after epoch over a whole capture (``gj_acq_series_dev``), and
``telemetry`` turns the result into gnssdec-shaped records for the drop-in worker's detector.  The C/N0 there is
the acquisition's 10 log10(maxP / meanP / ctime), not gnssdec's tracking SNR: comparable between the epochs of one
capture, not with gnssdec's numbers.  ``AcqSearch.peaks`` keeps the K largest peaks of every PRN's surface at code phases
a guard apart (``gj_acq_peaks_dev``) and tests each against ``peak_threshold``, a ratio to the floor that needs no
calibration: the second signal of a PRN that is in the air twice is the second peak.

Nothing here is a CPU fallback for the kernels: without the HIP library ``AcqSearch`` cannot be built.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import math
from dataclasses import dataclass
from typing import Iterator, List, Sequence

import numpy as np

CA_LEN = 1023                 # chips per C/A code period (LEN_L1CA)
CA_RATE = 1.023e6             # chips per second (CRATE_L1CA)
ACQ_INTG_L1CA = 10            # sdr.h:59
ACQ_HBAND = 7000.0            # sdr.h:64
ACQ_STEP = 200.0              # sdr.h:65
ACQ_THRESHOLD = 3.0           # sdr.h:66 (ACQTH)

# IS-GPS-200, Table 3-Ia: G2 code delay in chips for PRN 1..32 (the reference's table, sdrcode.c:104-106,
# continues with the SBAS / QZSS entries, which the GPS search does not use)
G2_DELAY = (5, 6, 7, 8, 17, 18, 139, 140, 141, 251, 252, 254, 255, 256, 257, 258, 469, 470, 471, 472,
            473, 474, 509, 512, 513, 514, 515, 516, 859, 860, 861, 862)


def _lfsr(taps: Sequence[int], n: int = CA_LEN) -> np.ndarray:
    """Output (stage 10) of a 10-stage shift register that starts as all ones; feedback = XOR of the
    stages in ``taps`` (1-based), as bits 0/1."""
    reg = 0x3FF                                   # bit k-1 = stage k
    out = np.empty(n, np.uint8)
    for i in range(n):
        out[i] = (reg >> 9) & 1
        fb = 0
        for t in taps:
            fb ^= (reg >> (t - 1)) & 1
        reg = ((reg << 1) | fb) & 0x3FF
    return out


_G1 = _lfsr((3, 10))
_G2 = _lfsr((2, 3, 6, 8, 9, 10))


def ca_code(prn: int) -> np.ndarray:
    """C/A code of GPS PRN 1..32 as int16 chips, +1 for a logical one (the reference's
    ``code[i] = -G1[i] * G2[i - delay]`` with its registers holding -1 for a one, sdrcode.c:129-145)."""
    if not 1 <= prn <= len(G2_DELAY):
        raise ValueError("GPS PRN must be 1..32")
    bits = _G1 ^ np.roll(_G2, G2_DELAY[prn - 1])
    return (2 * bits.astype(np.int16) - 1).astype(np.int16)


def resample_code(code: np.ndarray, nsamp: int, fs: float = 2.048e6, chip_rate: float = CA_RATE) -> np.ndarray:
    """rescode(code, len, coff=0, smax=0, ci=chip_rate/fs, n=nsamp) in the reference's 32-bit fixed-point form
    (sdrcmn.c:541-575): phase = round(k ci 2^nbit) for the first four samples, then += round(4 ci 2^nbit) per
    group of four, wrapped at len 2^nbit, index = phase >> nbit."""
    code = np.asarray(code, np.int16)
    ln = int(code.size)
    ci = (1.0 / fs) * chip_rate                               # sdr->ci = sdr->ti * sdr->crate (sdrinit.c:378,384)
    nbit = 31 - ln.bit_length() - 1                           # for (i = len, nbit = 31; i; i >>= 1, nbit--); nbit -= 1
    scale = 1 << nbit
    x = np.empty(4, np.int64)
    coff = 0.0
    for i in range(4):
        x[i] = int(coff * scale + 0.5)
        coff += ci
    step = int(ci * 4 * scale + 0.5)
    wrap = ln * scale
    out = np.empty(nsamp, np.int16)
    for g in range(0, nsamp, 4):
        x = np.where(x > wrap - 1, x - wrap, x)
        idx = x >> nbit
        out[g:g + 4] = code[idx[:min(4, nsamp - g)]]
        x = x + step
    return out


def doppler_bins(f_if: float = 0.0, hband: float = ACQ_HBAND, step: float = ACQ_STEP, foffset: float = 0.0) -> np.ndarray:
    """acq.freq[i] = f_if + (i - (nfreq-1)/2) step + foffset, nfreq = 2 (hband/step) + 1 (sdrinit.c:184,409-412;
    the reference's integer division of the two #defines is kept)."""
    nfreq = 2 * (int(hband) // int(step)) + 1
    i = np.arange(nfreq)
    return f_if + (i - (nfreq - 1) // 2) * step + foffset


def mixer_phase_table(freqs: Sequence[float], fs: float, m: int) -> np.ndarray:
    """uint8[n_freq][m]: the 4-bit table index mixcarr (SSE2 form, phi0 = 0) uses for sample n of a window of m
    samples at carrier ``freq``.  The reference keeps sixteen phases in doubles -- phi, phi + ps, then phi += 2 ps
    eight times -- adds 16 ps to each after every block of sixteen samples, and converts with cvttpd (truncation
    toward zero) before masking with 15 (sdrcmn.c:636-659,676-684,215-223); the same additions in the same order
    are made here so that every index is the reference's index, also where a phase sits on an integer."""
    if m % 16:
        raise ValueError("window length must be a multiple of 16")
    ti = 1.0 / fs
    out = np.empty((len(freqs), m), np.uint8)
    nblk = m // 16
    for f_idx, freq in enumerate(freqs):
        ps = float(freq) * 16 * ti
        base = np.empty(16, np.float64)
        phi = 0.0                                              # phi0 / DPI * 16 - floor(phi0 / DPI) * 16
        for k in range(0, 16, 2):
            base[k] = phi
            base[k + 1] = phi + ps
            phi += ps * 2
        inc = ps * 16
        ph = np.empty((nblk, 16), np.float64)
        ph[0] = base
        ph[1:] = inc
        ph = np.add.accumulate(ph, axis=0)                     # sequential double additions, block after block
        out[f_idx] = (np.trunc(ph).astype(np.int64) & 15).astype(np.uint8).reshape(-1)
    return out


@dataclass
class AcqResult:
    prn: int
    acquired: bool
    peak_ratio: float
    cn0: float
    code_index: int
    freq_index: int
    doppler_hz: float
    steps: int
    max_power: float
    second_power: float
    mean_power: float


@dataclass
class AcqPeak:
    power: float
    ratio: float             # power / the PRN's floor (``AcqPeaks.mean_power``)
    code_index: int
    freq_index: int
    doppler_hz: float
    significant: bool        # ratio > peak_threshold(steps, n_freq nsamp, pfa)


@dataclass
class AcqPeaks:
    """``AcqSearch.peaks`` of one PRN: its ``k`` largest peaks at code phases at least a guard apart, largest first."""
    prn: int
    steps: int               # integration steps of the surface: all ``intg`` of them
    mean_power: float        # the floor: mean of the cells outside every peak's zone
    peaks: List[AcqPeak]


def _erlang_tail(s: int, x: float) -> float:
    """Q(s, x) = exp(-x) sum_{j < s} x^j / j!: the probability that a sum of ``s`` unit exponentials exceeds x."""
    if x <= 0.0:
        return 1.0
    lx = math.log(x)
    return math.fsum(math.exp(-x + j * lx - math.lgamma(j + 1.0)) for j in range(int(s)))


def peak_threshold(steps: int, n_cells: int, pfa: float = 1e-3) -> float:
    """The ratio gamma of a cell to the floor above which a peak of a noise-only surface of ``n_cells`` cells has
    probability at most ``pfa``: n_cells Q(steps, gamma steps) = pfa, by bisection.

    Under noise a correlation sample is a complex Gaussian, its squared magnitude an exponential, and a cell of the
    surface the sum of ``steps`` of them: divided by the floor (the mean of such cells, ``steps`` in units of one
    exponential's mean) it exceeds gamma with probability Q(steps, gamma steps).  The union bound over all cells makes
    ``pfa`` a bound per PRN; neighbouring Doppler bins are correlated, which only makes it conservative.  At one step
    gamma = ln(n_cells / pfa); 10 steps and 71 x 2048 cells give 3.93."""
    steps, n_cells, pfa = int(steps), int(n_cells), float(pfa)
    if steps < 1 or n_cells < 1 or not pfa > 0.0:
        raise ValueError("steps and n_cells must be at least 1 and pfa positive")
    if n_cells <= pfa:
        return 0.0
    lo, hi = 0.0, 1.0
    while n_cells * _erlang_tail(steps, hi * steps) > pfa:
        lo, hi = hi, 2.0 * hi
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if mid <= lo or mid >= hi:
            break
        if n_cells * _erlang_tail(steps, mid * steps) > pfa:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


@dataclass
class AcqSeries:
    """One search per epoch over a capture: arrays [n_epochs][n_prn] (PRNs in ``prns`` order), and per epoch its
    first sample and that sample's time from the start of the capture."""
    prns: List[int]
    first_sample: np.ndarray     # int64 [n_epochs]
    elapsed_s: np.ndarray        # float64 [n_epochs]
    acquired: np.ndarray         # bool
    cn0: np.ndarray              # float64, dB-Hz (acquisition C/N0)
    peak_ratio: np.ndarray
    code_index: np.ndarray
    freq_index: np.ndarray
    doppler_hz: np.ndarray
    steps: np.ndarray

    @property
    def n_epochs(self) -> int:
        return int(self.first_sample.size)

    def cn0_avg(self) -> np.ndarray:
        """Per epoch the mean C/N0 of the PRNs acquired at that epoch, 0.0 where none is: the worker's
        ``current_cn0_avg = mean(snr of the observations)`` (worker.py:303-306), acquired standing for tracked."""
        n = self.acquired.sum(axis=1)
        tot = np.where(self.acquired, self.cn0, 0.0).sum(axis=1)
        return np.where(n > 0, tot / np.maximum(n, 1), 0.0)


def telemetry(series: AcqSeries) -> Iterator[dict]:
    """One gnssdec-shaped telemetry record per epoch (the fields ``process_incoming_data`` reads, sdrout.c:214-325):
    ``elapsed_time``; ``position`` with ``buffcnt`` = the epoch's first BYTE (the unit of ``jamming_byte_ranges``),
    no fix (nsat 0, lat / lon / hgt 0, so the altitude flag stays off); ``observations`` = prn and snr of each PRN
    acquired at the epoch.  Fed to an unmodified ``GPSAnalysisThread`` they drive its own F1 / F2 state machine."""
    for e in range(series.n_epochs):
        obs = [{"prn": int(p), "snr": float(series.cn0[e, k])}
               for k, p in enumerate(series.prns) if series.acquired[e, k]]
        yield {"elapsed_time": float(series.elapsed_s[e]),
               "position": {"buffcnt": 2 * int(series.first_sample[e]), "lat": 0.0, "lon": 0.0, "hgt": 0.0, "nsat": 0},
               "observations": obs}


class _AcqStruct(C.Structure):
    _fields_ = [("max_power", C.c_double), ("second_power", C.c_double), ("mean_power", C.c_double),
                ("peak_ratio", C.c_double), ("cn0", C.c_double), ("code_index", C.c_int32),
                ("freq_index", C.c_int32), ("steps", C.c_int32), ("acquired", C.c_int32)]


class AcqSearch:
    """Codes and mixer tables resident in HBM; ``search()`` runs one cold search of every PRN over every
    Doppler bin on a resident capture (what 32 channel threads of the reference do one after the other)."""

    def __init__(self, dev, prns: Sequence[int] = tuple(range(1, 33)), fs: float = 2.048e6, f_if: float = 0.0,
                 intg: int = ACQ_INTG_L1CA, threshold: float = ACQ_THRESHOLD, hband: float = ACQ_HBAND,
                 step: float = ACQ_STEP):
        self.dev, self.prns, self.fs, self.intg, self.threshold = dev, list(prns), fs, int(intg), float(threshold)
        self.ctime = CA_LEN / CA_RATE                          # sdr->ctime = clen / crate (sdrinit.c:385)
        self.nsamp = int(fs * self.ctime)                      # sdrinit.c:386
        self.nsampchip = int(self.nsamp / CA_LEN)              # sdrinit.c:387
        self.freqs = doppler_bins(f_if, hband, step)
        codes = np.stack([resample_code(ca_code(p), self.nsamp, fs) for p in self.prns]).astype(np.int16)
        phase = mixer_phase_table(self.freqs, fs, 2 * self.nsamp)
        self.d_codes = dev.alloc(codes.nbytes).upload(codes)
        self.d_phase = dev.alloc(phase.nbytes).upload(phase)
        self.d_out = dev.alloc(C.sizeof(_AcqStruct) * len(self.prns))
        dev.reserve(dev._lib.gj_acq_workspace(dev._ctx, self.nsamp, len(self.freqs), len(self.prns), self.intg, 0))

    def samples_needed(self) -> int:
        return (self.intg + 1) * self.nsamp

    def search_dev(self, d_iq, nbytes: int, first_sample: int = 0, d_power=None):
        """Enqueue one search (no host synchronisation); results land in ``self.d_out``."""
        self._search_dev(d_iq, nbytes, first_sample, d_power, self.threshold, self.d_out)

    def _search_dev(self, d_iq, nbytes, first_sample, d_power, threshold, d_out):
        from . import _ptr
        self.dev._check(self.dev._lib.gj_acq_search_dev(
            self.dev._ctx, _ptr(d_iq), int(nbytes), int(first_sample), self.nsamp, self.intg, self.d_codes.ptr,
            len(self.prns), self.d_phase.ptr, len(self.freqs), self.nsampchip, self.ctime, threshold,
            d_out.ptr, _ptr(d_power) or None))

    def results(self, d_out=None) -> List[AcqResult]:
        raw = (d_out or self.d_out).download(np.uint8, C.sizeof(_AcqStruct) * len(self.prns)).tobytes()
        out = []
        for k, prn in enumerate(self.prns):
            r = _AcqStruct.from_buffer_copy(raw, k * C.sizeof(_AcqStruct))
            out.append(AcqResult(prn, bool(r.acquired), r.peak_ratio, r.cn0, r.code_index, r.freq_index,
                                 float(self.freqs[r.freq_index]), r.steps, r.max_power, r.second_power, r.mean_power))
        return out

    def search(self, capture, first_sample: int = 0, want_power: bool = False):
        """Search a resident capture (gpsjam.Capture / DevBuf / torch tensor with ``nbytes``)."""
        nbytes = getattr(capture, "nbytes", None)
        if nbytes is None:
            nbytes = capture.numel() * capture.element_size()
        cells = len(self.prns) * len(self.freqs) * self.nsamp
        with (self.dev.alloc(8 * cells) if want_power else contextlib.nullcontext()) as d_power:
            self.dev.timer_start()
            self.search_dev(capture, nbytes, first_sample, d_power)
            self.dev.last_kernel_ms = self.dev.timer_stop()
            res = self.results()
            if want_power:
                return res, d_power.download(np.float64).reshape(len(self.prns), len(self.freqs), self.nsamp)
        return res

    def peaks(self, capture, first_sample: int = 0, k: int = 2, guard=None, pfa: float = 1e-3, want_results: bool = False):
        """The ``k`` largest peaks of every PRN's surface at code phases more than ``guard`` samples apart (default
        2 nsampchip: checkacquisition's zone), largest first: a second signal of one PRN -- a counterfeit above the
        authentic one -- is the second peak.  The search runs with a threshold that never passes, so every PRN
        integrates all ``intg`` steps (``self.threshold`` and ``self.d_out`` are left alone); gj_acq_peaks_dev reduces
        the surface where it lies.  A peak is ``significant`` when its ratio to the floor exceeds
        ``peak_threshold(steps, n_freq nsamp, pfa)``.  One ``AcqPeaks`` per PRN; ``want_results``: also the
        ``AcqResult`` records of the same search, whose maximum is peak 0."""
        nbytes = getattr(capture, "nbytes", None)
        if nbytes is None:
            nbytes = capture.numel() * capture.element_size()
        k = int(k)
        guard = 2 * self.nsampchip if guard is None else int(guard)
        n_prn, n_freq = len(self.prns), len(self.freqs)
        from . import ACQ_FLOOR_DTYPE, ACQ_MAX_PEAKS, ACQ_PEAK_DTYPE
        held = min(max(k, 1), ACQ_MAX_PEAKS)           # a k outside 1 .. ACQ_MAX_PEAKS is the library's to refuse
        dev = self.dev
        with dev.alloc(8 * n_prn * n_freq * self.nsamp) as d_power, dev.alloc(C.sizeof(_AcqStruct) * n_prn) as d_out, \
                dev.alloc(16 * n_prn * held) as d_peaks, dev.alloc(16 * n_prn) as d_floor:
            dev.timer_start()
            self._search_dev(capture, nbytes, first_sample, d_power, float("inf"), d_out)
            dev.acq_peaks_dev(d_power, n_prn, n_freq, self.nsamp, k, guard, d_peaks, d_floor)
            dev.last_kernel_ms = dev.timer_stop()
            results = self.results(d_out)
            pk = d_peaks.download(ACQ_PEAK_DTYPE, n_prn * k).reshape(n_prn, k)
            fl = d_floor.download(ACQ_FLOOR_DTYPE, n_prn)
        out, gamma = [], {}
        for p, r in enumerate(results):
            if r.steps not in gamma:
                gamma[r.steps] = peak_threshold(r.steps, n_freq * self.nsamp, pfa)
            mean = float(fl["mean_power"][p])
            peaks = []
            for rec in pk[p]:
                ratio = float(rec["power"]) / mean if mean > 0.0 else float("inf")
                peaks.append(AcqPeak(float(rec["power"]), ratio, int(rec["code_index"]), int(rec["freq_index"]),
                                     float(self.freqs[int(rec["freq_index"])]), ratio > gamma[r.steps]))
            out.append(AcqPeaks(r.prn, r.steps, mean, peaks))
        return (out, results) if want_results else out

    def series_workspace(self, n_epochs: int, epochs_per_launch: int = 0) -> int:
        return int(self.dev._lib.gj_acq_series_workspace(self.dev._ctx, self.nsamp, len(self.freqs), len(self.prns),
                                                         self.intg, int(n_epochs), int(epochs_per_launch)))

    def series_dev(self, d_iq, nbytes: int, first_sample: int, stride_samples: int, n_epochs: int, d_out,
                   epochs_per_launch: int = 0):
        """Enqueue a series (no host synchronisation); d_out receives gj_acq_result[n_epochs][n_prn]."""
        from . import _ptr
        self.dev._check(self.dev._lib.gj_acq_series_dev(
            self.dev._ctx, _ptr(d_iq), int(nbytes), int(first_sample), int(stride_samples), int(n_epochs),
            int(epochs_per_launch), self.nsamp, self.intg, self.d_codes.ptr, len(self.prns), self.d_phase.ptr,
            len(self.freqs), self.nsampchip, self.ctime, self.threshold, _ptr(d_out)))

    def series(self, capture, first_sample: int = 0, stride_samples=None, n_epochs=None,
               epochs_per_launch: int = 0) -> AcqSeries:
        """Search a resident capture at first_sample + e * stride_samples, e = 0 .. n_epochs-1.  Default stride: 0.1 s
        of samples (gnssdec's telemetry cadence); default n_epochs: as many as fit in the capture."""
        nbytes = getattr(capture, "nbytes", None)
        if nbytes is None:
            nbytes = capture.numel() * capture.element_size()
        if stride_samples is None:
            stride_samples = int(round(0.1 * self.fs))
        first_sample, stride_samples = int(first_sample), int(stride_samples)
        if n_epochs is None:
            room = nbytes // 2 - first_sample - self.samples_needed()
            if room < 0:
                raise ValueError("the capture does not hold one search window after first_sample")
            n_epochs = 1 if stride_samples == 0 else room // stride_samples + 1
        n_epochs = int(n_epochs)
        if n_epochs >= 1:
            self.dev.reserve(self.series_workspace(n_epochs, epochs_per_launch))
        rec = C.sizeof(_AcqStruct)
        with self.dev.alloc(rec * max(n_epochs, 1) * len(self.prns)) as d_out:
            self.dev.timer_start()
            self.series_dev(capture, nbytes, first_sample, stride_samples, n_epochs, d_out, epochs_per_launch)
            self.dev.last_kernel_ms = self.dev.timer_stop()
            raw = d_out.download(np.uint8, rec * n_epochs * len(self.prns))
        r = np.frombuffer(raw.tobytes(), dtype=np.dtype([(n, np.float64 if t is C.c_double else np.int32)
                                                         for n, t in _AcqStruct._fields_]))
        r = r.reshape(n_epochs, len(self.prns))
        first = first_sample + stride_samples * np.arange(n_epochs, dtype=np.int64)
        return AcqSeries(prns=list(self.prns), first_sample=first, elapsed_s=first / self.fs,
                         acquired=r["acquired"] != 0, cn0=r["cn0"].copy(), peak_ratio=r["peak_ratio"].copy(),
                         code_index=r["code_index"].copy(), freq_index=r["freq_index"].copy(),
                         doppler_hz=self.freqs[r["freq_index"]], steps=r["steps"].copy())

    def close(self):
        for b in (self.d_codes, self.d_phase, self.d_out):
            b.free()
