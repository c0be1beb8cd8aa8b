"""Captures, cases and measured constants of the acquisition search's edge tests.  Not a test module:
tests/test_acq_edges_host.py (CPU: pins the restatement, measures the complex64 oracle's error, asserts the conditions
below) and tests/acq_edges/test_acq_gpu.py (GPU) import it.

Every capture is (intg + 1) nsamp samples plus a few dozen (family (g): the lengths of tests/test_acq_gpu.py), built once
from a fixed seed and returned read-only; every reference is tests/acq_restatement.py's exact power, computed once per
case (lru_cache) and shared.

Seeds, amplitudes and thresholds were chosen ON THE CPU so that every case of families (a) (b) (c) (e) (g) is CLEAR at
every step up to the deciding one (acq_restatement.is_clear: the best cell beats every cell outside the tie set by 1e-3
and the peak ratio stays 1e-2 away from the threshold).  tests/test_acq_edges_host.py asserts it for every case and
prints the smallest margins.  Two exceptions: code index 0 of family (a), whose ratio is 1 by construction, and the PRNs
of EXISTING_NOT_CLEAR in family (g), whose captures are tests/test_acq_gpu.py's and not this module's to choose.
"""
import ctypes as C
import functools
import math

import numpy as np

import acq_restatement as ar
from gpsjam import gnss

RATES = (2.048e6, 1.024e6, 0.512e6)               # nsamp 2048 / 1024 / 512, nsampchip 2 / 1 / 0
TAIL = 40                                         # "a few dozen" samples behind the last window

# The complex64 oracle (oracle.gpsjam_oracle.acq_search: scipy's pocketfft in complex64, like FFTW's float build)
# against exact power, as a share of the (PRN, step) array's maximum; measured by tests/test_acq_edges_host.py, which
# prints the figure per family and asserts it stays under the constant.  Never measured from the GPU.
#   noise      Gaussian-noise captures, families (a) (b) (c) (e) (g)
#   saturated  family (d); largest on the Nyquist pattern, whose maximum is small against its cells' common level
E64_MEASURED = {"noise": 4.0e-7, "saturated": 2.7e-6}
GATE = {k: 8.0 * v for k, v in E64_MEASURED.items()}   # a second correct complex64 chain: other butterfly order, other table rounding
OLD_GATE = 2e-4                                        # tests/test_acq_gpu.py's; no gate here may exceed it
TIE_SET_CAP = 16                                       # family (d): cells of n_freq nsamp a tie set may hold


def readonly(a):
    a.setflags(write=False)
    return a


def gps_like(n, sats, fs=2.048e6, noise_sigma=12.0, seed=4):
    """tests/test_acq_gpu.py's generator at any rate: uint8 I/Q of C/A signals (prn, doppler_hz, code_delay_samples,
    amplitude) + Gaussian noise, + 128."""
    rng = np.random.default_rng(seed)
    k = np.arange(n)
    z = rng.normal(0, noise_sigma, n) + 1j * rng.normal(0, noise_sigma, n)
    for prn, dop, delay, amp in sats:
        chip = ((k - delay) * 1.023e6 / fs) % 1023
        z += amp * gnss.ca_code(prn)[chip.astype(np.int64)] * np.exp(-2j * np.pi * dop * (k / fs))
    iq = np.empty(2 * n, np.float64)
    iq[0::2], iq[1::2] = z.real, z.imag
    return readonly((np.clip(np.round(iq), -128, 127) + 128).astype(np.uint8))


def nsamp_of(fs):
    return ar.geometry(fs)[0]


class Case:
    """One search: capture, first sample and the AcqSearch arguments.  n_freq < the table's bin count runs the search on
    the first n_freq bins of the table (the phase table is [n_freq][m], so its first rows are a table of their own)."""

    def __init__(self, name, raw, fs, prns, first=0, intg=3, hband=7000.0, threshold=3.0, nsampchip=None, n_freq=None,
                 family="noise"):
        self.name, self.raw, self.fs, self.prns, self.first, self.intg = name, raw, fs, list(prns), first, intg
        self.hband, self.threshold, self.family = hband, threshold, family
        self.nsamp, chip, self.ctime = ar.geometry(fs)
        self.nsampchip = chip if nsampchip is None else nsampchip
        bins = 2 * (int(hband) // 200) + 1
        self.n_freq = bins if n_freq is None else n_freq
        self._at = {}
        assert 1 <= self.n_freq <= bins
        assert 2 * (first + (intg + 1) * self.nsamp) <= raw.size

    def __repr__(self):
        return self.name

    def at(self, first):
        """The same search at another first sample (one object per first sample, so its reference is computed once)."""
        if first not in self._at:
            self._at[first] = Case(f"{self.name}@{first}", self.raw, self.fs, self.prns, first, self.intg, self.hband,
                                   self.threshold, self.nsampchip, self.n_freq, self.family)
        return self._at[first]

    @property
    def gate(self):
        return GATE[self.family]


@functools.lru_cache(maxsize=None)
def _reference(case):
    uniq = sorted(set(case.prns))
    Pint = ar.exact_power_prns(case.raw, case.first, uniq, case.fs, case.intg, case.hband)[:, :, :case.n_freq]
    out = {}
    for k, prn in enumerate(uniq):
        steps = ar.search(case.raw, case.first, prn, case.fs, case.intg, case.hband, case.threshold, case.nsampchip,
                          Pint=Pint[k])
        for s in steps:
            readonly(s["P"])
        out[prn] = steps
    return out


def reference(case):
    """{prn: [step entries of acq_restatement.search]}, computed once per case.  Read-only."""
    return _reference(case)


# ------------------------------------------------------------------------------- (g) the inputs of tests/test_acq_gpu.py
@functools.lru_cache(maxsize=None)
def existing_cases():
    """The captures of tests/test_acq_gpu.py by its recipes, with its PRN lists and first samples."""
    out = [Case("g:2048 three satellites",
                gps_like(14 * 2048, [(3, 1400.0, 517, 9.0), (17, -3000.0, 1201, 1.5), (25, 5230.0, 88, 3.0)]),
                2.048e6, [3, 8, 17, 25], first=1000, intg=10),
           Case("g:2048 all 32",
                gps_like(12 * 2048, [(p, 200.0 * ((7 * p) % 60 - 30), (97 * p) % 2048, 6.0) for p in (1, 9, 14, 22, 31)],
                         noise_sigma=10.0, seed=9),
                2.048e6, range(1, 33), first=0, intg=10)]
    for fs in (1.024e6, 0.512e6):
        nsamp = int(fs * 1e-3)
        raw = gps_like(13 * nsamp, [(4, 1800.0, nsamp // 3, 7.0), (20, -4400.0, nsamp - 9, 2.0)], fs=fs, noise_sigma=10.0,
                       seed=int(fs) % 97)
        out.append(Case(f"g:{nsamp} two satellites", raw, fs, [4, 9, 20], first=17, intg=10))
    return tuple(out)


# tests/test_acq_gpu.py's captures were not made for clear margins: these PRNs have, at some step, two cells within 1e-3
# of each other or (PRN 17 of the first capture) a ratio within 1e-2 of the threshold.  tests/test_acq_edges_host.py asserts
# that the lists are exactly the PRNs that are not clear.  Their power is held to the gate; their records are not compared.
EXISTING_NOT_CLEAR = {"g:2048 three satellites": [8, 17], "g:2048 all 32": [7, 10, 15, 21, 27, 29],
                      "g:1024 two satellites": [], "g:512 two satellites": [20]}


# ------------------------------------------------------------------------------- (a) the zone and the seed
ZONE_PRN, ZONE_DOPPLER, ZONE_DELAY, ZONE_AMP = 3, 400.0, 40, 9.0
ZONE_EPOCHS = 13                                  # stride 1 from delay - 6: code index 6 .. 0, nsamp - 1 .. nsamp - 6
ZONE_SEED = {2048: 21, 1024: 22, 512: 23}
ZONE_CHIPS_2048 = (1, 100, 511)                   # nsampchip overrides at 2048; 511 leaves cnt = 3


@functools.lru_cache(maxsize=None)
def zone_case(fs, nsampchip=None):
    """Epoch 0 of the stride-1 series; epoch e is zone_case(...).at(first + e)."""
    nsamp = nsamp_of(fs)
    n = ZONE_DELAY - 6 + ZONE_EPOCHS + 4 * nsamp + TAIL
    raw = gps_like(n, [(ZONE_PRN, ZONE_DOPPLER, ZONE_DELAY, ZONE_AMP)], fs=fs, seed=ZONE_SEED[nsamp])
    return Case(f"a:{nsamp} chip {nsampchip}", raw, fs, [ZONE_PRN], first=ZONE_DELAY - 6, intg=3, hband=1000.0,
                nsampchip=nsampchip)


def zone_cases():
    return [zone_case(fs) for fs in RATES] + [zone_case(2.048e6, c) for c in ZONE_CHIPS_2048]


def zone_code_index(case, epoch):
    return (6 - epoch) % case.nsamp


# ------------------------------------------------------------------------------- (b) many steps
STEPS_STRONG, STEPS_ABSENT, STEPS_WEAK = 3, 8, 17       # PRNs: 9 LSB, not in the capture, 1.5 LSB
STEPS_SEED = {2048: 31, 1024: 31, 512: 49}
STEPS_WEAK_AMP = {2048: 1.5, 1024: 1.5, 512: 2.5}
# 512 samples: the weak satellite's ratio first passes STEPS_THRESHOLD at step STEPS_WEAK_PASSES, and the running
# maximum of its earlier steps stays under it (asserted by the host test)
STEPS_THRESHOLD = 2.97
STEPS_WEAK_PASSES = 31


@functools.lru_cache(maxsize=None)
def steps_capture(fs, most):
    nsamp = nsamp_of(fs)
    sats = [(STEPS_STRONG, 200.0, nsamp // 3, 9.0), (STEPS_WEAK, -200.0, nsamp // 2 + 5, STEPS_WEAK_AMP[nsamp])]
    return gps_like((most + 1) * nsamp + TAIL, sats, fs=fs, seed=STEPS_SEED[nsamp])


@functools.lru_cache(maxsize=None)
def steps_cases():
    prns = [STEPS_STRONG, STEPS_ABSENT, STEPS_WEAK]
    out = [Case(f"b:512 intg {intg}", steps_capture(0.512e6, 64), 0.512e6, prns, first=3, intg=intg, hband=600.0,
                threshold=STEPS_THRESHOLD) for intg in (1, 16, 17, 64)]
    out += [Case(f"b:{nsamp_of(fs)} intg 17", steps_capture(fs, 17), fs, prns, first=3, intg=17, hband=200.0)
            for fs in (1.024e6, 2.048e6)]
    return tuple(out)


# ------------------------------------------------------------------------------- (c) ragged shapes
RAGGED_SEED = {2048: 43, 1024: 41, 512: 41}
RAGGED_PRNS = {"one": [3], "three": [3, 7, 20],
               "forty with repeats": [(3, 7, 20, 11, 29)[(i * i + i // 7) % 5] for i in range(40)]}
RAGGED_N_FREQ = {512: (1, 2, 5, 9), 1024: (1, 2, 5, 9), 2048: (1, 9)}


@functools.lru_cache(maxsize=None)
def ragged_capture(fs):
    nsamp = nsamp_of(fs)
    sats = [(3, -800.0, nsamp // 5, 9.0), (7, 0.0, nsamp - 3, 9.0)]      # bin 0 of the 9-bin table; the one bin of hband 0
    return gps_like(4 * nsamp + TAIL + 9, sats, fs=fs, seed=RAGGED_SEED[nsamp])


@functools.lru_cache(maxsize=None)
def ragged_cases():
    """n_freq = 1 is hband 0 (the single bin at 0 Hz); 2, 5 and 9 are the first bins of the 9-bin table of hband 800."""
    out = []
    for fs in RATES:
        nsamp = nsamp_of(fs)
        for n_freq in RAGGED_N_FREQ[nsamp]:
            for label, prns in RAGGED_PRNS.items():
                out.append(Case(f"c:{nsamp} bins {n_freq} prns {label}", ragged_capture(fs), fs, prns, first=9, intg=3,
                                hband=0.0 if n_freq == 1 else 800.0, n_freq=n_freq))
    return tuple(out)


# ------------------------------------------------------------------------------- (d) degenerate and saturated captures
EXTREME_NAMES = ("constant 128", "constant 128/127", "constant 0", "constant 255", "nyquist full scale", "uniform bytes",
                 "quiet then rail to rail")
EXTREME_RATES = (2.048e6, 0.512e6)
EXTREME_PRNS = [3, 22]
EXTREME_SEED = 11


def _interleave(i, q):
    raw = np.empty(2 * i.size, np.uint8)
    raw[0::2], raw[1::2] = i, q
    return raw


@functools.lru_cache(maxsize=None)
def extreme_capture(name, n):
    """The recipes of tests/extremes_inputs.py at n samples."""
    t = np.arange(n)
    if name == "constant 128":
        raw = np.full(2 * n, 128, np.uint8)
    elif name == "constant 128/127":
        raw = _interleave(np.full(n, 128, np.uint8), np.full(n, 127, np.uint8))
    elif name == "constant 0":
        raw = np.zeros(2 * n, np.uint8)
    elif name == "constant 255":
        raw = np.full(2 * n, 255, np.uint8)
    elif name == "nyquist full scale":
        raw = _interleave(np.where(t & 1, 255, 0).astype(np.uint8), np.where(t & 1, 0, 255).astype(np.uint8))
    elif name == "uniform bytes":
        raw = np.random.RandomState(EXTREME_SEED).randint(0, 256, 2 * n).astype(np.uint8)
    elif name == "quiet then rail to rail":
        rng = np.random.RandomState(EXTREME_SEED + 2)
        raw = (np.clip(np.rint(rng.normal(0, 2.0, 2 * n)), -128, 127) + 128).astype(np.uint8)
        rail = 3 * n // 4
        raw[2 * rail:] = np.where(rng.randint(0, 2, 2 * (n - rail)) == 1, 255, 0)
    else:
        raise ValueError(name)
    return readonly(raw)


@functools.lru_cache(maxsize=None)
def extreme_cases():
    out = []
    for fs in EXTREME_RATES:
        nsamp = nsamp_of(fs)
        for name in EXTREME_NAMES:
            out.append(Case(f"d:{nsamp} {name}", extreme_capture(name, 4 * nsamp + TAIL + 1), fs, EXTREME_PRNS, first=1,
                            intg=3, family="saturated"))
    return tuple(out)


# ------------------------------------------------------------------------------- (e) the race
RACE_SEED = {2048: 53, 1024: 51, 512: 55}
RACE_INTG = 2
RACE_RUNS = 16


@functools.lru_cache(maxsize=None)
def race_case(fs):
    nsamp = nsamp_of(fs)
    raw = gps_like((RACE_INTG + 1) * nsamp + TAIL + 5, [], fs=fs, seed=RACE_SEED[nsamp])
    return Case(f"e:{nsamp} noise only", raw, fs, range(1, 33), first=5, intg=RACE_INTG)


# ------------------------------------------------------------------------------- (f) past byte 2^32
BIG = 2 ** 32 + 2 ** 20                           # one allocation, never filled
FAR_SAMPLE = 2 ** 31                              # the capture is uploaded at byte 2^32 ...
FAR_FIRST = FAR_SAMPLE + 1                        # ... and searched from its sample 1: byte 2^32 + 2
FAR_STRIDE = 1500


REC = C.sizeof(gnss._AcqStruct)


RECORD = np.dtype([(n, np.float64 if t is C.c_double else np.int32) for n, t in gnss._AcqStruct._fields_])


assert RECORD.itemsize == REC


def records(raw):
    return np.frombuffer(raw, RECORD)


def check_record(got, want, case, what):
    """One record against the deciding step of the restatement (a clear case)."""
    gate = case.gate
    assert (int(got["code_index"]), int(got["freq_index"]), int(got["steps"]), bool(got["acquired"])) == \
           (want["codei"], want["freqi"], want["steps"], want["acquired"]), (what, got, want["peakr"])
    check_values(got, want, case, what)
    r = want["peakr"]
    assert abs(got["peak_ratio"] - r) <= gate * (1.0 + r) * r, (what, got["peak_ratio"], r)
    assert abs(got["cn0"] - want["cn0"]) <= 10.0 / math.log(10.0) * gate * (1.0 + want["maxP"] / want["meanP"]), (what, got["cn0"], want["cn0"])


def check_values(got, want, case, what):
    tol = case.gate * want["maxP"]
    for field, key in (("max_power", "maxP"), ("second_power", "maxP2"), ("mean_power", "meanP")):
        assert abs(got[field] - want[key]) <= tol, (what, field, got[field], want[key], tol)


def check_power(P, want, case, what):
    err = float(np.max(np.abs(P - want["P"])) / want["P"].max())
    assert err <= case.gate, (what, err, case.gate)
    return err


def series_like(n, sats, fs=2.048e6, noise_sigma=12.0, seed=4, t0=0, burst=None):
    """tests/acq_series' generator, writable: uint8 I/Q of samples t0 .. t0+n: C/A signals (prn, doppler_hz,
    code_delay_samples, amplitude) + Gaussian noise, + 128.  burst = (first, end, sigma): extra noise on those samples."""
    rng = np.random.default_rng(seed)
    k = np.arange(t0, t0 + n)
    z = rng.normal(0, noise_sigma, n) + 1j * rng.normal(0, noise_sigma, n)
    if burst is not None:
        lo, hi, sig = burst
        m = (k >= lo) & (k < hi)
        z[m] += rng.normal(0, sig, int(m.sum())) + 1j * rng.normal(0, sig, int(m.sum()))
    for prn, dop, delay, amp in sats:
        chip = ((k - delay) * 1.023e6 / fs) % 1023
        z += amp * gnss.ca_code(prn)[chip.astype(np.int64)] * np.exp(-2j * np.pi * dop * (k / fs))
    iq = np.empty(2 * n, np.float64)
    iq[0::2], iq[1::2] = z.real, z.imag
    return (np.clip(np.round(iq), -128, 127) + 128).astype(np.uint8)
