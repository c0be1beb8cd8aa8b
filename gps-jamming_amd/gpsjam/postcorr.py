"""From the acquisition to post-correlation observables: Doppler to about a hertz, a tracking-style C/N0, the code error
and the complex prompt series of every acquired PRN, open loop.

The acquisition search (``gnss.AcqSearch``, k_acq.hip) knows a satellite to a 200 Hz Doppler bin and one sample of code
phase, and no carrier phase.  The reference goes on with closed loops (DLL / PLL, sdrtrk.c) around its correlator
(sdrcmn.c:707-740); those loops are sequential per millisecond.  The correlator is not: with the code phase and the
Doppler of the acquisition, and the code rate tied to the Doppler, every block of every channel is independent, and
``Device.corr_bank`` (gj_corr_bank_dev, k_corr.hip) correlates a whole capture in one launch, in exact integers.  What
is left for the host is float arithmetic on a hundred complex numbers per PRN, and lives here.

Nothing here is a CPU fallback for the kernels: the prompts come from the library.
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Sequence

import numpy as np

from . import _ffi, gnss

L1_HZ = 1575.42e6              # carrier the code rate is tied to (FREQ1)
TAPS = (0, -1, 1)              # prompt, late, early: whole samples (gj_corr_bank_dev's taps shift the code by t + d)
_PERIOD = gnss.CA_LEN << 32


class Channel(NamedTuple):
    """The fixed-point fields of gj_corr_channel (include/gpsjam.h), in its order."""
    code_phase: int
    code_step: int
    carr_phase: int
    carr_step: int
    code_row: int
    reserved: int = 0


def channel(code_row: int, code_phase_chips: float, doppler_hz: float, fs: float, carr_cycles: float = 0.0) -> Channel:
    """One channel: the code at ``code_phase_chips`` chips (mod 1023) at the range's first sample, its rate tied to
    the Doppler, code_step = round(CA_RATE (1 + doppler / L1) / fs 2^32); the carrier at ``carr_cycles`` cycles there,
    carr_step = round(doppler / fs 2^32) mod 2^32.  The sign is the reference mixer's: a capture that holds
    code exp(-2j pi dop t) peaks at doppler = +dop."""
    code_phase = int(round((float(code_phase_chips) % gnss.CA_LEN) * 2.0 ** 32)) % _PERIOD
    code_step = int(round(gnss.CA_RATE * (1.0 + float(doppler_hz) / L1_HZ) / float(fs) * 2.0 ** 32))
    carr_phase = int(round((float(carr_cycles) % 1.0) * 2.0 ** 32)) % 2 ** 32
    carr_step = int(round(float(doppler_hz) / float(fs) * 2.0 ** 32)) % 2 ** 32
    return Channel(code_phase, code_step, carr_phase, carr_step, int(code_row), 0)


def advance(ch: Channel, samples: int) -> Channel:
    """The same channel ``samples`` samples later (or earlier): exact integer arithmetic."""
    return ch._replace(code_phase=(ch.code_phase + int(samples) * ch.code_step) % _PERIOD,
                       carr_phase=(ch.carr_phase + int(samples) * ch.carr_step) % 2 ** 32)


def codes(prns: Sequence[int]) -> np.ndarray:
    """int16[len(prns)][1023]: the unresampled C/A codes, one row per PRN (the bank resamples them itself)."""
    return np.stack([gnss.ca_code(int(p)) for p in prns]).astype(np.int16)


def channels_from_acq(search, results, first_sample: int, at_sample: Optional[int] = None, doppler_hz=None):
    """(prns, channels): one channel per acquired PRN of ``results`` (``search.search(capture, first_sample)``), code row
    k for the k-th of them.  The acquisition's ``code_index`` says that the code starts ``code_index`` samples after
    ``first_sample``: the phase there is -code_index code_step, exactly.  ``at_sample``: the sample the bank's range
    starts at (default ``first_sample``); ``doppler_hz``: a Doppler per acquired PRN to use instead of the bin's."""
    at_sample = int(first_sample) if at_sample is None else int(at_sample)
    prns, out = [], []
    for r in results:
        if not r.acquired:
            continue
        dop = float(r.doppler_hz) if doppler_hz is None else float(doppler_hz[len(out)])
        ch = channel(len(out), 0.0, dop, search.fs)
        out.append(advance(ch, at_sample - int(first_sample) - int(r.code_index)))
        prns.append(int(r.prn))
    return prns, out


def residual_doppler(prompts, block_s: float, pad: int = 16) -> float:
    """Hz by which the Doppler the prompts were made with falls short of the signal's.  Squaring the prompts removes
    the navigation bits and doubles the rotation; the peak of the zero-padded FFT of the squares, refined by a parabola
    through the log magnitudes, sits at MINUS twice the residual (the mixer turns by +doppler, the signal by -doppler).
    Unambiguous within +-1 / (4 block_s): +-250 Hz for 1 ms blocks, the acquisition leaves +-100."""
    p = np.asarray(prompts, np.complex128)
    if p.size < 2 or not np.any(p):
        return 0.0
    n = 1 << int(np.ceil(np.log2(p.size * int(pad))))
    spec = np.abs(np.fft.fft(p * p, n))
    k = int(np.argmax(spec))
    a, b, c = (np.log(max(spec[(k + d) % n], 1e-300)) for d in (-1, 0, 1))
    den = a - 2.0 * b + c
    delta = 0.5 * (a - c) / den if den < 0 else 0.0
    f = (k + delta) / n
    if f >= 0.5:
        f -= 1.0
    return -0.5 * f / float(block_s)


def cn0(prompts, block_s: float) -> float:
    """C/N0 in dB-Hz by the second and fourth moments of the prompts (no bit decisions, no phase lock):
    Pd = sqrt(2 M2^2 - M4), Pn = M2 - Pd, C/N0 = Pd / Pn / block_s.  -inf where the moments leave no signal."""
    m = np.abs(np.asarray(prompts, np.complex128)) ** 2
    if m.size == 0:
        return float("-inf")
    m2, m4 = float(m.mean()), float((m * m).mean())
    d = 2.0 * m2 * m2 - m4
    if d <= 0.0:
        return float("-inf")
    pd = np.sqrt(d)
    pn = m2 - pd
    if pn <= 0.0:
        return float("inf")
    return float(10.0 * np.log10(pd / pn / float(block_s)))


def code_error(E, P, L) -> float:
    """The reference's discriminator (|E| - |L|) / (|E| + |L|) (sdrtrk.c:99-100) on the mean magnitudes of the early and
    late series; ``P`` is taken for the signature's sake.  Positive: the replica is late."""
    e, l = float(np.mean(np.abs(E))), float(np.mean(np.abs(L)))
    return (e - l) / (e + l) if e + l > 0.0 else 0.0


def code_shift(error: float, ch: Channel) -> float:
    """Chips by which a replica with the discriminator value ``error`` at taps one sample either side is late.  With the
    ideal triangle R(x) = 1 - |x| and a tap spacing of d chips (code_step / 2^32), an offset x inside the spacing gives
    E - L = 2 x and E + L = 2 (1 - d): x = error (1 - d).  0 where the taps are a chip or more apart."""
    d = ch.code_step / 2.0 ** 32
    return float(error) * (1.0 - d) if d < 1.0 else 0.0


class Observation(NamedTuple):
    prn: int
    doppler_hz: float        # the bin's Doppler plus the residual
    cn0_dbhz: float
    code_error: float        # what is left behind the code shift
    code_shift_chips: float  # by which the acquisition's code phase was advanced for the second bank
    prompts: np.ndarray      # complex128[periods]: one per whole code period
    channel: Channel         # what the prompts were made with, at first_sample
    first_block: int         # bank block at which the first of ``prompts`` starts: where this PRN's code period does


SUB_BLOCKS = 8                 # bank blocks per code period


def block_samples(search) -> int:
    """An eighth of a code period in samples, down to the bank's multiple of 16 (256 at 2.048 MS/s).  A navigation bit
    flips where a code period ends, which is anywhere inside a block cut at the range's start: a block that straddles
    a flip loses its sum, and at 15 dB and more per prompt a few such blocks in a hundred are what the moments see.  So
    the bank runs on eighths and ``periods`` puts eight of them together from where THIS PRN's period starts."""
    return max(16, int(search.nsamp) // SUB_BLOCKS // 16 * 16)


def first_block(code_index: int, B: int) -> int:
    """The bank block nearest to the start of a code period that begins ``code_index`` samples into the range."""
    return int(round(int(code_index) / float(B))) % SUB_BLOCKS


def periods(series, start: int) -> np.ndarray:
    """complex128[periods]: the sums of SUB_BLOCKS consecutive whole blocks of one channel's series from block ``start``."""
    z = np.asarray(series, np.complex128)
    m = max(0, (z.size - int(start)) // SUB_BLOCKS)
    return z[int(start):int(start) + m * SUB_BLOCKS].reshape(m, SUB_BLOCKS).sum(axis=1)


def tap_periods(bank, tap: int, starts) -> List[np.ndarray]:
    """``periods`` of every channel of a ``CorrBank`` at one tap, without the ragged last block."""
    z = bank.tap(tap)[:, :bank.n_samples // bank.block_samples]
    return [periods(row, s) for row, s in zip(z, starts)]


MIXER_GAIN = 1042.5            # the mean of C[i]^2 + S[i]^2 over GJ_CORR_COS_TABLE
SUB_FRAC = _ffi.GJ_SUB_FRAC    # fraction bits of an amplitude of gj_subtract_dev


def amplitudes(bank, starts, tap: int = 0) -> np.ndarray:
    """int32[n_channels][n_blocks][2]: the amplitudes (aI, aQ) with which ``Device.subtract`` takes out what a
    ``CorrBank`` of the same channels, range and block size saw at ``tap``.  Per channel the least-squares amplitude of
    the bank's own template, held constant over each code period of that PRN: a period is SUB_BLOCKS blocks from block
    ``starts[ch]`` (``Observation.first_block``) on, the blocks in front of the first period are a group of their own,
    so are the blocks behind the last whole one, and the ragged last block counts the samples it holds.  For a group

        alpha = sum of its prompts / (its samples * MIXER_GAIN),    a = round(alpha * 2^SUB_FRAC)

    A sample of the replica alpha c (C - jS) adds alpha (C^2 + S^2) to the prompt; MIXER_GAIN = 1042.5 is the mean of
    C^2 + S^2 over the 16 table entries (1024 at the multiples of 4, 1044 and 1058 elsewhere: every entry, and so the
    mean along any carrier step, a still carrier included, is within 1.8 % of 1042.5).  The sum is over the period, not per block: an eighth of
    a period carries 9 dB less SNR, and amplitudes made per eighth take more noise out with the signal."""
    z = bank.tap(tap)
    n_ch, n_blocks = z.shape
    B, n = int(bank.block_samples), int(bank.n_samples)
    samples = np.full(n_blocks, B, np.float64)
    if n_blocks:
        samples[-1] = n - (n_blocks - 1) * B
    out = np.zeros((n_ch, n_blocks, 2), np.int32)
    for k in range(n_ch):
        s = int(starts[k]) % SUB_BLOCKS
        edges = ([0] if s else []) + list(range(s, n_blocks, SUB_BLOCKS)) + [n_blocks]
        for lo, hi in zip(edges, edges[1:]):
            if hi <= lo:
                continue
            alpha = z[k, lo:hi].sum() / (samples[lo:hi].sum() * MIXER_GAIN) * 2.0 ** SUB_FRAC
            out[k, lo:hi, 0], out[k, lo:hi, 1] = int(round(alpha.real)), int(round(alpha.imag))
    return out


def observe(dev, capture, search, first_sample: int = 0, duration_s: float = 0.1, results=None) -> List[Observation]:
    """The chain on a resident capture (or host bytes): acquisition at ``first_sample``; a bank at each bin's Doppler
    over ``duration_s``; the residual Doppler of each PRN and, from the early and late taps, the fraction of a sample by
    which the acquisition's code phase is off (``code_shift``); a bank again at the refined Doppler and code phase.
    One ``Observation`` per acquired PRN, in the search's order; its prompts are one per code period of that PRN.
    ``results``: ``gnss.AcqResult`` records to use in place of ``search.search`` -- the candidates of a K-peak search,
    say, in which a PRN may stand twice; at most as many acquired ones as one bank takes channels."""
    with dev._resident(capture) as cap:
        results = search.search(cap, first_sample) if results is None else list(results)
        prns, chans = channels_from_acq(search, results, first_sample)
        if not prns:
            return []
        B = block_samples(search)
        n = min(int(round(duration_s * search.fs)), cap.nsamples - int(first_sample))
        rows, period_s = codes(prns), SUB_BLOCKS * B / float(search.fs)
        acquired = [r for r in results if r.acquired]
        starts = [first_block(r.code_index, B) for r in acquired]
        first = dev.corr_bank(cap, chans, rows, first_sample, n, B, TAPS)
        P, L, E = (tap_periods(first, d, starts) for d in TAPS)
        dops = [float(r.doppler_hz) + residual_doppler(p, period_s) for r, p in zip(acquired, P)]
        shifts = [code_shift(code_error(E[k], P[k], L[k]), ch) for k, ch in enumerate(chans)]
        prns, chans = channels_from_acq(search, results, first_sample, doppler_hz=dops)
        chans = [ch._replace(code_phase=(ch.code_phase + int(round(s * 2.0 ** 32))) % _PERIOD) for ch, s in zip(chans, shifts)]
        bank = dev.corr_bank(cap, chans, rows, first_sample, n, B, TAPS)
    P, L, E = (tap_periods(bank, d, starts) for d in TAPS)
    return [Observation(prn, dop, cn0(P[k], period_s), code_error(E[k], P[k], L[k]), shifts[k], P[k], chans[k], starts[k])
            for k, (prn, dop) in enumerate(zip(prns, dops))]
