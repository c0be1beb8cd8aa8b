"""The acquisition search (csrc/k_acq.hip, gj_acq_search_dev / gj_acq_series_dev) restated on EXACT correlation power.
Not a test module: tests/acq_edges_inputs.py, tests/test_acq_edges_host.py and tests/acq_edges/ import it.  numpy only;
gpsjam.gnss gives the codes and the mixer's phase table (pinned by tests/test_acq_host.py), the oracle is not imported.

The reference's mixer is integer (int8 data times a 16-entry int8 table: |II|, |QQ| <= 8192) and the resampled code is
+-1, so what pcorrelator + cpxconv accumulate is, by definition (sdrcmn.c:124-147,742-773, restated without an FFT in
tests/test_acq_host.py::test_pcorrelator_restatement_against_the_definition),

    P[f][k] = (CSCALE / m)^2  sum over steps of  |sum_n (II_f + j QQ_f)[(n + k) mod m] code[n]|^2,     m = 2 nsamp,

an INTEGER times (CSCALE / m)^2.  exact_power() computes the inner sums by a float64 FFT and rounds them to the integers
they are (the residual is asserted), so every cell is exact: no float32 chain, neither the oracle's nor the kernels',
has a say in it.  check() is checkacquisition on such an array, search() the step loop with its early stop.
"""
import numpy as np

from gpsjam import gnss

CSCALE = 1.0 / 32.0                               # sdrcmn.c:7
COS16 = np.array([32, 30, 23, 12, 0, -12, -23, -30, -32, -30, -23, -12, 0, 12, 23, 30], np.int64)
SIN16 = np.array([0, 12, 23, 30, 32, 30, 23, 12, 0, -12, -23, -30, -32, -30, -23, -12], np.int64)
TIE_BAND = 1e-5                                   # the tie set: cells within this (relative) of the array's maximum
CLEAR_CELL = 1e-3                                 # a clear case: the best cell beats every cell outside the tie set by this
CLEAR_RATIO = 1e-2                                # ... and the peak ratio keeps this (relative) distance from the threshold
SEEN = {"residual": 0.0, "power": 0}              # largest rounding residual and integer power so far (the host test prints them)


def geometry(fs):
    """(nsamp, nsampchip, ctime) as sdrinit.c:385-387 and gnss.AcqSearch derive them."""
    ctime = gnss.CA_LEN / gnss.CA_RATE
    nsamp = int(fs * ctime)
    return nsamp, int(nsamp / gnss.CA_LEN), ctime


def unit(nsamp):
    """(CSCALE / m)^2: a power of two, so integer power times it is exact in float64."""
    return (CSCALE / (2 * nsamp)) ** 2


def mixed(raw, first_sample, fs, hband, step_index, nsamp):
    """int64 II, QQ [n_freq][m] of the window of integration step `step_index`: int8 = u8 - 128 (sdrrcv.c:104-106)
    through the 16-entry tables at the phase indices of gnss.mixer_phase_table."""
    m = 2 * nsamp
    loc = int(first_sample) + step_index * nsamp
    win = np.asarray(raw, np.uint8)[2 * loc:2 * (loc + m)].astype(np.int64) - 128
    assert win.size == 2 * m, "the capture does not hold this step's window"
    di, dq = win[0::2], win[1::2]
    tab = gnss.mixer_phase_table(gnss.doppler_bins(0.0, hband), fs, m)
    co, si = COS16[tab], SIN16[tab]
    return co * di - si * dq, si * di + co * dq


def exact_power_prns(raw, first_sample, prns, fs, intg, hband):
    """exact_power() of several PRNs, [n_prn][intg][n_freq][nsamp]: the windows are mixed and transformed once."""
    nsamp, _, _ = geometry(fs)
    m = 2 * nsamp
    rcode = np.zeros((len(prns), m), np.float64)
    for k, prn in enumerate(prns):
        rcode[k, :nsamp] = gnss.resample_code(gnss.ca_code(prn), nsamp, fs)
    cconj = np.conj(np.fft.fft(rcode, axis=1))
    out = [[] for _ in prns]
    for s in range(intg):
        ii, qq = mixed(raw, first_sample, fs, hband, s, nsamp)
        X = np.fft.fft(ii + 1j * qq, axis=1)
        for k in range(len(prns)):
            corr = np.fft.ifft(X * cconj[k][None, :], axis=1)[:, :nsamp]                 # sum_n x[n + k] code[n]
            re, im = np.rint(corr.real), np.rint(corr.imag)
            resid = max(float(np.max(np.abs(corr.real - re))), float(np.max(np.abs(corr.imag - im))))
            assert resid < 1e-3, ("the float64 FFT does not land on the integers", resid)
            SEEN["residual"] = max(SEEN["residual"], resid)
            re, im = re.astype(np.int64), im.astype(np.int64)
            acc = re * re + im * im + (out[k][-1] if s else 0)
            assert int(acc.max()) < 2 ** 53, "the accumulated power must stay exact in int64 and in float64"
            SEEN["power"] = max(SEEN["power"], int(acc.max()))
            out[k].append(acc)
    return np.array(out)


def exact_power(raw, first_sample, prn, fs, intg, hband):
    """int64 [intg][n_freq][nsamp]: the power accumulated after every step, in units of (CSCALE / m)^2."""
    return exact_power_prns(raw, first_sample, [prn], fs, intg, hband)[0]


def kept(nsamp, codei, nsampchip, wrapped=True):
    """bool [nsamp]: the indices outside the +-2 nsampchip exclusion zone around codei, as maxvd / meanvd read exinds and
    exinde (sdrcmn.c:411-440): a wrapped zone (exinds > exinde) keeps only the indices strictly between.
    wrapped=False is the WRONG rule -- the unwrapped test applied to a wrapped zone -- for the mutation argument of
    tests/test_acq_edges_host.py."""
    exinds, exinde = codei - 2 * nsampchip, codei + 2 * nsampchip
    if exinds < 0:
        exinds += nsamp
    if exinde >= nsamp:
        exinde -= nsamp
    i = np.arange(nsamp)
    if exinds <= exinde or not wrapped:
        return (i < exinds) | (i > exinde)
    return (i < exinds) & (i > exinde)


def check(P, nsamp, n_freq, nsampchip, ctime, threshold, seed=True, wrapped=True, cell=None):
    """checkacquisition (sdracq.c:52-84) in float64 with the C's semantics, as oracle.acq_check states them, with
    nsampchip and the threshold as arguments and IEEE division: 0/0 is NaN and NaN is not acquired.  The threshold is
    the C's float.  seed=False / wrapped=False are the two WRONG rules of the mutation argument.  cell = a flat index:
    the record as it reads when THAT cell is taken for the maximum (exact ties: any cell of the tie set may be)."""
    P = np.asarray(P, np.float64).reshape(n_freq * nsamp)
    maxi = int(np.argmax(P)) if cell is None else int(cell)   # strict '>' from index 0: the FIRST maximum
    maxP = P[maxi]
    codei, freqi = maxi % nsamp, maxi // nsamp
    row = P[freqi * nsamp:(freqi + 1) * nsamp]
    keep = kept(nsamp, codei, nsampchip, wrapped)
    cand = keep.copy()
    cand[0] = False
    mx = row[0] if seed else -1.0                             # maxvd: max = data[0] whatever the exclusion zone says
    if cand.any():
        mx = max(mx, row[cand].max())
    with np.errstate(divide="ignore", invalid="ignore"):
        meanP = row[keep].sum() / np.float64(keep.sum())
        peakr = np.float64(maxP) / np.float64(mx)
        cn0 = 10.0 * np.log10(np.float64(maxP) / meanP / ctime)
    return {"maxP": float(maxP), "maxP2": float(mx), "meanP": float(meanP), "peakr": float(peakr), "cn0": float(cn0),
            "codei": codei, "freqi": freqi, "cnt": int(keep.sum()),
            "acquired": bool(peakr > float(np.float32(threshold)))}


def search(raw, first_sample, prn, fs, intg, hband, threshold=3.0, nsampchip=None, seed=True, wrapped=True, Pint=None):
    """sdraqcuisition's step loop (sdracq.c:3-50) on exact power: one entry per step RUN, the last one deciding.
    Each entry: the record of check() plus 'steps'; 'P' (float64 [n_freq][nsamp], exact); 'ties' (flat indices of the cells
    whose power is >= max (1 - TIE_BAND)); 'cell_margin' (best cell over the best cell outside the tie set, minus one;
    inf where every cell ties); 'ratio_margin' (|peak_ratio / threshold - 1|, NaN for 0/0)."""
    nsamp, chip, ctime = geometry(fs)
    if nsampchip is None:
        nsampchip = chip
    if Pint is None:                                          # (a caller with many PRNs passes exact_power_prns()'s)
        Pint = exact_power(raw, first_sample, prn, fs, intg, hband)
    n_freq = Pint.shape[1]
    out = []
    for s in range(intg):
        P = Pint[s].astype(np.float64) * unit(nsamp)
        rec = check(P, nsamp, n_freq, nsampchip, ctime, threshold, seed, wrapped)
        rec["steps"] = s + 1
        flat = Pint[s].reshape(-1)
        top = int(flat.max())
        tie = flat.astype(np.float64) >= top * (1.0 - TIE_BAND)
        rest = flat[~tie]
        rec["P"] = P
        rec["ties"] = np.flatnonzero(tie)
        rec["cell_margin"] = float(top) / float(rest.max()) - 1.0 if rest.size and rest.max() > 0 else float("inf")
        with np.errstate(invalid="ignore"):
            rec["ratio_margin"] = float(abs(np.float64(rec["peakr"]) / np.float64(np.float32(threshold)) - 1.0))
        out.append(rec)
        if rec["acquired"]:
            break
    return out


def is_clear(steps):
    """Every step up to the deciding one: one cell (or one tie set) stands out and the ratio is away from the threshold."""
    return all(s["cell_margin"] >= CLEAR_CELL and s["ratio_margin"] >= CLEAR_RATIO for s in steps)
