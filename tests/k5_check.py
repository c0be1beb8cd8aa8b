"""What K5 must return for one pair, and the check (CPU helper of the GPU tests; never imported by the product).

``expect(raw_i, raw_j)`` is the pair (i, j) -- the lag of slice j relative to slice i -- restated twice: the lag of the
oracle (the reference's complex64 arithmetic) and the float64 restatement (exact_restatement.xcorr_f64).  Both must
agree and the float64 peak must stand clear of the runner-up, or the case proves nothing: those are asserted as
preconditions.  ``check`` then holds a GPU (lag, peak, margin) to: the lag exactly, the peak to rtol 1e-4 and the margin
(1 - runner_up / peak) to atol 1e-4."""
import numpy as np

import exact_restatement as ex
from oracle import gpsjam_oracle as orc

GAP = 1e-3          # smallest relative gap between peak and runner-up a case may have
PEAK_RTOL = 1e-4
MARGIN_ATOL = 1e-4


def expect(raw_i: np.ndarray, raw_j: np.ndarray) -> dict:
    zi, zj = orc.tdoa_unpack(raw_i), orc.tdoa_unpack(raw_j)
    lag, peak, run = ex.xcorr_f64(zj, zi)
    lag32, _ = orc.xcorr_lag(zj, zi)
    assert lag32 == lag, f"oracle lag {lag32} != float64 lag {lag}: not a usable case"
    assert peak > 0 and (peak - run) / peak > GAP, f"peak {peak} and runner-up {run} are too close: not a usable case"
    return dict(lag=lag, peak=peak, margin=1.0 - run / peak)


def mirror(e: dict) -> dict:
    """The pair (j, i) from (i, j): |c_ji(m)| = |c_ij(-m)|, so the peak moves to -lag and peak and runner-up stay (with a
    clear gap no tie rule is involved)."""
    return dict(e, lag=-e["lag"])


def check(lag, peak, margin, e: dict, what=""):
    assert int(lag) == e["lag"], f"{what}: lag {int(lag)}, want {e['lag']}"
    assert abs(float(peak) - e["peak"]) <= PEAK_RTOL * e["peak"], f"{what}: peak {float(peak)}, want {e['peak']}"
    assert abs(float(margin) - e["margin"]) <= MARGIN_ATOL, f"{what}: margin {float(margin)}, want {e['margin']}"


def k5_fft_len(n: int) -> int:
    return max(1 << 16, 1 << (2 * n - 2).bit_length())


def k5_planted(n: int, lag: int, rng, second_lag=None, width=None, at=None):
    """(sig0, sig1), n samples each: low-level noise (bytes 127 / 128: +-0.5 after unpack) and one burst of rail values
    (0 / 255: +-127.5), 1..16 samples long, at the two places whose overlap is `lag` -- the correlation peak
    (correlate(sig1, sig0) peaks where sig1 is sig0 delayed by `lag`).  ``second_lag``: a copy at 0.8 amplitude
    (bytes 25 / 230) in sig1 as well, whose overlap is that lag -- a deliberate runner-up.  ``at``: the burst's place in
    sig0 (default: random)."""
    w = int(width or rng.integers(1, 17))
    w = min(w, n - abs(lag))
    sig = [rng.integers(127, 129, size=2 * n, dtype=np.uint8) for _ in range(2)]
    if at is not None:
        p0 = at
    elif lag >= 0:
        p0 = int(rng.integers(0, n - w - lag + 1))
    else:
        p0 = int(rng.integers(0, n - w + lag + 1)) - lag
    burst = rng.integers(0, 2, size=2 * w, dtype=np.uint8)
    assert 0 <= p0 <= n - w and 0 <= p0 + lag <= n - w
    sig[0][2 * p0:2 * (p0 + w)] = burst * 255
    sig[1][2 * (p0 + lag):2 * (p0 + lag + w)] = burst * 255
    if second_lag is not None:
        q = p0 + second_lag
        assert 0 <= q <= n - w and (q + w <= p0 + lag or q >= p0 + lag + w)
        sig[1][2 * q:2 * (q + w)] = np.where(burst == 1, 230, 25).astype(np.uint8)
    return sig[0], sig[1]


def k5_edge_lags(n: int):
    """Peaks at both ends of the 'full' range (circular index N-1 and L-N+1, the last ones before the zero-padding
    band), at 0, on both sides of a 4096-point row (the column index n2 = lag mod 4096 is 4095, 0, 1), at the first
    and last rows that hold a lag, and at the edge of a column kernel's tile of B = 4096 / L1 columns."""
    B = 4096 // (k5_fft_len(n) // 4096)
    K = (n - 2) // 4096
    lags = {n - 1, -(n - 1), n - 2, -(n - 2), 0, 4095, 4096, 4097, -4095, -4096, -4097, 4096 * K - 1, -(4096 * K + 1),
            B - 1, B, -B}
    return sorted(x for x in lags if abs(x) <= n - 1)


K5_PLANT_N = [32768, (1 << 22) - 3]      # L1 = 16 (L = 2N: a one-point padding band), L1 = 2048
