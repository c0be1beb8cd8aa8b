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
