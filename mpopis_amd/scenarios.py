"""Scenario rollouts and risk costs: the written definition of what mpopis_set_risk computes (include/mpopis.h).

`aggregate` is plain NumPy and needs no GPU.  The device's risk kernel follows the same operation order (tail mean: sorted descending, summed
from the largest down, one division; entropic: the extreme the sign of theta selects is subtracted before exp), so in float64 the two differ
only by the rounding of exp / log; given dtype=np.longdouble it serves as the reference the tests bound the device against."""
import numpy as np

from . import _lib

RISK_TAIL_MEAN, RISK_ENTROPIC = 0, 1          # MPOPIS_RISK_*
MAX_SCENARIOS = 16                            # MPOPIS_MAX_SCENARIOS
RISK_KINDS = ("mean", "worst", "cvar", "entropic")


def _refuse(msg):
    raise _lib.MPOPISError(_lib.ERR_ARG, msg)


def resolve_risk(kind, M, tail=0, theta=0.0):
    """("mean" | "worst" | "cvar" | "entropic", tail, theta) for M scenarios -> (MPOPIS_RISK_*, tail in 1..M, theta); refuses what
    mpopis_set_risk refuses."""
    k = str(kind).lstrip(":")
    M = int(M)
    if M < 1:
        _refuse("risk: no scenarios set")
    if k == "mean":
        return RISK_TAIL_MEAN, M, 0.0
    if k == "worst":
        return RISK_TAIL_MEAN, 1, 0.0
    if k == "cvar":
        t = int(tail)
        if t != tail or t < 0 or t > M:
            _refuse("risk 'cvar': tail must be an integer in 0..%d (0 = all), got %r" % (M, tail))
        return RISK_TAIL_MEAN, t or M, 0.0
    if k == "entropic":
        th = float(theta)
        if th == 0.0 or not np.isfinite(th):
            _refuse("risk 'entropic': theta must be finite and non-zero, got %r" % (theta,))
        return RISK_ENTROPIC, M, th
    _refuse("unknown risk kind %r (%s)" % (kind, ", ".join(RISK_KINDS)))


def parse_risk(risk):
    """The harnesses' risk= argument -- "mean", "worst", ("cvar", tail), ("entropic", theta) -- as (kind, tail, theta)."""
    if isinstance(risk, str):
        if risk.lstrip(":") not in ("mean", "worst"):
            _refuse("risk=%r needs its parameter: (\"cvar\", tail) or (\"entropic\", theta)" % (risk,))
        return risk.lstrip(":"), 0, 0.0
    try:
        kind, val = risk
    except (TypeError, ValueError):
        _refuse("risk: \"mean\", \"worst\", (\"cvar\", tail) or (\"entropic\", theta), got %r" % (risk,))
    kind = str(kind).lstrip(":")
    if kind == "cvar":
        return kind, val, 0.0
    if kind == "entropic":
        return kind, 0, val
    _refuse("risk: \"mean\", \"worst\", (\"cvar\", tail) or (\"entropic\", theta), got %r" % (risk,))


def aggregate(costs, kind="mean", tail=0, theta=0.0, dtype=np.float64):
    """The risk aggregate J over the scenario axis: costs (..., M, K) -> (..., K), computed in `dtype` (np.float64 or np.longdouble).

      mean / worst / cvar   the mean of the `tail` largest of c_0..c_{M-1} (mean: M, worst: 1, cvar: tail, 0 = M), summed from the largest
                            down; tail = 1 returns that input itself.  Any NaN gives NaN, otherwise plain IEEE arithmetic.
      entropic              c* + log(mean(exp(theta (c - c*)))) / theta with c* = max c for theta > 0, min c for theta < 0.  If any c_m is not
                            finite, J is the IEEE sum of the non-finite c_m (NaN for a NaN or both infinities, else that infinity)."""
    c = np.asarray(costs, dtype=dtype)
    if c.ndim < 2:
        _refuse("aggregate: costs of shape (..., M, K)")
    M = c.shape[-2]
    rk, tl, th = resolve_risk(kind, M, tail, theta)
    c = np.moveaxis(c, -2, 0)                                   # (M, ..., K)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if rk == RISK_TAIL_MEAN:
            nan = np.isnan(c).any(axis=0)
            s = -np.sort(-np.where(np.isnan(c), dtype(0), c), axis=0)      # descending (NaN columns are overwritten below)
            if tl == 1:
                J = s[0].copy()
            else:
                J = s[0].copy()
                for i in range(1, tl):
                    J = J + s[i]
                J = J / dtype(tl)
            return np.where(nan, dtype(np.nan), J)
        bad = ~np.isfinite(c)
        any_bad = bad.any(axis=0)
        bad_sum = np.zeros(c.shape[1:], dtype=dtype)
        for m in range(M):
            bad_sum = bad_sum + np.where(bad[m], c[m], dtype(0))
        cf = np.where(bad, dtype(0), c)
        cs = cf.max(axis=0) if th > 0 else cf.min(axis=0)
        s = np.zeros(c.shape[1:], dtype=dtype)
        for m in range(M):
            s = s + np.exp(dtype(th) * (cf[m] - cs))
        J = cs + np.log(s / dtype(M)) / dtype(th)
        return np.where(any_bad, bad_sum, J)


def check_scenarios(params, B, n, per_slot=False):
    """set_scenarios' argument as a contiguous float64 array of shape (M, n) or, per slot, (B, M, n); None or an empty array -> None (M = 0)."""
    if params is None:
        return None
    p = np.ascontiguousarray(params, dtype=np.float64)
    if p.size == 0:
        return None
    want = 3 if per_slot else 2
    if p.ndim != want or (per_slot and p.shape[0] != B):
        _refuse("scenarios: an array of shape %s, got %s" % ("(B, M, n)" if per_slot else "(M, n)", p.shape))
    M = p.shape[-2]
    if M > MAX_SCENARIOS:
        _refuse("scenarios: at most %d per slot, got %d" % (MAX_SCENARIOS, M))
    if p.shape[-1] != n:
        _refuse("scenarios: this env expects %d parameters per scenario, got %d" % (n, p.shape[-1]))
    return p

