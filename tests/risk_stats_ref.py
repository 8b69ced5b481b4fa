"""Expected values of mpcmmd_validate_risk from the oracle.  The rollouts
come from ``oracle.validation.compute_stats(..., return_rollouts=True)``, the
estimators from ``oracle.costs`` (quantile_linear, cvar, saa, mmd); this module
only forms the three per-rollout channels (obs, lane_lb, lane_ub) and calls
those.  Plain module like parity.py, and the sample patterns of the GPU tests.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

from oracle import costs as Cst
from oracle import validation as V

F32 = np.float32
F64 = np.float64
CHANNELS = ("obs", "lane_lb", "lane_ub")


def channels(prob, xr, yr, x_obs, y_obs):
    """[3][R] fp32 costs of the [R][H] fp64 rollouts (xr, yr): the fp64 bars of
    oracle.validation.compute_stats, max-reduced, rounded once."""
    H = xr.shape[1]
    xo = np.asarray(x_obs, F32)[:, :H].astype(F64)
    yo = np.asarray(y_obs, F32)[:, :H].astype(F64)
    wc = xr[None] - xo[:, None]
    ws = yr[None] - yo[:, None]
    cost = -(wc ** 2) / (4.25 ** 2) - (ws ** 2) / (2.75 ** 2) + 1.0
    obs = np.maximum(0.0, cost).max(axis=(0, 2))
    lb = np.maximum(0.0, -yr + prob.y_lb).max(axis=1)
    ub = np.maximum(0.0, yr - prob.y_ub).max(axis=1)
    return np.stack([obs, lb, ub]).astype(F32)


def rollout_channels(prob, cx, cy, init_state, x_obs, y_obs, noise, noise_level, acc_const, steer_const, draws):
    _, _, xr, yr = V.compute_stats(prob, cx, cy, init_state, x_obs, y_obs, noise, noise_level, acc_const, steer_const,
                                   draws, return_rollouts=True)
    return channels(prob, xr, yr, x_obs, y_obs)


def stats(c, alpha=0.98, sigma=(), ker_wt=1000.0):
    """The statistics of samples c [..., R] fp32: dict of count_pos, saa, var,
    cvar, mean, max [...] and mmd [..., S]."""
    c = np.asarray(c, F32)
    R = c.shape[-1]
    prob = SimpleNamespace(alpha_quant=alpha, ker_wt=ker_wt)
    with np.errstate(invalid="ignore", over="ignore"):
        out = dict(count_pos=(~(c <= 0)).sum(axis=-1).astype(np.int32),
                   saa=Cst.saa(prob, c),
                   var=Cst.quantile_linear(c, alpha),
                   cvar=Cst.cvar(prob, c),
                   mean=Cst.f32(c.astype(F64).sum(axis=-1) / R),
                   max=np.sort(c, axis=-1)[..., -1])
        beta = np.full(c.shape, F32(1.0 / R), F32)
        out["mmd"] = np.stack([Cst.mmd(prob, beta, c, np.full(c.shape[:-1], s, F32)) for s in sigma],
                              axis=-1) if len(sigma) else np.zeros(c.shape[:-1] + (0,), F32)
    return out


# ------------------------------------------------------------------ patterns
def position(R, alpha=0.98):
    """(lo, hi) of oracle.costs.quantile_linear."""
    pos = F32(alpha) * F32(R - 1)
    return int(np.floor(pos)), int(np.ceil(pos))


def patterns(R, rng, alpha=0.98):
    """Named fp32 sample vectors [R] in the style of tie_patterns.py: the cases
    where a count, an order statistic or a sum can go wrong."""
    lo, hi = position(R, alpha)
    out = {}

    def put(name, sorted_vals):
        out[name] = np.asarray(sorted_vals, F32)[rng.permutation(R)]

    def some_positive(frac):
        v = np.zeros(R, F32)
        n = max(1, int(round(frac * R)))
        v[:n] = rng.uniform(0.01, 1.0, n).astype(F32)
        return np.sort(v)

    distinct = np.sort((F32(0.001) + rng.permutation(R).astype(F32) / F32(R)).astype(F32))
    out["all_zero"] = np.zeros(R, F32)
    put("one_percent", some_positive(0.01))
    put("five_percent", some_positive(0.05))
    put("distinct", distinct)
    v = distinct.copy()          # a block of equal values across ranks lo / hi
    a, b = max(lo - 3, 0), min(hi + 3, R - 1)
    v[a:b + 1] = v[a]
    put("tie_block", np.sort(v))
    v = np.where(rng.random(R) < 0.5, F32(0.0), F32(-0.0)).astype(F32)   # either zero, a few positives on top
    n = max(1, R // 50)
    v[:n] = rng.uniform(0.1, 1.0, n).astype(F32)
    out["signed_zeros"] = v[rng.permutation(R)]
    v = distinct.copy()          # neighbours 1 ulp apart at lo / hi
    if hi > lo:
        v[hi] = np.nextafter(v[lo], F32(np.inf))
    elif lo > 0:
        v[lo] = np.nextafter(v[lo - 1], F32(np.inf))
    put("one_ulp", np.sort(v))
    put("subnormal", np.sort((rng.integers(1, 1 << 20, R).astype(np.uint32)).view(F32)))
    v = distinct.copy()
    v[-1] = np.inf
    put("inf_top", v)
    v = distinct.copy()
    v[rng.permutation(R)[:min(3, R)]] = np.nan
    out["three_nan"] = v[rng.permutation(R)]
    return out


def mmd_patterns(R, rng):
    """Finite vectors for the MMD: mostly zero, signed, all non-zero."""
    out = dict(all_zero=np.zeros(R, F32))
    v = np.zeros(R, F32)
    n = max(1, R // 10)
    v[rng.permutation(R)[:n]] = rng.uniform(0.001, 2.0, n).astype(F32)
    out["sparse"] = v
    v = rng.normal(0.0, 0.5, R).astype(F32)
    v[rng.permutation(R)[:R // 3]] = np.where(rng.random(R // 3) < 0.5, F32(0.0), F32(-0.0))
    out["signed"] = v
    out["dense"] = (rng.uniform(0.001, 3.0, R) * np.where(rng.random(R) < 0.2, -1.0, 1.0)).astype(F32)
    return out


def ulp_close(a, b, ulps=1):
    """a within `ulps` fp32 spacings of b (NaN == NaN, equal infinities)."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    same = (a == b) | (np.isnan(a) & np.isnan(b))
    with np.errstate(invalid="ignore"):
        near = np.abs(a.astype(F64) - b.astype(F64)) <= ulps * np.spacing(np.abs(b)).astype(F64)
    return same | near
