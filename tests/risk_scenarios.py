"""Obstacle scenarios that collide at any horizon, and the conditions that
keep a risk-stage comparison from being trivially zero (shared by
``test_gpu_risk_shapes.py`` and ``test_risk_scenarios.py``, its CPU counterpart).

The lockstep shapes of ``test_gpu_parity_baseline.py`` (obstacles at x = 40,
45, 70, the ego reaching x ~ 10 in H = 12 steps) see an obstacle cost of
exactly 0 (the MMD floor for mmd_random): here the obstacles are placed where
the oracle's rollouts of the shape actually go.
"""
from __future__ import annotations

import numpy as np

import oracle
from oracle import costs as C
from oracle import helper as Hh
from parity import DEFAULT_COV, DEFAULT_MEAN

B = 20
ACC_C, STEER_C = 0.05, 0.01
# cvar, mmd_random: the ego starts 5 cm inside the upper lane bound (y_ub =
# 2.25) and drifts out of it at 0.5 m/s, so the lane bars are non-zero from
# step 1 on, at H = 2 as well.  saa: it starts 3 cm inside with no drift, so
# only some samples of a candidate leave the lane and the lane count is not
# saturated either (every saa shape has H >= 12)
RISK_INIT = {"cvar": np.array([0.0, 2.2, 5.0, 0.5, 0.0, 0.0], np.float32),
             "mmd_random": np.array([0.0, 2.2, 5.0, 0.5, 0.0, 0.0], np.float32),
             "saa": np.array([0.0, 2.22, 5.0, 0.0, 0.0, 0.0], np.float32)}
Y_CYCLE = (1.75, -1.75, 3.6)
# saa: every obstacle on one line whose ellipses (b_obs = 2.75) graze the
# rollouts (y = 2.2 .. 2.3), so a candidate's samples fall on both sides;
# the line of each shape was chosen on the CPU for the conditions of
# assert_not_degenerate and a narrow bracket (saa_brackets)
SAA_Y = {(24, 3, 12): 4.9, (65, 64, 20): 4.7, (513, 65, 12): 4.85}
DELTA = 1e-4   # the contract's absolute tolerance on a residual


def make_oracle(cost, noise, S, O, H, level=None, seed=3):
    """(ora, draws, st, acc, steer): the oracle of the shape, its injected
    draws, the initial carry and the oracle's own controls of iteration 0."""
    level = (0.1 if noise == "gaussian" else 0.3) if level is None else level
    ora = oracle.CEM(S, O, level, H, noise, ACC_C, STEER_C, num_batch=B, maxiter_cem=1)
    draws = oracle.Draws.random(ora.prob, np.random.default_rng(seed), idx_mpc=123, seed=0, with_beta_cem=False)
    st = ora.init_state(RISK_INIT[cost], DEFAULT_MEAN, DEFAULT_COV, draws)
    _, acc, steer = ora.front(dict(st))
    return ora, draws, st, acc[:, :100], steer


def collision_scenario(ora, st, acc, steer, cost, overtaker=False):
    """x_obs, y_obs [O, 100] of O moving obstacles around the rollouts.

    x_end = the median final x of the oracle's noise-free rollouts.  x0 is
    spread over [0.35, 1.1] x_end + 3; obstacle 4k+1 starts at 4k's x and
    4k+3 at 4k+1's; vx = +3 m/s (even) / -3 m/s (odd).  So 4k and 4k+1 have
    bit-equal x at step 0 and part in opposite directions (the sorted order
    changes within any horizon), and 4k+1 and 4k+3 keep bit-equal x at every
    step, with different y.  y cycles over ``Y_CYCLE``; for saa every obstacle
    is on the line ``SAA_Y`` of the shape.

    ``overtaker`` (O >= 3, not saa): obstacle 2 overtakes in the ego's own
    lane.  It starts 4.3 m behind the ego (a_obs = 4.25: outside the window of
    step 0) at 19.3 m/s and is alongside at step 2 (x = 1.55, every rollout's
    x = 1.54 +- 0.01) while every other obstacle is still ahead of both.  So
    the window's start has to walk BACK to take it in, and at step 2 it is the
    nearest obstacle of every sample; it dominates every maximum, which is why
    the shape sweep runs without it."""
    p = ora.prob
    O, H, S = p.num_obs, p.num_prime, p.num_reduced
    xr, _ = Hh.rollout(p, acc[:, :H], steer[:, :H], st["st0"])
    x_end = float(np.median(xr[:, H - 1]))
    o = np.arange(O)
    x0 = np.linspace(0.35, 1.1, O) * x_end + 3.0
    i1 = np.nonzero(o % 4 == 1)[0]
    x0[i1] = x0[i1 - 1]
    i3 = np.nonzero(o % 4 == 3)[0]
    x0[i3] = x0[i3 - 2]
    y0 = np.full(O, SAA_Y[(S, O, H)]) if cost == "saa" else np.array(Y_CYCLE)[o % 3]
    vx = np.where(o % 2 == 0, 3.0, -3.0)
    if overtaker:
        assert O >= 3 and cost != "saa"
        x0[2], vx[2], y0[2] = -4.3, 19.3, float(RISK_INIT[cost][1])
    z = np.zeros(O)
    xo, yo, _ = Hh.compute_obs_trajectories(p, x0, y0, vx, z, z)
    return xo, yo


def mmd_floor(ora):
    """mmd_random's obstacle cost of a candidate that never collides."""
    p = ora.prob
    n = p.num_reduced
    return float(C.mmd(p, np.full((1, n), np.float32(1.0 / n)), np.zeros((1, n), np.float32),
                       np.full(1, np.float32(0.01)))[0])


def assert_not_degenerate(ora, cost, obs, lane, xo):
    """The oracle's values of a case are worth comparing (see the module
    docstring): asserted before any GPU value is looked at."""
    p = ora.prob
    O, H = p.num_obs, p.num_prime
    obs = np.asarray(obs)
    lane = np.asarray(lane)
    nb = obs.shape[0]
    if cost == "saa":
        mid = int(np.sum((obs > 0) & (obs < 1)))
        assert mid >= nb / 4, f"saa: only {mid}/{nb} candidates with 0 < obs < 1"
    else:
        floor = mmd_floor(ora) if cost == "mmd_random" else 0.0
        live = (obs != 0) & (obs != np.float32(floor))
        assert live.sum() >= nb / 2, f"{cost}: only {int(live.sum())}/{nb} non-zero, non-floor obstacle costs"
        assert len(np.unique(obs)) >= nb / 2, f"{cost}: only {len(np.unique(obs))} distinct obstacle costs"
    if O >= 2:
        x = np.asarray(xo, np.float32)[:, :H]
        assert not np.array_equal(np.argsort(x[:, 0], kind="stable"), np.argsort(x[:, H - 1], kind="stable")), \
            "the obstacles' x order never changes"
        assert any(len(np.unique(x[:, h])) < O for h in range(H)), "no two obstacles ever share an x"
    if cost == "mmd_random":
        assert not lane.any()       # cem.py:427: mmd_random's lane cost is zeros by definition
    else:
        assert np.count_nonzero(lane) >= 1, "every lane cost is 0"


def noisy_rollouts(ora, st, acc, steer, draws):
    """The oracle's fp32 rollouts of iteration 0: x, y [B, S, H]."""
    p = ora.prob
    H = p.num_prime
    acc_n, steer_n = Hh.noisy_controls(p, acc[:, :H], steer[:, :H], draws, 0, p.num_reduced)
    return Hh.rollout(p, acc_n, steer_n, st["st0"])


def saa_brackets(ora, xr, yr, xo, yo, delta=DELTA):
    """saa is a count: ((obs_lo, obs_hi), (lane_lo, lane_hi)) [B] integer
    brackets of S * cost from the unclipped fp64 margins of the oracle's
    rollouts, m = max over (o, h) of 1 - dx^2 / a^2 - dy^2 / b^2 (obstacles)
    and -y + y_lb, y - y_ub (lane): count(m > +delta) .. count(m > -delta)."""
    p = ora.prob
    H = p.num_prime
    x = np.asarray(xr, np.float64)
    y = np.asarray(yr, np.float64)
    a2 = float(np.float32(p.a_obs ** 2))
    b2 = float(np.float32(p.b_obs ** 2))
    m = np.full(x.shape[:-1], -np.inf)
    for o in range(p.num_obs):
        dx = x - np.float64(xo[o, :H])
        dy = y - np.float64(yo[o, :H])
        m = np.maximum(m, (1.0 - dx * dx / a2 - dy * dy / b2).max(axis=-1))
    lb = (-y + float(np.float32(p.y_lb))).max(axis=-1)
    ub = (y - float(np.float32(p.y_ub))).max(axis=-1)
    cnt = lambda v, d: (v > d).sum(axis=-1)
    return ((cnt(m, delta), cnt(m, -delta)),
            (cnt(lb, delta) + cnt(ub, delta), cnt(lb, -delta) + cnt(ub, -delta)))
