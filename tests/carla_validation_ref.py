"""Expected counts of ``mpcmmd_validate_carla`` (include/mpcmmd.h), composed
from the oracle's own functions: ``CarlaCEM.noisy_init``, ``helper.inject_noise``,
``carla.rollout_cr``, ``carla.frenet_points``, ``costs.compute_f_bar`` and the
comparisons of ``costs.lane_bar``.  Not a test; shared by
test_carla_validation_cpu.py and test_gpu_carla_validation.py.

Acceptance rule (``check_counts``).  The device functions are the ones
test_carla_tick_lockstep shows bit-identical to these oracle pieces, so
equality of the counts is expected and reported -- but a margin within an ulp
of zero may round to the other side, so the assertion is a bracket: the GPU's
count_oh[o][h] must lie in [#(m > +TOL), #(m > -TOL)] over the rows, m = 1 -
ds^2/a^2 - dd^2/b^2 the collision margin; the lane counters likewise on their
margins.  The bracket is only meaningful when few margins are that close, so
the share of |m| < TOL must be <= MAX_NEAR (asserted on the oracle side).
"""
import numpy as np

from oracle import carla as K
from oracle import costs as C
from oracle import helper as Hh
from oracle.rng import beta_draws, philox_normals

F32 = np.float32
F64 = np.float64
TOL = 1e-4
MAX_NEAR = 1e-3
# csrc/rng.hpp: kStreamVc*
STREAM_ACC, STREAM_STEER, STREAM_CONST = 32, 33, 34
STREAM_GAMMA_ACC_A, STREAM_GAMMA_ACC_B, STREAM_GAMMA_STEER_A, STREAM_GAMMA_STEER_B = 35, 36, 37, 38
STREAM_INIT_EPS = 39


def controls(prob, v, steer):
    """acc [100] = diff([v, v_end]) / t (helper.compute_controls' acc) and the steering as given."""
    v = np.asarray(v, F32).reshape(-1)
    acc = (np.diff(np.concatenate([v, v[-1:]])) / F32(prob.t)).astype(F32)
    return acc, np.asarray(steer, F32).reshape(-1)


def philox_draws(prob, key, seed, v, steer, R):
    """The library's internal streams of one tick: (draws [3, R, H], init_eps [R, 4])."""
    Hn = prob.num_prime
    kk = (int(key) & 0xFFFFFFFF, int(seed) & 0xFFFFFFFF)
    nrm = lambda s, n: philox_normals(kk, s, 0, n)
    nc = nrm(STREAM_CONST, R * Hn).reshape(R, Hn)
    if prob.noise == "gaussian":
        na = nrm(STREAM_ACC, R * Hn).reshape(R, Hn)
        ns = nrm(STREAM_STEER, R * Hn).reshape(R, Hn)
    else:
        acc, st = controls(prob, v, steer)
        elem = np.arange(R * Hn, dtype=np.uint64).reshape(R, Hn)
        a = np.broadcast_to(np.abs(acc[:Hn])[None], (R, Hn))
        s = np.broadcast_to(np.abs(st[:Hn])[None], (R, Hn))
        na = beta_draws((F32(prob.beta_a) * a).astype(F64), (F32(prob.beta_b) * a).astype(F64), kk,
                        STREAM_GAMMA_ACC_A, STREAM_GAMMA_ACC_B, elem)
        ns = beta_draws((F32(prob.beta_a) * s).astype(F64), (F32(prob.beta_b) * s).astype(F64), kk,
                        STREAM_GAMMA_STEER_A, STREAM_GAMMA_STEER_B, elem)
    return np.stack([na, ns, nc]).astype(F32), nrm(STREAM_INIT_EPS, R * 4).reshape(R, 4)


def reference(ora, init_state, v, steer, x_obs, y_obs, path, draws, init_eps):
    """One tick.  ora: oracle.carla.CarlaCEM of the tick's constants; draws
    [3, R, H]; init_eps [R, 4].  Returns count_oh [O, H], m [O, R, H], the lane
    margins lb, ub [R, H] and the reduced counts."""
    p = ora.prob
    Hn = p.num_prime
    acc, st = controls(p, v, steer)
    d = np.asarray(draws, F32)
    rows = ora.noisy_init(init_state, np.asarray(init_eps, F32))
    if p.noise == "gaussian":
        acc_n, steer_n = Hh.inject_noise(p, acc[None, :Hn], st[None, :Hn], d[0], d[1], d[2])
    else:
        acc_n, steer_n = Hh.inject_noise(p, acc[None, :Hn], st[None, :Hn], None, None, d[2], d[0][None], d[1][None])
    xr, yr = K.rollout_cr(p, acc_n, steer_n, rows[None, :, :])
    sf, df = K.frenet_points(xr[0], yr[0], path)                       # [R, H]
    xo, yo = np.asarray(x_obs, F32)[:, :Hn], np.asarray(y_obs, F32)[:, :Hn]
    hit = C.compute_f_bar(p, sf, df, xo, yo) > 0                        # [O, R, H]
    a2, b2 = F32(p.a_obs ** 2), F32(p.b_obs ** 2)
    ws, wd = sf[None] - xo[:, None, :], df[None] - yo[:, None, :]
    m = ((-(ws * ws)) / a2 - (wd * wd) / b2) + F32(1)
    assert np.array_equal(hit, m > 0)
    lb = (-df + F32(p.y_lb)).astype(F32)
    ub = (df - F32(p.y_ub)).astype(F32)
    count_oh = hit.sum(axis=1).astype(np.int32)
    return dict(count_oh=count_oh, m=m, lb=lb, ub=ub, count=int(count_oh.max()),
                count_rows=int(hit.any(axis=(0, 2)).sum()),
                count_lane=int((lb > 0).sum(axis=0).max() + (ub > 0).sum(axis=0).max()), frenet=(sf, df))


def near_share(ref):
    """Share of (o, r, h) collision margins within TOL of zero."""
    return float((np.abs(ref["m"]) < TOL).mean())


def check_counts(ref, got, R, label=""):
    """The acceptance rule on one tick: ``got`` = dict of the GPU's count,
    count_lane, count_rows (ints) and count_oh [O, H]."""
    m = ref["m"]
    share = near_share(ref)
    assert share <= MAX_NEAR, f"{label}: {share} of the margins within {TOL} of zero"
    oh = np.asarray(got["count_oh"])
    lo, hi = (m > TOL).sum(axis=1), (m > -TOL).sum(axis=1)
    exact = bool(np.array_equal(oh, ref["count_oh"]))
    print(f"{label}: count GPU {int(got['count'])} oracle {ref['count']}, rows GPU {int(got['count_rows'])} oracle "
          f"{ref['count_rows']}, lane GPU {int(got['count_lane'])} oracle {ref['count_lane']}, "
          f"count_oh equal: {exact}, near-zero share {share:.2e}")
    assert np.all(oh >= lo) and np.all(oh <= hi), f"{label}: count_oh outside the bracket"
    assert int(got["count"]) == int(oh.max()), f"{label}: count is not max count_oh"
    # rows: between the rows with a hit for sure and the rows with a possible hit; consistent with count_oh
    rlo, rhi = (m > TOL).any(axis=(0, 2)).sum(), (m > -TOL).any(axis=(0, 2)).sum()
    assert rlo <= int(got["count_rows"]) <= rhi, f"{label}: count_rows outside the bracket"
    assert int(oh.max()) <= int(got["count_rows"]) <= min(R, int(oh.sum())), f"{label}: count_rows vs count_oh"
    lane_lo = (ref["lb"] > TOL).sum(axis=0).max() + (ref["ub"] > TOL).sum(axis=0).max()
    lane_hi = (ref["lb"] > -TOL).sum(axis=0).max() + (ref["ub"] > -TOL).sum(axis=0).max()
    assert lane_lo <= int(got["count_lane"]) <= lane_hi, f"{label}: count_lane outside the bracket"
    return exact
