"""Monte-Carlo validation of a CARLA replay: which cost gives plans that
collide less under the noise model, tick by tick.

For a replay file (``replay.py``; or ``--synthetic TICKS``) and each cost of
``--costs`` (``mmd``, ``cvar``, ``det``) the ticks of ``--ticks A B`` are solved
one after the other as ``carla/main_carla.py:378-382`` does -- ``mean_param``
carried from tick to tick, ``idx_mpc`` = the tick -- the returned plans
(``v_best``, ``steering_best``) are collected, and all ticks of the cost are
validated in ONE ``mpcmmd_validate_carla`` call (``optimizer/validation.py``:
``num_rollouts`` noisy rollouts per plan against the tick's obstacles and lane
bounds).  Per cost one ``validate_<cost>.npz`` is written with ``count``
(max over (obstacle, step) of the rollouts in collision), ``count_rows``
(rollouts with any collision: the plan's collision probability times R),
``count_lane``, ``tick`` and ``num_rollouts``; and one line is printed with the
share of ticks with ``count_rows > 0`` and the mean ``count_rows / R``.

With ``--risk`` the one call per cost is ``mpcmmd_validate_carla_risk``
(``optimizer/validation.py: risk_plans``): the count arrays come from it, and
the file also holds ``risk_count_pos``, ``risk_var``, ``risk_cvar``,
``risk_mean``, ``risk_max`` [ticks, 3] (channels obs, lane_lb, lane_ub: the
plan's own cost terms over the R rollouts, at quantile ``--risk-alpha``),
``risk_mmd`` [ticks, 3, S] at the bandwidths ``--risk-sigma``, ``risk_sigma``
and ``risk_alpha``; one more line per cost gives the mean obstacle CVaR and
SAA.  Without ``--risk`` the file and the line are what they were.

The solver is a sampling optimizer, so a difference between two costs needs
replicas over solver seeds.  With ``--replicas E`` (E > 1) every cost runs E
independent chains in lockstep: at tick k all E chains are ONE batched solve
(``CEM.compute_cem_batch``, mpcmmd_carla_solve_batch) on the tick's inputs,
computed once; chain e solves with ``idx_mpc = k + 100000 e`` (so every tick
must be < 100000) and carries its own ``mean_param``; chain 0 is the chain of
``--replicas 1``.  All E x ticks plans of a cost go to the one validation call
with the TICK as every chain's validation key -- common random numbers: the
chains differ by their plans only.  Every per-tick array of the file then has a
leading [E] axis, ``replica_key_stride`` (100000) is stored, and the lines
give mean +- sample standard deviation over the chains.  With ``--replicas 1``
files and lines are byte for byte what they are without the option.

With ``--device-setup`` the solves go through the tick route
(``CEM.compute_cem_tick_batch``, mpcmmd_carla_tick_solve_batch): the path
smoothing, path parameters and Frenet setup of every tick run on the GPU in
front of the solve, from ``replay.tick_raw_inputs``.  The route is bit-equal to
the host helpers', so files and lines are unchanged.

    cd mpc-mmd_amd/carla
    python -m validate_replay --synthetic 200 --costs cvar det --ticks 40 120 --out stats

The solver, the validator and the per-tick inputs are parameters of
``validate_replay`` (``solve=``, ``solve_batch=``, ``validate=``, ``risk_fn=``, ``inputs=``), so the
accounting is testable without a GPU.
"""
from __future__ import annotations

import argparse
import importlib
import importlib.util
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
COSTS = {"mmd": "compute_cem_mmd", "cvar": "compute_cem_cvar", "det": "compute_cem_det"}
# main_carla.py:302-320: v_des = 10, mean (v_des x 4, y = 0 x 4), cov diag(20 x 4, 100 x 4)
V_DES = 10.0
MEAN = np.array([V_DES] * 4 + [0.0] * 4, np.float32)
COV = np.diag([20.0] * 4 + [100.0] * 4).astype(np.float32)
REPLICA_KEY_STRIDE = 100000   # chain e of --replicas solves tick k with idx_mpc = k + REPLICA_KEY_STRIDE e


def _replay():
    """replay.py of this directory (loaded by path: the module may itself be loaded by path)."""
    name = "mpcmmd_carla_replay"
    if name not in sys.modules:
        spec = importlib.util.spec_from_file_location(name, os.path.join(_HERE, "replay.py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
    return sys.modules[name]


def _solve(prob, cost, tick, init, mean, cov, xo, yo, v_des, path):
    """func_cem of main_carla.py:188-194, 378-382."""
    p = path
    return getattr(prob, COSTS[cost])(tick, init, mean, cov, xo, yo, v_des, p["x_path"], p["y_path"], p["arc_vec"],
                                      p["Fx_dot"], p["Fy_dot"], p["kappa"])


def _solve_batch(prob, cost, idx_mpc, inits, means, cov, xo, yo, v_des, paths):
    """len(idx_mpc) independent solves of one cost in one batch: a list of func_cem's 5-tuples."""
    return prob.compute_cem_batch(cost, idx_mpc, inits, means, cov, xo, yo, v_des, paths)


def _inputs(rec, prob, tick):
    return _replay().tick_inputs(rec, tick, prob.cem_helper, prob.num_obs)


THRESHOLD = 0.1   # custom_path_smoothing's (main_carla.py:363)


def _device_tick(prob, rec, cost, tick, idx_mpc, means, v_des):
    """len(idx_mpc) solves of one tick through the tick route (``--device-setup``):
    (the 5-tuples, init, xo, yo, path) with the path read back from the device
    and the validator's obstacle tracks made from it by the host helpers."""
    E = len(idx_mpc)
    init, xw, yw, ob = _replay().tick_raw_inputs(rec, tick, prob.num_obs)
    res, paths = prob.compute_cem_tick_batch(cost, idx_mpc, [init] * E, [xw] * E, [yw] * E, [ob] * E, THRESHOLD,
                                             means, COV, v_des)
    path, h = paths[0], prob.cem_helper
    xi, yi, vxi, vyi, pi = h.global_to_frenet_obs_vmap(ob[:, 0], ob[:, 1], ob[:, 2], ob[:, 3], ob[:, 4],
                                                       *(path[k] for k in ("x_path", "y_path", "arc_vec", "Fx_dot",
                                                                           "Fy_dot", "kappa")))
    xo, yo, _ = h.compute_obs_trajectories(xi, yi, vxi, vyi, pi)
    return res, init, xo, yo, path


def _validate(prob, plans, num_rollouts, seed):
    # optimizer/validation.py of the package prob's class lives in (whatever name it was imported under)
    pkg = type(prob).__module__.rpartition(".")[0]
    validate_plans = importlib.import_module(pkg + ".validation").validate_plans
    return validate_plans(prob, plans, num_rollouts=num_rollouts, seed=seed)


def _risk(prob, plans, num_rollouts, seed, alpha, sigma):
    pkg = type(prob).__module__.rpartition(".")[0]
    risk_plans = importlib.import_module(pkg + ".validation").risk_plans
    return risk_plans(prob, plans, num_rollouts=num_rollouts, alpha=alpha, sigma=sigma, seed=seed)


RISK_KEYS = ("count_pos", "var", "cvar", "mean", "max", "mmd")


def solve_ticks(prob, rec, cost, ticks, v_des=V_DES, solve=None, inputs=None, device_setup=False):
    """The plans of ``ticks`` (in order) under ``cost``: per tick a dict with
    init, xo, yo, path, v_best, steering, mean_param, tick, key (= tick).
    device_setup: the tick route (``solve`` and ``inputs`` are unused then)."""
    solve = solve or _solve
    inputs = inputs or _inputs
    mean = MEAN.copy()
    plans = []
    for k in ticks:
        if device_setup:
            res, init, xo, yo, path = _device_tick(prob, rec, cost, int(k), [int(k)], mean, v_des)
            _, _, v_best, steering, mean = res[0]
        else:
            init, xo, yo, path = inputs(rec, prob, int(k))
            _, _, v_best, steering, mean = solve(prob, cost, int(k), init, mean, COV, xo, yo, v_des, path)
        plans.append(dict(tick=int(k), key=int(k), init=init, xo=xo, yo=yo, path=path, v_best=np.array(v_best),
                          steering=np.array(steering), mean_param=np.array(mean)))
    return plans


def solve_ticks_replicas(prob, rec, cost, ticks, replicas, v_des=V_DES, solve_batch=None, inputs=None,
                         device_setup=False):
    """``replicas`` chains over ``ticks`` in lockstep, a tick's chains as one
    batched solve: plans[e][i] as ``solve_ticks`` gives them (key = the tick
    for every chain), plus ``replica`` and ``idx_mpc``.  device_setup: the
    tick route (``solve_batch`` and ``inputs`` are unused then)."""
    solve_batch = solve_batch or _solve_batch
    inputs = inputs or _inputs
    E = int(replicas)
    means = [MEAN.copy() for _ in range(E)]
    plans = [[] for _ in range(E)]
    for k in ticks:
        idx = [int(k) + REPLICA_KEY_STRIDE * e for e in range(E)]
        if device_setup:
            res, init, xo, yo, path = _device_tick(prob, rec, cost, int(k), idx, [m.copy() for m in means], v_des)
        else:
            init, xo, yo, path = inputs(rec, prob, int(k))   # once per tick: the chains share them
            res = solve_batch(prob, cost, idx, [init] * E, [m.copy() for m in means], COV, [xo] * E, [yo] * E, v_des,
                              [path] * E)
        if len(res) != E:
            raise ValueError(f"solve_batch returned {len(res)} results for {E} chains")
        for e, (_, _, v_best, steering, mean) in enumerate(res):
            means[e] = np.array(mean, np.float32)
            plans[e].append(dict(tick=int(k), key=int(k), replica=e, idx_mpc=idx[e], init=init, xo=xo, yo=yo,
                                 path=path, v_best=np.array(v_best), steering=np.array(steering),
                                 mean_param=means[e].copy()))
    return plans


def _mean_std(v):
    """mean and sample standard deviation (n - 1) over the chains"""
    v = np.asarray(v, np.float64)
    return float(v.mean()), float(v.std(ddof=1)) if v.size > 1 else 0.0


def validate_replay(rec, prob, costs=("mmd", "cvar", "det"), ticks=None, num_rollouts=1000, out_dir=None, seed=0,
                    v_des=V_DES, solve=None, validate=None, inputs=None, log=print, risk=False, risk_sigma=(),
                    risk_alpha=0.98, risk_fn=None, replicas=1, solve_batch=None, device_setup=False):
    """See the module docstring.  ticks: iterable of tick indices (default:
    every tick of the recording).  risk: one ``risk_fn(prob, plans,
    num_rollouts, seed, alpha, sigma)`` call per cost (default: ``risk_plans``)
    in place of ``validate``; it returns the counts too.  replicas: E chains per
    cost through ``solve_batch(prob, cost, idx_mpc, inits, means, cov, xo, yo,
    v_des, paths)`` (default: ``prob.compute_cem_batch``; ``solve`` is the
    single chain's and unused then).  device_setup: solve through the tick route
    (``prob.compute_cem_tick_batch`` on ``replay.tick_raw_inputs``); the files
    equal the host route's.  Returns {cost: the npz fields}."""
    ticks = list(range(rec["ego"].shape[0])) if ticks is None else [int(k) for k in ticks]
    E = int(replicas)
    if E < 1:
        raise ValueError("replicas must be >= 1")
    if E > 1:
        if any(k < 0 or k >= REPLICA_KEY_STRIDE for k in ticks):
            raise ValueError(f"replicas need every tick in [0, {REPLICA_KEY_STRIDE}): chain e solves tick k with "
                             f"idx_mpc = k + {REPLICA_KEY_STRIDE} e")
        return _validate_replicas(rec, prob, costs, ticks, num_rollouts, out_dir, seed, v_des, solve_batch, validate,
                                  inputs, log, risk, risk_sigma, risk_alpha, risk_fn, E, device_setup)
    validate = validate or _validate
    risk_fn = risk_fn or _risk
    sigma = np.asarray(risk_sigma, np.float32).reshape(-1)
    R = int(num_rollouts)
    results = {}
    for cost in costs:
        if cost not in COSTS:
            raise ValueError(f"cost must be one of {sorted(COSTS)}")
        plans = solve_ticks(prob, rec, cost, ticks, v_des, solve, inputs, device_setup)
        if risk:
            res = risk_fn(prob, plans, R, seed, float(risk_alpha), sigma) if plans else {}
        else:
            res = validate(prob, plans, R, seed) if plans else {}
        out = {k: np.asarray(res.get(k, np.zeros(0, np.int32)), np.int32).reshape(len(ticks))
               for k in ("count", "count_rows", "count_lane")}
        out["tick"] = np.asarray(ticks, np.int32)
        out["num_rollouts"] = np.int32(R)
        if risk:
            n = len(ticks)
            for k in RISK_KEYS:
                shape = (n, 3, sigma.size) if k == "mmd" else (n, 3)
                dt = np.int32 if k == "count_pos" else np.float32
                out["risk_" + k] = np.asarray(res.get(k, np.zeros(shape, dt)), dt).reshape(shape)
            out["risk_sigma"] = sigma
            out["risk_alpha"] = np.float32(risk_alpha)
        if out_dir is not None:
            os.makedirs(out_dir, exist_ok=True)
            np.savez(os.path.join(out_dir, f"validate_{cost}.npz"), **out)
        n = len(ticks)
        share = float((out["count_rows"] > 0).mean()) if n else 0.0
        prob_mean = float((out["count_rows"] / R).mean()) if n else 0.0
        log(f"{cost}: {n} ticks, share with count_rows > 0 = {share:.4f}, mean count_rows / R = {prob_mean:.6f}")
        if risk:
            cvar_obs = float(out["risk_cvar"][:, 0].mean()) if n else 0.0
            saa_obs = float((out["risk_count_pos"][:, 0] / R).mean()) if n else 0.0
            log(f"{cost}: risk over {R} rollouts, mean obstacle CVaR({float(risk_alpha):g}) = {cvar_obs:.6f}, "
                f"mean obstacle SAA = {saa_obs:.6f}")
        results[cost] = out
    return results


def _validate_replicas(rec, prob, costs, ticks, num_rollouts, out_dir, seed, v_des, solve_batch, validate, inputs, log,
                       risk, risk_sigma, risk_alpha, risk_fn, E, device_setup=False):
    """validate_replay with E > 1 chains per cost."""
    validate = validate or _validate
    risk_fn = risk_fn or _risk
    sigma = np.asarray(risk_sigma, np.float32).reshape(-1)
    R, n = int(num_rollouts), len(ticks)
    results = {}
    for cost in costs:
        if cost not in COSTS:
            raise ValueError(f"cost must be one of {sorted(COSTS)}")
        chains = solve_ticks_replicas(prob, rec, cost, ticks, E, v_des, solve_batch, inputs, device_setup)
        plans = [p for chain in chains for p in chain]   # chain-major: [E][ticks]
        if risk:
            res = risk_fn(prob, plans, R, seed, float(risk_alpha), sigma) if plans else {}
        else:
            res = validate(prob, plans, R, seed) if plans else {}
        out = {k: np.asarray(res.get(k, np.zeros(0, np.int32)), np.int32).reshape(E, n)
               for k in ("count", "count_rows", "count_lane")}
        out["tick"] = np.tile(np.asarray(ticks, np.int32), (E, 1))
        out["num_rollouts"] = np.int32(R)
        out["replica_key_stride"] = np.int32(REPLICA_KEY_STRIDE)
        if risk:
            for k in RISK_KEYS:
                shape = (E, n, 3, sigma.size) if k == "mmd" else (E, n, 3)
                dt = np.int32 if k == "count_pos" else np.float32
                out["risk_" + k] = np.asarray(res.get(k, np.zeros(shape, dt)), dt).reshape(shape)
            out["risk_sigma"] = sigma
            out["risk_alpha"] = np.float32(risk_alpha)
        if out_dir is not None:
            os.makedirs(out_dir, exist_ok=True)
            np.savez(os.path.join(out_dir, f"validate_{cost}.npz"), **out)
        share = _mean_std((out["count_rows"] > 0).mean(axis=1) if n else np.zeros(E))
        prob_mean = _mean_std((out["count_rows"] / R).mean(axis=1) if n else np.zeros(E))
        log(f"{cost}: {n} ticks x {E} replicas, share with count_rows > 0 = {share[0]:.4f} +- {share[1]:.4f}, "
            f"mean count_rows / R = {prob_mean[0]:.6f} +- {prob_mean[1]:.6f}")
        if risk:
            cvar_obs = _mean_std(out["risk_cvar"][:, :, 0].mean(axis=1) if n else np.zeros(E))
            saa_obs = _mean_std((out["risk_count_pos"][:, :, 0] / R).mean(axis=1) if n else np.zeros(E))
            log(f"{cost}: risk over {R} rollouts, mean obstacle CVaR({float(risk_alpha):g}) = {cvar_obs[0]:.6f} +- "
                f"{cvar_obs[1]:.6f}, mean obstacle SAA = {saa_obs[0]:.6f} +- {saa_obs[1]:.6f}")
        results[cost] = out
    return results


def main(argv=None):
    ap = argparse.ArgumentParser(description="Monte-Carlo validation of the plans of a CARLA replay")
    ap.add_argument("replay", nargs="?", help="replay .npz (replay.py)")
    ap.add_argument("--synthetic", type=int, metavar="TICKS", help="record_synthetic(TICKS) instead of a file")
    ap.add_argument("--town", default="Town05", help="town of the synthetic recording")
    ap.add_argument("--costs", nargs="+", default=["mmd", "cvar", "det"], choices=sorted(COSTS))
    ap.add_argument("--ticks", type=int, nargs=2, metavar=("A", "B"), help="ticks A .. B-1 (default: all)")
    ap.add_argument("--num-rollouts", type=int, default=1000)
    ap.add_argument("--out", default="stats_carla")
    ap.add_argument("--num-reduced", type=int, default=10, help="num_reduced_sqrt (main_carla.py: 10)")
    ap.add_argument("--num-obs", type=int, default=3)
    ap.add_argument("--num-prime", type=int, default=60)
    ap.add_argument("--noise", default="gaussian", choices=["gaussian", "beta"])
    ap.add_argument("--noise-level", type=float, default=0.1)
    ap.add_argument("--acc-const-noise", type=float, default=0.0)
    ap.add_argument("--steer-const-noise", type=float, default=0.0)
    ap.add_argument("--num-batch", type=int, default=100)
    ap.add_argument("--maxiter-cem", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--risk", action="store_true",
                    help="also the risk statistics of the plans' cost terms (mpcmmd_validate_carla_risk)")
    ap.add_argument("--risk-sigma", type=float, nargs="+", default=[], metavar="S", help="MMD bandwidths")
    ap.add_argument("--risk-alpha", type=float, default=0.98, help="quantile level of VaR / CVaR")
    ap.add_argument("--replicas", type=int, default=1, metavar="E",
                    help="independent solver chains per cost, a tick's E solves in one batch")
    ap.add_argument("--device-setup", action="store_true",
                    help="the per-tick path and Frenet preprocessing on the GPU (mpcmmd_carla_tick_solve_batch)")
    a = ap.parse_args(argv)
    if (a.replay is None) == (a.synthetic is None):
        ap.error("give a replay file or --synthetic TICKS")
    R = _replay()
    rec = R.record_synthetic(a.synthetic, town=a.town) if a.synthetic is not None else R.load(a.replay)
    if sys.path[0] != _HERE:
        sys.path.insert(0, _HERE)
    from optimizer import cem
    prob = cem.CEM(a.num_reduced, 1, a.num_obs, a.noise_level, a.num_prime, a.noise, str(rec["town"]),
                   a.acc_const_noise, a.steer_const_noise, num_batch=a.num_batch, maxiter_cem=a.maxiter_cem,
                   seed=a.seed, max_configs=a.replicas)
    ticks = None if a.ticks is None else range(a.ticks[0], a.ticks[1])
    validate_replay(rec, prob, a.costs, ticks, a.num_rollouts, a.out, a.seed, risk=a.risk,
                    risk_sigma=a.risk_sigma, risk_alpha=a.risk_alpha, replicas=a.replicas,
                    device_setup=a.device_setup)
    prob.handle.close()


if __name__ == "__main__":
    main()
