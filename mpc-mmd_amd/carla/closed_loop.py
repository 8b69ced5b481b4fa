"""Closed-loop CARLA episodes on the surrogate world.

The reference's CARLA experiment is closed-loop (``carla/main_carla.py:
329-457``): each tick the plan's first controls are averaged, perturbed by the
noise model and applied, the ego moves, and the next tick is solved from where
it ended up.  Here the simulator is replaced by a world model of this
project's (a kinematic bicycle, constant-velocity vehicles, the route's
splines), and E independent episodes run in lockstep on one CARLA batch handle.
By default the whole loop is enqueued on the GPU (mpcmmd_world_run: per tick the
chained begin, the CEM iterations and k_world_step, nothing crossing the host,
one readback of the log at the end).  With ``--host-step`` each tick is one
batched solve through the tick route (mpcmmd_carla_tick_solve_batch) and one
host step (mpcmmd_world_step_host); the files are equal.

    cd mpc-mmd_amd/carla
    python -m closed_loop --synthetic --episodes 8 --ticks 200 --costs cvar det --out stats

The synthetic route and spawns are those of ``replay.py``.  Episodes differ by
their key (the solver's streams and the perturbation's variates, which the
library draws after each tick's solve, normals or Beta(2 |control|, 5 |control|)
with ``--noise beta``) and, with
``--start-spread S``, by a start offset of up to S m along the route.  Per cost
``closed_loop_<cost>.npz`` holds the log arrays ``log_d`` [T, E, 3] (x, y, arc),
``log_f`` [T, E, 13] (v, psi, psidot, a_c, s_c, a, s, u[4], clear, d), ``log_i``
[T, E, 4] (idx, lane_out, collided, goal) and ``done_tick``, ``collided``,
``goal`` [E]; one line per cost gives the collision share, the mean minimum
-clear, the lane-departure share and the mean progress, each as mean +- sample
standard deviation over the episodes.

With ``--validate R [--alpha A] [--risk-sigma s ...]`` every tick's plan is also
rolled out under R fresh noise rows (on the GPU inside
the chained loop, or from the host with ``--host-step``; the files are equal
again).  The npz then also holds ``val_counts`` (count, count_lane, count_rows),
``val_count_pos``, ``val_var``, ``val_cvar``, ``val_mean``, ``val_max`` [T, E, 3]
(channels obs, lane_lb, lane_ub), ``val_mmd`` [T, E, 3, S] and ``val_est``
[T, E, 2] (the cost_lane and cost_obs the solve itself estimated), and a second
line per cost gives, over the live (tick, episode) pairs, the plans' mean
Monte-Carlo collision probability count_rows / R and the mean validated CVaR of
the obstacle cost beside the mean of the solver's own obstacle cost.

With ``--vehicles routed [--speed-limit V]`` the vehicles are not parked: they
follow the route at their spawn lane with car-following (DESIGN.md section 24,
a model of this project's, not CARLA's traffic manager).  Vehicle i of episode
e starts at rest at the spawn offset of ``replay.py`` ahead of the episode's
start, on its spawn lane, with the target speed (1 - p) V, p drawn from the
reference's (0.4, 0.6, 0.4) by a NumPy generator seeded with the episode's key;
V defaults to 8.33 m/s.  The npz then also holds ``veh`` [T, E, total_obs, 3]
(s, v and the acceleration applied after each tick's step), and one more line
per cost gives the mean vehicle speed, the smallest bumper gap between two
vehicles on one lane and the count of ticks on which the ego was some
vehicle's leader, over the live (tick, episode) pairs.

The episode runner is a parameter of ``closed_loop`` (``run=``), so the
accounting is testable without a GPU.
"""
from __future__ import annotations

import argparse
import importlib.util
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
COSTS = ("mmd", "cvar", "det")
V_DES = 10.0
LOG_KEYS = ("log_d", "log_f", "log_i", "done_tick", "collided", "goal")
SPEED_LIMIT = 8.33                # m/s (30 km/h)
SPEED_DIFFERENCE = (0.4, 0.6, 0.4)  # carla_simulation.py:222-225: vehicle_percentage_speed_difference
KEY_STRIDE = 100000               # run_episodes' default: episode e has the key KEY_STRIDE e
# the routed vehicles' scalars as the library defaults them (_native.ROUTED_DEFAULTS); the accounting reads three
LENGTH, LANE_TOL = 4.5, 1.75
VAL_KEYS = ("val_counts", "val_count_pos", "val_var", "val_cvar", "val_mean", "val_max", "val_mmd", "val_est")


def _load(name, *path):
    """The module at ``path``, loaded by file path once (this directory's ``optimizer`` hides the other one)."""
    if name not in sys.modules:
        spec = importlib.util.spec_from_file_location(name, os.path.join(*path))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
    return sys.modules[name]


def _replay():
    return _load("mpcmmd_carla_replay", _HERE, "replay.py")


# (mean, sample sd) of a vector: one definition for both drivers, in a module without relative imports
_mean_std = _load("mpcmmd_episode_stats", os.path.dirname(_HERE), "optimizer", "episode_stats.py").mean_std


def synthetic_world(town="Town05"):
    """The route and spawns of ``replay.record_synthetic``: ((x, y) of the
    extended route, goal_index = len_path - 1, vehicles [total_obs, 5])."""
    R = _replay()
    offs, lanes = R.SPAWN["Town10HD" if town.startswith("Town10") else "Town05"]
    rx, ry = R.synthetic_route()
    rt = R.Route(rx, ry)
    ox, oy, opsi = rt.at(offs.copy(), np.array([lanes[i % 2] for i in range(offs.size)]))
    vehicles = np.zeros((offs.size, 5), np.float32)
    vehicles[:, 0], vehicles[:, 1], vehicles[:, 4] = ox, oy, np.arctan2(np.sin(opsi), np.cos(opsi))
    return R.extend_route(rx, ry), rx.size - 1, vehicles


def synthetic_starts(route, episodes, spread=0.0, v0=0.1):
    """[E, 4] = x, y, v, psi: on the route, episode e ``spread`` e / E m along it, heading along it."""
    R = _replay()
    rt = R.Route(*route)
    s = spread * np.arange(episodes) / max(episodes, 1)
    x, y, psi = rt.at(s)
    return np.stack([x, y, np.full(episodes, v0), np.arctan2(np.sin(psi), np.cos(psi))], 1)


def routed_traffic(route, starts, town="Town05", speed_limit=SPEED_LIMIT, key_base=0, key_stride=KEY_STRIDE):
    """The ``routed`` dict of ``run_episodes`` for the spawns of ``replay.py``: s [E, total_obs] the spawn
    offsets ahead of each episode's start (its arc length on the route), d the spawn lanes, v = 0 and
    v0 = (1 - p) speed_limit with p one of SPEED_DIFFERENCE per vehicle, drawn by
    ``np.random.default_rng(key of the episode)``."""
    R = _replay()
    offs, lanes = R.SPAWN["Town10HD" if town.startswith("Town10") else "Town05"]
    rt = R.Route(*route)
    starts = np.asarray(starts, np.float64).reshape(-1, 4)
    E, V = starts.shape[0], offs.size
    s0 = np.array([rt.s[int(np.argmin(np.hypot(rt.x - x, rt.y - y)))] for x, y in starts[:, :2]])
    p = np.stack([np.random.default_rng(int(key_base) + int(key_stride) * e).choice(SPEED_DIFFERENCE, V)
                  for e in range(E)])
    return dict(s=s0[:, None] + offs[None, :], v=np.zeros((E, V), np.float32),
                d=np.tile(np.array([lanes[i % 2] for i in range(V)], np.float32), (E, 1)),
                v0=((1.0 - p) * float(speed_limit)).astype(np.float32))


def summarise_vehicles(res, routed):
    """The three figures of one cost's routed traffic over the live (tick, episode) pairs
    (``summarise``'s convention): the mean vehicle speed as (mean, sample sd) over the episodes, the
    smallest bumper gap s_k - s_j - length between two vehicles on one lane (|d_k - d_j| < lane_tol),
    and the count of ticks on which the ego -- at (arc, d) of its log row -- was the nearest thing
    ahead of some vehicle on its lane."""
    veh = np.asarray(res["veh"], np.float64)
    T, E, V = veh.shape[:3]
    done = np.asarray(res["done_tick"])
    last = np.where(done >= 0, done, T - 1)
    live = np.arange(T)[:, None] <= last[None, :]
    d = np.broadcast_to(np.asarray(routed["d"], np.float64).reshape(-1, V), (E, V))
    length, tol = float(routed.get("length", LENGTH)), float(routed.get("lane_tol", LANE_TOL))
    n = np.maximum(live.sum(axis=0), 1)
    speed = np.where(live, veh[:, :, :, 1].mean(axis=2) if V else np.zeros((T, E)), 0.0).sum(axis=0) / n
    s = veh[:, :, :, 0]
    ahead = s[:, :, None, :] - s[:, :, :, None]                          # [T, E, j, k] = s_k - s_j
    lane = np.abs(d[:, None, :] - d[:, :, None]) < tol                   # [E, j, k]
    pair = lane[None] & (ahead > 0) & live[:, :, None, None]
    gaps = np.where(pair, ahead - length, np.inf)
    ego_s, ego_d = np.asarray(res["log_d"])[:, :, 2], np.asarray(res["log_f"], np.float64)[:, :, 12]
    ego_ahead = ego_s[:, :, None] - s                                    # [T, E, j]
    ego_lane = np.abs(ego_d[:, :, None] - d[None]) < tol
    cand = ego_lane & (ego_ahead > 0)
    nearest = np.where(pair, ahead, np.inf).min(axis=3) if V else np.zeros((T, E, 0))
    leads = (cand & (ego_ahead < nearest)).any(axis=2) & live
    return dict(vehicle_speed=_mean_std(speed), min_gap=float(gaps.min()) if gaps.size else float("inf"),
                ego_led=int(leads.sum()))


def _run(prob, cost, route, goal_index, vehicles, starts, ticks, **kw):
    return prob.run_episodes(cost, route, vehicles, starts, ticks, goal_index=goal_index, **kw)


def summarise(res):
    """The four figures of one cost's episodes, each (mean, sample sd) over the
    episodes.  Rows after an episode's ``done_tick`` repeat its frozen state and
    are left out."""
    log_f, log_i, log_d = res["log_f"], res["log_i"], res["log_d"]
    T, E = log_i.shape[:2]
    done = np.asarray(res["done_tick"])
    last = np.where(done >= 0, done, T - 1)
    live = np.arange(T)[:, None] <= last[None, :]
    neg_clear = np.where(live, -log_f[:, :, 11].astype(np.float64), np.inf)
    return dict(collision=_mean_std(np.asarray(res["collided"], float)),
                min_neg_clear=_mean_std(neg_clear.min(axis=0) if T else np.zeros(E)),
                lane_departure=_mean_std((log_i[:, :, 1].astype(bool) & live).any(axis=0).astype(float)),
                progress=_mean_std(log_d[last, np.arange(E), 2] - log_d[0, :, 2] if T else np.zeros(E)))


def summarise_validation(res, rollouts):
    """The three figures of one cost's validated plans, each (mean, sample sd)
    over the episodes of the episode's mean over its live ticks (``summarise``'s
    convention: rows after ``done_tick`` are left out): the Monte-Carlo
    collision probability count_rows / R, the validated CVaR of the obstacle
    cost, and the obstacle cost the solver estimated."""
    T, E = res["val_counts"].shape[:2]
    done = np.asarray(res["done_tick"])
    last = np.where(done >= 0, done, T - 1)
    live = np.arange(T)[:, None] <= last[None, :]
    n = np.maximum(live.sum(axis=0), 1)
    per_episode = lambda a: np.where(live, np.asarray(a, np.float64), 0.0).sum(axis=0) / n
    return dict(p_collision=_mean_std(per_episode(res["val_counts"][:, :, 2] / float(rollouts))),
                cvar_obs=_mean_std(per_episode(res["val_cvar"][:, :, 0])),
                est_obs=_mean_std(per_episode(res["val_est"][:, :, 1])))


def closed_loop(prob, costs, route, goal_index, vehicles, starts, ticks, out_dir=None, run=None, log=print, **kw):
    """Runs ``run(prob, cost, route, goal_index, vehicles, starts, ticks, **kw)``
    (default: ``prob.run_episodes``) per cost, writes the files and prints the
    lines of the module docstring.  Returns {cost: (the result, its summary)}."""
    run = run or _run
    val = kw.get("validate")
    routed = kw.get("routed")
    keys = LOG_KEYS + (VAL_KEYS if val is not None else ()) + (("veh",) if routed is not None else ())
    results = {}
    for cost in costs:
        if cost not in COSTS:
            raise ValueError(f"cost must be one of {sorted(COSTS)}")
        res = run(prob, cost, route, goal_index, vehicles, starts, ticks, **kw)
        if out_dir is not None:
            os.makedirs(out_dir, exist_ok=True)
            np.savez(os.path.join(out_dir, f"closed_loop_{cost}.npz"), **{k: res[k] for k in keys})
        s = summarise(res)
        E = np.asarray(res["done_tick"]).size
        log(f"{cost}: {E} episodes x {int(ticks)} ticks, collision share = {s['collision'][0]:.4f} +- "
            f"{s['collision'][1]:.4f}, mean min -clear = {s['min_neg_clear'][0]:.4f} +- {s['min_neg_clear'][1]:.4f}, "
            f"lane departure share = {s['lane_departure'][0]:.4f} +- {s['lane_departure'][1]:.4f}, "
            f"mean progress = {s['progress'][0]:.2f} +- {s['progress'][1]:.2f} m")
        if val is not None:
            sv = summarise_validation(res, val["rollouts"])
            s.update(sv)
            log(f"{cost}: plans under {int(val['rollouts'])} fresh noise rows, mean collision probability = "
                f"{sv['p_collision'][0]:.4f} +- {sv['p_collision'][1]:.4f}, mean validated CVaR(obs) = "
                f"{sv['cvar_obs'][0]:.4f} +- {sv['cvar_obs'][1]:.4f}, mean solver cost_obs = "
                f"{sv['est_obs'][0]:.4f} +- {sv['est_obs'][1]:.4f}")
        if routed is not None:
            sr = summarise_vehicles(res, routed)
            s.update(sr)
            log(f"{cost}: routed vehicles, mean speed = {sr['vehicle_speed'][0]:.4f} +- {sr['vehicle_speed'][1]:.4f} "
                f"m/s, smallest bumper gap = {sr['min_gap']:.4f} m, ticks with the ego as a leader = {sr['ego_led']}")
        results[cost] = (res, s)
    return results


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="closed-loop CARLA episodes on the surrogate world")
    ap.add_argument("--synthetic", action="store_true", help="the synthetic route and spawns of replay.py")
    ap.add_argument("--town", default="Town05")
    ap.add_argument("--episodes", type=int, default=8)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--costs", nargs="+", default=["mmd", "cvar", "det"], choices=sorted(COSTS))
    ap.add_argument("--host-step", action="store_true", help="solve tick by tick and step the world on the host (mpcmmd_world_step_host)")
    ap.add_argument("--start-spread", type=float, default=0.0, metavar="S")
    ap.add_argument("--out", default="stats_carla")
    ap.add_argument("--num-reduced", type=int, default=10)
    ap.add_argument("--num-obs", type=int, default=3)
    ap.add_argument("--num-prime", type=int, default=60)
    ap.add_argument("--num-path", type=int, default=600)
    ap.add_argument("--noise", default="gaussian", choices=["gaussian", "beta"])
    ap.add_argument("--noise-level", type=float, default=0.1)
    ap.add_argument("--acc-const-noise", type=float, default=0.0)
    ap.add_argument("--steer-const-noise", type=float, default=0.0)
    ap.add_argument("--num-batch", type=int, default=100)
    ap.add_argument("--maxiter-cem", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--validate", type=int, default=None, metavar="R",
                    help="also roll every tick's plan out under R fresh noise rows (Monte-Carlo risk of the plans)")
    ap.add_argument("--alpha", type=float, default=0.98, help="quantile level of the validated VaR / CVaR")
    ap.add_argument("--risk-sigma", type=float, nargs="*", default=[], metavar="s", help="MMD bandwidths (at most 8)")
    ap.add_argument("--vehicles", default="parked", choices=["parked", "routed"],
                    help="routed: the vehicles follow the route with car-following (DESIGN.md section 24)")
    ap.add_argument("--speed-limit", type=float, default=SPEED_LIMIT, metavar="V",
                    help="speed limit of the routed vehicles in m/s; each drives 40 or 60 per cent below it")
    a = ap.parse_args(argv)
    if not a.synthetic:
        ap.error("only --synthetic worlds are built in")
    return a


def main(argv=None):
    a = parse_args(argv)
    if sys.path[0] != _HERE:
        sys.path.insert(0, _HERE)
    from optimizer import cem
    route, goal_index, vehicles = synthetic_world(a.town)
    prob = cem.CEM(a.num_reduced, 1, a.num_obs, a.noise_level, a.num_prime, a.noise, a.town, a.acc_const_noise,
                   a.steer_const_noise, num_batch=a.num_batch, maxiter_cem=a.maxiter_cem, seed=a.seed,
                   max_configs=a.episodes)
    kw = {} if a.validate is None else dict(validate=dict(rollouts=a.validate, alpha=a.alpha, sigma=a.risk_sigma))
    starts = synthetic_starts(route, a.episodes, a.start_spread)
    if a.vehicles == "routed":
        kw["routed"] = routed_traffic(route, starts, a.town, a.speed_limit)
    closed_loop(prob, a.costs, route, goal_index, vehicles, starts, a.ticks, a.out, num_path=a.num_path, v_des=V_DES, seed=a.seed, chained=not a.host_step,
                device_step=False, **kw)
    prob.close()


if __name__ == "__main__":
    main()
