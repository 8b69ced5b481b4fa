"""Closed-loop MPC episodes of the synthetic variants.

``optimizer.sweep`` solves every configuration once from a standing start and
``optimizer.validation`` scores that open-loop plan.  Here the plan moves an
ego: each tick the plan's first control is perturbed by the noise model and
applied, the ego and the vehicles move, and the next tick is solved from where
the ego ended up, warm-started from the previous mean (``CEM.run_episodes``).
The world is the optimizer's own rollout model with one realised draw.  E
independent episodes run in lockstep on one batch handle; by default the whole
loop is enqueued on the GPU (mpcmmd_mpc_run: per tick the chained begin, the
CEM iterations and k_mpc_step, nothing crossing the host, one readback of the
log at the end).  With ``--host-step`` each tick is one batched solve
(mpcmmd_solve_batch) and one host step (mpcmmd_mpc_step_host); the files are
equal.

    cd mpc-mmd_amd
    python -m optimizer.closed_loop --variant static --episodes 8 --ticks 100 \\
        --costs mmd_opt mmd_random cvar saa --out stats

Episode e is configuration e of the sweep's scenario generator
(``sweep.obstacles``): its obstacle positions and, for the dynamic variant, the
generator's initial velocities.  By default (``--vehicles constant``) the world
keeps those velocities constant; with ``--vehicles planned`` every vehicle follows
the dynamic generator's lane-tracking QP and re-plans it each tick from its own
state towards the driver's targets: the tracked speed
``obs_data(1).sampling_param(43 e + 11 o + 5)[0]`` of vehicle o of episode e, the
driver's seeds, and the lane y = -1.75 -- the cut-in of the dynamic driver, whose
tick-0 tracks are then the sweep's own.  The npz then also holds ``veh``
[T, E, O, 6], every vehicle's (x, y, vx, vy, ax, ay) after each tick, and one more
line per cost gives the share of vehicles inside |y + 1.75| < 0.5 at their
episode's last live tick.  The ego starts as the sweep starts it.  Episodes also differ by their key (the solver's streams and the
perturbation's variates, which the library draws after each tick's solve:
normals, or Beta(2 |control|, 5 |control|) with ``--noise beta``).  Per cost
``closed_loop_<cost>.npz`` holds ``log_d`` [T, E, 2] (x, y), ``log_f`` [T, E, 12]
(vx, vy, psi, a_c, s_c, a, s, u[3], clear, curv), ``log_i`` [T, E, 4] (lane_out,
collided, goal, frozen), every tick's ``cx``, ``cy`` [T, E, 11] and ``mean``
[T, E, 8], and ``done_tick`` [E]; one line per cost gives the collision share,
the mean minimum -clear, the lane-departure share and the mean progress in x,
each as mean +- sample standard deviation over the episodes.

With ``--validate R [--alpha A] [--risk-sigma s ...] [--no-overlap]`` every
tick's plan is also rolled out under R fresh noise rows from the tick's state
against the tick's tracks: inside the chained loop on the
GPU, on a side stream unless ``--no-overlap`` puts it in-line, or, with
``--host-step``, by mpcmmd_validate and mpcmmd_validate_risk after each tick's
solve -- the same bits again.  The npz then also holds ``val_counts`` [T, E, 2]
(count, count_lane), ``val_count_pos`` [T, E, 3], ``val_stats`` [T, E, 4, 3]
(var, cvar, mean, max by obs, lane_lb, lane_ub), ``val_mmd`` [T, E, 3, S] and
``val_est`` [T, E, 2] (the cost_lane, cost_obs the solve estimated), and a second
line per cost gives, over the live (tick, episode) pairs, the mean Monte-Carlo
collision probability count_pos[obs] / R, the mean count / R (the reference's
coll_* metric) and the mean validated CVaR of the obstacle cost beside the mean
of the solver's own cost_obs.

With ``--slots E`` and more episodes than slots the run is a campaign
(``CEM.run_campaign``): the N scenes go through E slots of
the chained loop, a slot refilled on the GPU as soon as its episode ends, so no
solve works on a finished episode while scenes are left.  The lines and the
files are the same, now over N scenes (every scene's rows equal those of the
scene run alone; the rows after a scene's end repeat its last row), and one more
line gives the lockstep ticks the campaign took.  The chained route only, and
without ``--validate``.

The episode runner is a parameter of ``closed_loop`` (``run=``), so the
accounting is testable without a GPU.
"""
from __future__ import annotations

import argparse
import os

import numpy as np

from .episode_stats import mean_std as _mean_std

COSTS = ("mmd_opt", "mmd_random", "cvar", "saa")
KEYS = ("log_d", "log_f", "log_i", "cx", "cy", "mean", "done_tick")
VAL_KEYS = ("val_counts", "val_count_pos", "val_stats", "val_mmd", "val_est")
CLEAR, LANE_OUT, COLLIDED = 10, 0, 1   # columns of log_f / log_i (_native.MPC_LOG_F / _I)


def scenario(variant, episodes, num_obs):
    """vehicles [E, num_obs, 4] = x, y, vx, vy and keys [E]: configuration e of the sweep's generator."""
    from .sweep import obstacles
    veh = np.zeros((episodes, num_obs, 4), np.float32)
    keys = np.zeros(episodes, np.int64)
    for e in range(episodes):
        ob = obstacles(variant, e, num_obs)
        veh[e] = np.stack([np.asarray(ob[k], np.float64).reshape(num_obs) for k in ("x", "y", "vx", "vy")], 1)
        keys[e] = int(ob["idx_mpc"])
    return veh, keys


def vehicle_targets(episodes, num_obs):
    """[E, num_obs, 2] = v_des, y_des of the planned vehicles: the dynamic driver's seeds
    (``dynamic_obstacles``: 43 k + 11 tt + 5) and its target lane."""
    from .obs_data_generate_dynamic import obs_data
    gen = obs_data(1)
    tg = np.empty((episodes, num_obs, 2), np.float32)
    for e in range(episodes):
        for o in range(num_obs):
            tg[e, o] = gen.sampling_param(43 * e + 11 * o + 5)[0], -1.75
    return tg


def summarise_vehicles(res, half_width=0.5, lane=-1.75):
    """(mean, sample sd) over the episodes of the share of an episode's vehicles inside
    |y - lane| < half_width at the episode's last live tick."""
    veh = np.asarray(res["veh"])
    T, E = veh.shape[:2]
    done = np.asarray(res["done_tick"])
    last = np.where(done >= 0, done, T - 1)
    y = veh[last, np.arange(E), :, 1] if T and veh.shape[2] else np.zeros((E, 0))
    inside = np.abs(y.astype(np.float64) - lane) < half_width
    return dict(in_lane=_mean_std(inside.mean(axis=1) if inside.shape[1] else np.zeros(E)))


def starts_of(variant, episodes):
    """[E, 4] = x, y, vx, vy: the sweep's standing start (sweep.main)."""
    y0 = 1.75 if variant == "static" else -1.75
    return np.tile(np.array([0.0, y0, 5.0, 0.0]), (episodes, 1))


def _run(prob, cost, vehicles, starts, ticks, **kw):
    return prob.run_episodes(cost, vehicles, starts, ticks, **kw)


def campaign_runner(slots, log=print):
    """A ``run=`` of ``closed_loop`` that puts the scenes through ``slots`` slots (``CEM.run_campaign``)."""
    def run(prob, cost, vehicles, starts, ticks, chained=True, device_step=None, validate=None, **kw):
        if chained is not True or validate is not None:
            raise ValueError("a campaign (--slots) runs on the chained route, without --validate")
        res = prob.run_campaign(cost, vehicles, starts, ticks, slots=slots, **kw)
        n = np.asarray(res["done_tick"]).size
        log(f"{cost}: campaign of {n} scenes through {slots} slots, {res['lockstep_ticks']} lockstep ticks "
            f"({res['finished']} finished; {-(-n // slots) * int(ticks)} in batches of {slots})")
        return res
    return run


def summarise(res):
    """The four figures of one cost's episodes, each (mean, sample sd) over the
    episodes.  Rows after an episode's ``done_tick`` repeat its frozen state and
    are left out."""
    log_f, log_i, log_d = res["log_f"], res["log_i"], res["log_d"]
    T, E = log_i.shape[:2]
    done = np.asarray(res["done_tick"])
    last = np.where(done >= 0, done, T - 1)
    live = np.arange(T)[:, None] <= last[None, :]
    neg_clear = np.where(live, -log_f[:, :, CLEAR].astype(np.float64), np.inf)
    return dict(collision=_mean_std((log_i[:, :, COLLIDED].astype(bool) & live).any(axis=0).astype(float)),
                min_neg_clear=_mean_std(neg_clear.min(axis=0) if T else np.zeros(E)),
                lane_departure=_mean_std((log_i[:, :, LANE_OUT].astype(bool) & live).any(axis=0).astype(float)),
                progress=_mean_std(log_d[last, np.arange(E), 0] - log_d[0, :, 0] if T else np.zeros(E)))


def summarise_validation(res, rollouts):
    """The four figures of one cost's validated plans, each (mean, sample sd)
    over the episodes of the episode's mean over its live ticks (``summarise``'s
    convention: rows after ``done_tick`` are left out): the Monte-Carlo collision
    probability count_pos[obs] / R, the reference's count / R, the validated
    CVaR of the obstacle cost, and the obstacle cost the solver estimated."""
    T, E = res["val_counts"].shape[:2]
    done = np.asarray(res["done_tick"])
    last = np.where(done >= 0, done, T - 1)
    live = np.arange(T)[:, None] <= last[None, :]
    n = np.maximum(live.sum(axis=0), 1)
    per_episode = lambda a: np.where(live, np.asarray(a, np.float64), 0.0).sum(axis=0) / n
    return dict(p_collision=_mean_std(per_episode(res["val_count_pos"][:, :, 0] / float(rollouts))),
                count_share=_mean_std(per_episode(res["val_counts"][:, :, 0] / float(rollouts))),
                cvar_obs=_mean_std(per_episode(res["val_stats"][:, :, 1, 0])),
                est_obs=_mean_std(per_episode(res["val_est"][:, :, 1])))


def closed_loop(prob, costs, vehicles, starts, ticks, out_dir=None, run=None, log=print, **kw):
    """Runs ``run(prob, cost, vehicles, starts, ticks, **kw)`` (default:
    ``prob.run_episodes``) per cost, writes the files and prints the lines of
    the module docstring.  Returns {cost: (the result, its summary)}."""
    run = run or _run
    val = kw.get("validate")
    planned = kw.get("planned") is not None
    keys = KEYS + (VAL_KEYS if val is not None else ()) + (("veh",) if planned else ())
    results = {}
    for cost in costs:
        if cost not in COSTS:
            raise ValueError(f"cost must be one of {sorted(COSTS)}")
        res = run(prob, cost, vehicles, starts, ticks, **kw)
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
                f"{sv['p_collision'][0]:.4f} +- {sv['p_collision'][1]:.4f}, mean count / R = "
                f"{sv['count_share'][0]:.4f} +- {sv['count_share'][1]:.4f}, mean validated CVaR(obs) = "
                f"{sv['cvar_obs'][0]:.4f} +- {sv['cvar_obs'][1]:.4f}, mean solver cost_obs = "
                f"{sv['est_obs'][0]:.4f} +- {sv['est_obs'][1]:.4f}")
        if planned:
            sp = summarise_vehicles(res)
            s.update(sp)
            log(f"{cost}: planned vehicles, share inside |y + 1.75| < 0.5 at the last live tick = "
                f"{sp['in_lane'][0]:.4f} +- {sp['in_lane'][1]:.4f}")
        results[cost] = (res, s)
    return results


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="closed-loop MPC episodes of the synthetic variants")
    ap.add_argument("--variant", default="static", choices=["static", "dynamic"])
    ap.add_argument("--episodes", type=int, default=8)
    ap.add_argument("--ticks", type=int, default=100)
    ap.add_argument("--slots", type=int, default=None, metavar="E",
                    help="with more episodes than E: a campaign through E slots, refilled on the GPU as episodes end")
    ap.add_argument("--costs", nargs="+", default=list(COSTS), choices=sorted(COSTS))
    ap.add_argument("--host-step", action="store_true",
                    help="solve tick by tick and step the world on the host (mpcmmd_mpc_step_host)")
    ap.add_argument("--vehicles", default="constant", choices=["constant", "planned"],
                    help="constant velocity, or every vehicle re-plans the dynamic driver's QP each tick (the veh array, "
                         "one more line)")
    ap.add_argument("--validate", type=int, default=None, metavar="R",
                    help="also roll every tick's plan out under R fresh noise rows (the val_* arrays, a second line)")
    ap.add_argument("--alpha", type=float, default=0.98, help="quantile level of the validated VaR / CVaR")
    ap.add_argument("--risk-sigma", type=float, nargs="*", default=[], metavar="s", help="MMD bandwidths (at most 8)")
    ap.add_argument("--no-overlap", action="store_true",
                    help="the validation stage in-line on the loop's stream (default: on a side stream; same bits)")
    ap.add_argument("--out", default="stats_closed_loop")
    ap.add_argument("--num-reduced", type=int, default=10)
    ap.add_argument("--num-obs", type=int, default=3)
    ap.add_argument("--num-prime", type=int, default=30)
    ap.add_argument("--noise", default="gaussian", choices=["gaussian", "beta"])
    ap.add_argument("--noise-level", type=float, default=0.1)
    ap.add_argument("--acc-const-noise", type=float, default=0.0)
    ap.add_argument("--steer-const-noise", type=float, default=0.0)
    ap.add_argument("--num-batch", type=int, default=100)
    ap.add_argument("--maxiter-cem", type=int, default=20)
    ap.add_argument("--v-des", type=float, default=15.0)
    ap.add_argument("--goal-x", type=float, default=200.0)
    ap.add_argument("--seed", type=int, default=0)
    return ap.parse_args(argv)


def validation_of(a):
    """The ``validate=`` keyword of the parsed options ({} without --validate)."""
    if a.validate is None:
        return {}
    return dict(validate=dict(rollouts=a.validate, alpha=a.alpha, sigma=a.risk_sigma, overlap=not a.no_overlap))


def planned_of(a):
    """The ``planned=`` keyword of the parsed options ({} without --vehicles planned)."""
    if a.vehicles != "planned":
        return {}
    return dict(planned=dict(target=vehicle_targets(a.episodes, a.num_obs), acc=None))


def main(argv=None):
    a = parse_args(argv)
    from .cem import CEM
    prob = CEM(a.num_reduced, a.num_obs, a.noise_level, a.num_prime, a.noise, a.acc_const_noise, a.steer_const_noise,
               num_batch=a.num_batch, variant=a.variant, maxiter_cem=a.maxiter_cem, seed=a.seed,
               max_configs=a.episodes if a.slots is None else min(a.slots, a.episodes))
    vehicles, keys = scenario(a.variant, a.episodes, a.num_obs)
    run = campaign_runner(a.slots) if a.slots is not None and a.episodes > a.slots else None
    try:
        closed_loop(prob, a.costs, vehicles, starts_of(a.variant, a.episodes), a.ticks, a.out, run=run, keys=keys,
                    v_des=a.v_des, goal_x=a.goal_x, chained=not a.host_step, device_step=None, **validation_of(a),
                    **planned_of(a))
    finally:
        prob.handle.close()


if __name__ == "__main__":
    main()
