"""The chained CARLA closed loop with parked, routed-but-parked and routed vehicles (GPU box).

    python tools/carla_vehicle_bench.py [--E 1 8] [--n 10] [--costs cvar mmd] [--ticks 40] [--reps 7]
                                        [--episode-ticks 200] [--out profiles/carla_vehicle_bench.json]

For every cost at B = 100, H = 60, O = 3, num_path = 600 on the synthetic Town05
world of ``carla/closed_loop.py`` and every number of episodes E, the wall time
of the loop proper -- ``World.run(0, ticks)`` and the synchronisation behind it,
after the context's create, ``route_vehicles`` and reset -- divided by the ticks:
per tick the chained begin, the CEM iterations and one k_world_step, which with
the policy on is the routed instantiation.  Three sides
alternate on the same handle, one context each:

  off      the policy off: the parked vehicles of the scene, constant velocity 0
  parked   the policy on, every vehicle at its spawn with target speed 0: nothing
           moves, the solves see the scene of ``off`` (to the rounding of the rows,
           which now come from the splines), so the difference is the step's own cost
  traffic  the policy on with the command line's traffic (``routed_traffic``): the
           vehicles drive, so the solves work on other obstacles and episodes end
           elsewhere; the difference is the scene's, not the step's

Median of ``--reps`` runs after one warm-up of each, with min and max, and the
differences of the medians.  Then, per cost, what the traffic does to the
episodes: ``closed_loop.summarise`` of 8 episodes of ``--episode-ticks`` ticks on
``off`` and on ``traffic`` (collision share, lane departure share, mean progress,
with the vehicles' line of ``summarise_vehicles``).  Prints one JSON line and
writes it to ``--out``.  Only figures of one session compare.
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CARLA = os.path.join(ROOT, "mpc-mmd_amd", "carla")
sys.path[:0] = [CARLA]

B, H, O, T, P = 100, 60, 3, 20, 600
KIND = {"mmd": "mmd_opt", "cvar": "cvar", "det": "det"}


def _closed_loop():
    spec = importlib.util.spec_from_file_location("mpcmmd_carla_closed_loop", os.path.join(CARLA, "closed_loop.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _stats(ms):
    return dict(median=round(statistics.median(ms), 4), min=round(min(ms), 4), max=round(max(ms), 4))


def measure(cem, native, CL, cost, n, E, ticks, reps):
    prob = cem.CEM(n, 1, O, 0.1, H, "gaussian", "Town05", 0.0, 0.0, num_batch=B, maxiter_cem=T, max_configs=E)
    route, goal, vehicles = CL.synthetic_world("Town05")
    starts = CL.synthetic_starts(route, E, spread=4.0 * E, v0=3.0)
    f32 = np.float32
    cov = np.diag([20.0] * 4 + [100.0] * 4).astype(f32)
    mean = np.tile(np.array([CL.V_DES] * 4 + [0.0] * 4, f32), (E, 1))
    ego = np.stack([starts[:, 2], starts[:, 3], np.zeros(E)], 1)
    u = np.random.default_rng(0).standard_normal((ticks, E, 4)).astype(f32)
    keys = CL.KEY_STRIDE * np.arange(E)
    model, tk = prob.world_model(route, vehicles.shape[0], goal, P, cov)
    traffic = CL.routed_traffic(route, starts)
    parked = CL.routed_traffic(route, np.zeros((E, 4)))   # the scene's own spawns, nobody's target above 0
    parked["v0"][:] = 0.0
    sides = {}
    for name, rt in (("off", None), ("parked", parked), ("traffic", traffic)):
        ctx = native.World(tk, model, ticks)
        if rt is not None:
            ctx.route_vehicles(rt["s"], rt["v"], np.stack([rt["d"], rt["v0"]], -1))
        sides[name] = (ctx, [])
    for rep in range(reps + 1):
        for name, (ctx, times) in sides.items():
            ctx.reset(starts[:, :2], ego, None if name != "off" else np.tile(vehicles[None], (E, 1, 1)), mean, cov, u, keys)
            prob.handle.sync()
            t0 = time.perf_counter()
            ctx.run(KIND[cost], 0, ticks, cov, CL.V_DES)
            prob.handle.sync()
            times.append((time.perf_counter() - t0) * 1e3 / ticks)
    live = {name: int((ctx.log(ticks)["done_tick"] < 0).sum()) for name, (ctx, _) in sides.items()}
    for ctx, _ in sides.values():
        ctx.close()
    prob.close()
    off, park, on = (_stats(sides[name][1][1:]) for name in ("off", "parked", "traffic"))
    return dict(cost=cost, n=n, E=E, ticks=ticks, reps=reps, off_ms_per_tick=off, parked_ms_per_tick=park,
                traffic_ms_per_tick=on, parked_minus_off_ms=round(park["median"] - off["median"], 4),
                traffic_minus_off_ms=round(on["median"] - off["median"], 4), live_episodes_at_end=live)


def episodes(cem, CL, cost, n, ticks, E=8):
    """What the traffic does to E episodes of `ticks` ticks: the command line's figures on both scenes."""
    prob = cem.CEM(n, 1, O, 0.1, H, "gaussian", "Town05", 0.0, 0.0, num_batch=B, maxiter_cem=T, max_configs=E)
    route, goal, vehicles = CL.synthetic_world("Town05")
    starts = CL.synthetic_starts(route, E)
    out = dict(cost=cost, n=n, E=E, ticks=ticks)
    for name, kw in (("off", {}), ("traffic", dict(routed=CL.routed_traffic(route, starts)))):
        res, s = CL.closed_loop(prob, [cost], route, goal, vehicles, starts, ticks, None, log=lambda line: None,
                                num_path=P, v_des=CL.V_DES, chained=True, **kw)[cost]
        out[name] = {k: ([round(x, 4) for x in v] if isinstance(v, tuple) else v) for k, v in s.items()}
        out[name]["done_tick"] = [int(x) for x in res["done_tick"]]
    prob.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--E", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--n", type=int, default=10)
    ap.add_argument("--costs", nargs="+", default=["cvar", "mmd"], choices=sorted(KIND))
    ap.add_argument("--ticks", type=int, default=40)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--episode-ticks", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "carla_vehicle_bench.json"))
    a = ap.parse_args()
    from optimizer import cem
    from optimizer._lib import native
    CL = _closed_loop()
    rows = [measure(cem, native(), CL, cost, a.n, E, a.ticks, a.reps) for cost in a.costs for E in a.E]
    eps = [episodes(cem, CL, cost, a.n, a.episode_ticks) for cost in a.costs] if a.episode_ticks > 0 else []
    out = dict(tool="carla_vehicle_bench", town="Town05", B=B, H=H, O=O, num_path=P, maxiter_cem=T, rows=rows,
               episodes=eps)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
