"""Closed-loop CARLA episodes: the chained route against the host-stepped route (GPU box).

    python tools/carla_episode_bench.py [--E 1 2 8] [--n 10] [--costs cvar mmd] [--ticks 40] [--reps 5]
                                        [--out profiles/carla_episode_bench.json]

For every cost at B = 100, H = 60, O = 3, num_path = 600 on the synthetic
Town05 world of ``closed_loop.py`` and every number of episodes E, the wall
time of ``CEM.run_episodes`` over ``--ticks`` ticks, end to end and the same
call on both sides -- the world model, the start (tick 0's inputs), the loop
and the log -- divided by the ticks (median of ``--reps`` runs after one
warm-up of each route, with min and max):

  chained  ``chained=True``: World create and reset, ``World.run(0, ticks)``
           (begin, CEM and k_world_step enqueued per tick, nothing crossing the
           host), ``World.log``
  host     ``chained=False, device_step=False``: per tick ``Tick.solve_batch``
           (mpcmmd_carla_tick_solve_batch, results read back) and
           ``world_step`` on the host (mpcmmd_world_step_host)

The route's splines are fitted once per optimizer (``CEM.world_model`` keeps the
last route's), before the warm-up, so neither side pays for them.  Both routes
produce the same bits (tests/test_gpu_closed_loop.py).  Prints one JSON line
and writes it to ``--out``.  Only figures of one session compare.
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


def _stats(ms):
    return dict(median=round(statistics.median(ms), 4), min=round(min(ms), 4), max=round(max(ms), 4))


def measure(cem, CL, cost, n, E, ticks, reps):
    prob = cem.CEM(n, 1, O, 0.1, H, "gaussian", "Town05", 0.0, 0.0, num_batch=B, maxiter_cem=T, max_configs=E)
    route, goal, vehicles = CL.synthetic_world("Town05")
    starts = CL.synthetic_starts(route, E, spread=4.0 * E, v0=3.0)
    u = np.random.default_rng(0).standard_normal((ticks, E, 4))
    kw = dict(goal_index=goal, num_path=P, u=u)
    chained, host = [], []
    for rep in range(reps + 1):
        for times, route_kw in ((chained, dict(chained=True)), (host, dict(chained=False, device_step=False))):
            prob.handle.sync()
            t0 = time.perf_counter()
            prob.run_episodes(cost, route, vehicles, starts, ticks, **kw, **route_kw)
            times.append((time.perf_counter() - t0) * 1e3 / ticks)
    prob.close()
    return dict(cost=cost, n=n, E=E, ticks=ticks, reps=reps, chained_ms_per_tick=_stats(chained[1:]),
                host_ms_per_tick=_stats(host[1:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--E", type=int, nargs="+", default=[1, 2, 8])
    ap.add_argument("--n", type=int, default=10)
    ap.add_argument("--costs", nargs="+", default=["cvar", "mmd"])
    ap.add_argument("--ticks", type=int, default=40)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "carla_episode_bench.json"))
    a = ap.parse_args()
    from optimizer import cem
    spec = importlib.util.spec_from_file_location("mpcmmd_carla_closed_loop", os.path.join(CARLA, "closed_loop.py"))
    CL = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(CL)
    rows = [measure(cem, CL, cost, a.n, E, a.ticks, a.reps) for cost in a.costs for E in a.E]
    out = dict(tool="carla_episode_bench", B=B, H=H, O=O, num_path=P, maxiter_cem=T, rows=rows)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
