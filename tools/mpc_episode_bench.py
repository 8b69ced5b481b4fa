"""Closed-loop episodes of the synthetic variants: the chained route against the host-stepped route (GPU box).

    python tools/mpc_episode_bench.py [--E 1 2 8] [--n 10] [--costs cvar mmd_opt] [--ticks 40] [--reps 5]
                                      [--variant static] [--out profiles/mpc_episode_bench.json]

For every cost at B = 100, H = 30, O = 10 on the scenes of
``optimizer.closed_loop`` (episode e = configuration e of the sweep's
generator) and every number of episodes E, the wall time of
``CEM.run_episodes`` over ``--ticks`` ticks, end to end and the same call on
both sides -- the model, the start (tick 0's inputs), the loop and the log --
divided by the ticks (median of ``--reps`` runs after one warm-up of each
route, with min and max):

  chained  ``chained=True``: Mpc create and reset, ``Mpc.run(0, ticks)`` (begin,
           CEM and k_mpc_step enqueued per tick, nothing crossing the host),
           ``Mpc.log``
  host     ``chained=False, device_step=None``: per tick ``Handle.solve_batch``
           (mpcmmd_solve_batch, results read back), ``Handle.read("mean")`` and
           ``mpc_step`` on the host (mpcmmd_mpc_step_host)

Both routes produce the same bits (tests/test_gpu_mpc_loop.py).  Prints one
JSON line and writes it to ``--out``.  Only figures of one session compare.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "mpc-mmd_amd")]

B, H, O, T = 100, 30, 10, 20


def _stats(ms):
    return dict(median=round(statistics.median(ms), 4), min=round(min(ms), 4), max=round(max(ms), 4))


def measure(cem, CL, variant, cost, n, E, ticks, reps):
    prob = cem.CEM(n, O, 0.1, H, "gaussian", 0.0, 0.0, num_batch=B, variant=variant, maxiter_cem=T, max_configs=E)
    vehicles, keys = CL.scenario(variant, E, O)
    starts = CL.starts_of(variant, E)
    u = np.random.default_rng(0).standard_normal((ticks, E, 3))
    kw = dict(u=u, keys=keys)
    chained, host = [], []
    for rep in range(reps + 1):
        for times, route_kw in ((chained, dict(chained=True)), (host, dict(chained=False, device_step=None))):
            prob.handle.sync()
            t0 = time.perf_counter()
            prob.run_episodes(cost, vehicles, starts, ticks, **kw, **route_kw)
            times.append((time.perf_counter() - t0) * 1e3 / ticks)
    prob.handle.close()
    return dict(cost=cost, n=n, E=E, ticks=ticks, reps=reps, chained_ms_per_tick=_stats(chained[1:]),
                host_ms_per_tick=_stats(host[1:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--E", type=int, nargs="+", default=[1, 2, 8])
    ap.add_argument("--n", type=int, default=10)
    ap.add_argument("--costs", nargs="+", default=["cvar", "mmd_opt"])
    ap.add_argument("--ticks", type=int, default=40)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--variant", default="static", choices=["static", "dynamic"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mpc_episode_bench.json"))
    a = ap.parse_args()
    from optimizer import cem, closed_loop as CL
    rows = [measure(cem, CL, a.variant, cost, a.n, E, a.ticks, a.reps) for cost in a.costs for E in a.E]
    out = dict(tool="mpc_episode_bench", variant=a.variant, B=B, H=H, O=O, maxiter_cem=T, rows=rows)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
