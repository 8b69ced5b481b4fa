"""Closed-loop CARLA episodes with the validation stage: what the Monte-Carlo risk of every
tick's plan costs inside the chained loop, and what it costs from the host (GPU box).

    python tools/carla_episode_validate_bench.py [--E 1 2 8] [--n 10] [--costs cvar mmd] [--ticks 40]
        [--reps 5] [--rollouts 1000] [--sigma 0.1] [--parent-lib PATH]
        [--out profiles/carla_episode_validate_bench.json]

For every cost at B = 100, H = 60, O = 3, num_path = 600 on the synthetic
Town05 world of ``closed_loop.py`` and every number of episodes E, the wall
time of ``CEM.run_episodes`` over ``--ticks`` ticks, end to end (world model,
start, loop, logs), divided by the ticks -- the method of
``carla_episode_bench.py``: one warm-up of each route, then ``--reps`` runs with
the routes alternating, median with min and max:

  chained      ``chained=True`` without validation
  chained_val  ``chained=True, validate=dict(rollouts=R, sigma=...)``: the stage
               inside the loop (mpcmmd_world_validate)
  host_val     ``device_step=False, validate=...``: per tick the solve, the
               readback of obs and path, ``validate_carla_risk`` from the host
               and the host world step

All three in one process.  ``--parent-lib`` adds the regression check: the
``chained`` column alone, measured in three fresh processes in the order parent
library, this tree's, parent library (``MPCMMD_LIB`` selects it; the parent's
lacks the new entry points, which this column does not call).  The clock state
(the sysfs DPM tables and performance level of every card, read only) is
recorded before and after.  Prints one JSON line and writes it to ``--out``.
Only figures of one session compare.
"""
import argparse
import glob
import importlib.util
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CARLA = os.path.join(ROOT, "mpc-mmd_amd", "carla")
sys.path[:0] = [CARLA]

B, H, O, T, P = 100, 60, 3, 20, 600
COLUMNS = ("chained", "chained_val", "host_val")


def _stats(ms):
    return dict(median=round(statistics.median(ms), 4), min=round(min(ms), 4), max=round(max(ms), 4))


def clock_state():
    """The current shader / memory clock rows and the performance level of every card, from sysfs."""
    out = {}
    for dev in sorted(glob.glob("/sys/class/drm/card*/device")):
        row = {}
        for name in ("pp_dpm_sclk", "pp_dpm_mclk", "power_dpm_force_performance_level"):
            try:
                with open(os.path.join(dev, name)) as f:
                    lines = f.read().split("\n")
                cur = [ln.strip() for ln in lines if ln.strip().endswith("*")]
                row[name] = cur if cur else [ln.strip() for ln in lines if ln.strip()][:4]
            except OSError:
                pass
        if row:
            out[os.path.basename(os.path.dirname(dev))] = row
    return out or "unavailable"


def measure(cem, CL, cost, n, E, ticks, reps, val, columns):
    prob = cem.CEM(n, 1, O, 0.1, H, "gaussian", "Town05", 0.0, 0.0, num_batch=B, maxiter_cem=T, max_configs=E)
    route, goal, vehicles = CL.synthetic_world("Town05")
    starts = CL.synthetic_starts(route, E, spread=4.0 * E, v0=3.0)
    u = np.random.default_rng(0).standard_normal((ticks, E, 4))
    kw = dict(goal_index=goal, num_path=P, u=u)
    route_kw = dict(chained=dict(chained=True), chained_val=dict(chained=True, validate=val),
                    host_val=dict(chained=False, device_step=False, validate=val))
    times = {c: [] for c in columns}
    for rep in range(reps + 1):
        for c in columns:
            prob.handle.sync()
            t0 = time.perf_counter()
            prob.run_episodes(cost, route, vehicles, starts, ticks, **kw, **route_kw[c])
            times[c].append((time.perf_counter() - t0) * 1e3 / ticks)
    prob.close()
    row = dict(cost=cost, n=n, E=E, ticks=ticks, reps=reps)
    row.update({c + "_ms_per_tick": _stats(times[c][1:]) for c in columns})
    print(json.dumps(row), file=sys.stderr, flush=True)   # progress; the result line goes to stdout
    return row


def run_rows(a, columns):
    from optimizer import cem
    spec = importlib.util.spec_from_file_location("mpcmmd_carla_closed_loop", os.path.join(CARLA, "closed_loop.py"))
    CL = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(CL)
    val = dict(rollouts=a.rollouts, alpha=0.98, sigma=a.sigma)
    return [measure(cem, CL, cost, a.n, E, a.ticks, a.reps, val, columns) for cost in a.costs for E in a.E]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--E", type=int, nargs="+", default=[1, 2, 8])
    ap.add_argument("--n", type=int, default=10)
    ap.add_argument("--costs", nargs="+", default=["cvar", "mmd"])
    ap.add_argument("--ticks", type=int, default=40)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rollouts", type=int, default=1000)
    ap.add_argument("--sigma", type=float, nargs="*", default=[0.1])
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libmpcmmd.so: adds parent / child / parent")
    ap.add_argument("--chained-only", action="store_true", help="(internal) the chained column alone, rows as JSON")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "carla_episode_validate_bench.json"))
    a = ap.parse_args()
    if a.chained_only:
        print(json.dumps(run_rows(a, ("chained",))))
        return
    out = dict(tool="carla_episode_validate_bench", B=B, H=H, O=O, num_path=P, maxiter_cem=T, rollouts=a.rollouts,
               sigma=a.sigma, clocks_before=clock_state())
    out["rows"] = run_rows(a, COLUMNS)
    if a.parent_lib:
        # fresh processes, the library chosen by MPCMMD_LIB: parent, this tree's, parent
        argv = [sys.executable, os.path.abspath(__file__), "--chained-only", "--n", str(a.n), "--ticks", str(a.ticks),
                "--reps", str(a.reps), "--E", *map(str, a.E), "--costs", *a.costs]
        child_lib = os.path.join(ROOT, "mpc-mmd_amd", "libmpcmmd.so")
        out["regression"] = []
        for who, lib in (("parent_a", a.parent_lib), ("child", child_lib), ("parent_b", a.parent_lib)):
            r = subprocess.run(argv, env={**os.environ, "MPCMMD_LIB": os.path.abspath(lib)}, check=True,
                               stdout=subprocess.PIPE, text=True)
            out["regression"].append(dict(library=who, rows=json.loads(r.stdout.strip().split("\n")[-1])))
    out["clocks_after"] = clock_state()
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
