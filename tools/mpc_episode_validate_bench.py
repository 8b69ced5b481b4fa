"""Closed-loop episodes of the synthetic variants with the validation stage: what the Monte-Carlo
risk of every tick's plan costs inside the chained loop -- in-line and on the side stream -- and
what it costs from the host (GPU box).

    python tools/mpc_episode_validate_bench.py [--E 1 2 8] [--n 10] [--costs cvar mmd_opt] [--ticks 30]
        [--reps 5] [--rollouts 1000] [--sigma 0.1] [--variant static] [--parent-lib PATH]
        [--out profiles/mpc_episode_validate_bench.json]

For every cost at B = 100, H = 30, O = 10 on the scenes of ``optimizer.closed_loop`` (episode e =
configuration e of the sweep's generator, given variates) and every number of episodes E, the wall
time of ``CEM.run_episodes`` over ``--ticks`` ticks, end to end (model, start, loop, logs),
divided by the ticks -- the method of ``mpc_episode_bench.py``: one warm-up of each route, then
``--reps`` runs with the routes alternating, median with min and max:

  chained          ``chained=True`` without validation
  chained_inline   ``chained=True, validate=dict(..., overlap=False)``: the stage on the handle's
                   stream between the CEM iterations and k_mpc_step
  chained_overlap  ``chained=True, validate=dict(..., overlap=True)``: k_mpc_validate_prep on the
                   handle's stream, the validators on the context's side stream
  host_val         ``chained=False, device_step=None, validate=...``: per tick the solve,
                   ``validate`` and ``validate_risk`` from the host, and the host step
  host             the same without ``validate`` (what the validators add to that route)

All in one process.  ``--parent-lib`` adds the regression check: the ``chained`` column alone and
``bench.py --gpus 1 --steps 100 --warmup 5``, each in three fresh processes in the order parent
library, this tree's, parent library (``MPCMMD_LIB`` selects it; the parent's lacks the new entry
points, which neither calls).  The clock state (the sysfs DPM tables and performance level of every
card, read only) is recorded before and after.  Prints one JSON line and writes it to ``--out``.
Only figures of one session compare.
"""
import argparse
import glob
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "mpc-mmd_amd")]

B, H, O, T = 100, 30, 10, 20
COLUMNS = ("chained", "chained_inline", "chained_overlap", "host_val", "host")


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


def measure(cem, CL, variant, cost, n, E, ticks, reps, val, columns):
    prob = cem.CEM(n, O, 0.1, H, "gaussian", 0.0, 0.0, num_batch=B, variant=variant, maxiter_cem=T, max_configs=E)
    vehicles, keys = CL.scenario(variant, E, O)
    starts = CL.starts_of(variant, E)
    u = np.random.default_rng(0).standard_normal((ticks, E, 3))
    kw = dict(u=u, keys=keys)
    host = dict(chained=False, device_step=None)
    route_kw = dict(chained=dict(chained=True),
                    chained_inline=dict(chained=True, validate=dict(val, overlap=False)),
                    chained_overlap=dict(chained=True, validate=dict(val, overlap=True)),
                    host_val=dict(host, validate=val), host=host)
    times = {c: [] for c in columns}
    for rep in range(reps + 1):
        for c in columns:
            prob.handle.sync()
            t0 = time.perf_counter()
            prob.run_episodes(cost, vehicles, starts, ticks, **kw, **route_kw[c])
            times[c].append((time.perf_counter() - t0) * 1e3 / ticks)
    prob.handle.close()
    row = dict(cost=cost, n=n, E=E, ticks=ticks, reps=reps)
    row.update({c + "_ms_per_tick": _stats(times[c][1:]) for c in columns})
    print(json.dumps(row), file=sys.stderr, flush=True)   # progress; the result line goes to stdout
    return row


def run_rows(a, columns):
    from optimizer import cem, closed_loop as CL
    val = dict(rollouts=a.rollouts, alpha=0.98, sigma=a.sigma)
    return [measure(cem, CL, a.variant, cost, a.n, E, a.ticks, a.reps, val, columns) for cost in a.costs for E in a.E]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--E", type=int, nargs="+", default=[1, 2, 8])
    ap.add_argument("--n", type=int, default=10)
    ap.add_argument("--costs", nargs="+", default=["cvar", "mmd_opt"])
    ap.add_argument("--ticks", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rollouts", type=int, default=1000)
    ap.add_argument("--sigma", type=float, nargs="*", default=[0.1])
    ap.add_argument("--variant", default="static", choices=["static", "dynamic"])
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libmpcmmd.so: adds parent / child / parent")
    ap.add_argument("--chained-only", action="store_true", help="(internal) the chained column alone, rows as JSON")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mpc_episode_validate_bench.json"))
    a = ap.parse_args()
    if a.chained_only:
        print(json.dumps(run_rows(a, ("chained",))))
        return
    out = dict(tool="mpc_episode_validate_bench", variant=a.variant, B=B, H=H, O=O, maxiter_cem=T, rollouts=a.rollouts,
               sigma=a.sigma, clocks_before=clock_state())
    out["rows"] = run_rows(a, COLUMNS)
    if a.parent_lib:
        # fresh processes, the library chosen by MPCMMD_LIB: parent, this tree's, parent
        chained = [sys.executable, os.path.abspath(__file__), "--chained-only", "--n", str(a.n), "--ticks", str(a.ticks),
                   "--reps", str(a.reps), "--variant", a.variant, "--E", *map(str, a.E), "--costs", *a.costs]
        bench = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "100", "--warmup", "5"]
        child_lib = os.path.join(ROOT, "mpc-mmd_amd", "libmpcmmd.so")
        order = (("parent_a", a.parent_lib), ("child", child_lib), ("parent_b", a.parent_lib))
        out["regression"], out["regression_bench"] = [], []
        for name, argv in (("regression", chained), ("regression_bench", bench)):
            for who, lib in order:
                r = subprocess.run(argv, env={**os.environ, "MPCMMD_LIB": os.path.abspath(lib)}, check=True,
                                   stdout=subprocess.PIPE, text=True, cwd=ROOT)
                got = json.loads(r.stdout.strip().split("\n")[-1])
                if name == "regression_bench":
                    got = {k: got[k] for k in ("metric", "value", "unit", "median_ms_per_step") if k in got}
                    out[name].append(dict(library=who, line=got))
                else:
                    out[name].append(dict(library=who, rows=got))
                print(json.dumps(out[name][-1]), file=sys.stderr, flush=True)
    out["clocks_after"] = clock_state()
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
