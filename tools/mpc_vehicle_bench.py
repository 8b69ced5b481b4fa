"""The chained closed loop of the dynamic variant with constant-velocity and with planned vehicles (GPU box).

    python tools/mpc_vehicle_bench.py [--E 1 8] [--n 10] [--costs cvar mmd_opt] [--ticks 40] [--reps 7]
                                      [--out profiles/mpc_vehicle_bench.json]

For every cost at B = 100, H = 30, O = 10 on the dynamic scenes of
``optimizer.closed_loop`` (episode e = configuration e of the sweep's generator,
the driver-seeded targets) and every number of episodes E, the wall time of the
loop proper -- ``Mpc.run(0, ticks)`` and the synchronisation behind it, after the
context's create, ``plan_vehicles`` and reset -- divided by the ticks: per tick the
chained begin, the CEM iterations and one k_mpc_step, which with the policy on
 is the planned instantiation.  Three sides alternate on
the same handle, one context each:

  constant  the policy off
  hold      the policy on, every vehicle's target its own speed and lane: the
            vehicles keep their course, the solves see the scene of ``constant``
            (to rounding), so the difference is the step's own cost
  planned   the policy on with the driver's targets: the vehicles cut in, so the
            solves work on other tracks and more episodes end early (the count of
            episodes still live at the end is reported); the difference is the
            scene's, not the step's

Median of ``--reps`` runs after one warm-up of each, with min and max, and the
differences of the medians.  Prints one JSON line and writes it to ``--out``.
Only figures of one session compare.
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


def measure(cem, native, CL, cost, n, E, ticks, reps):
    prob = cem.CEM(n, O, 0.1, H, "gaussian", 0.0, 0.0, num_batch=B, variant="dynamic", maxiter_cem=T, max_configs=E)
    vehicles, keys = CL.scenario("dynamic", E, O)
    starts = CL.starts_of("dynamic", E)
    f32 = np.float32
    cov = np.diag([20.0] * 4 + [100.0] * 4).astype(f32)
    mean = np.tile(np.array([15.0] * 4 + [0.0] * 4, f32), (E, 1))
    vel = np.concatenate([starts[:, 2:4], np.zeros((E, 1))], 1).astype(f32)
    u = np.random.default_rng(0).standard_normal((ticks, E, 3)).astype(f32)
    model = native.MpcModel(prob._cfg, cov, native.pop0_normals(prob._cfg), goal_x=1e6)   # nobody reaches it
    sides = {}
    targets = dict(hold=vehicles[:, :, [2, 1]], planned=CL.vehicle_targets(E, O))
    for name in ("constant", "hold", "planned"):
        ctx = native.Mpc(prob.handle, model, ticks)
        if name in targets:
            ctx.plan_vehicles(targets[name])
        sides[name] = (ctx, [])
    for rep in range(reps + 1):
        for ctx, times in sides.values():
            ctx.reset(starts[:, :2], vel, vehicles, mean, cov, u, keys)
            prob.handle.sync()
            t0 = time.perf_counter()
            ctx.run(cost, 0, ticks, cov, 15.0)
            prob.handle.sync()
            times.append((time.perf_counter() - t0) * 1e3 / ticks)
    live = {name: int((ctx.log(ticks)["done_tick"] < 0).sum()) for name, (ctx, _) in sides.items()}
    for ctx, _ in sides.values():
        ctx.close()
    prob.handle.close()
    off, hold, on = (_stats(sides[name][1][1:]) for name in ("constant", "hold", "planned"))
    return dict(cost=cost, n=n, E=E, ticks=ticks, reps=reps, constant_ms_per_tick=off, hold_ms_per_tick=hold,
                planned_ms_per_tick=on, hold_minus_constant_ms=round(hold["median"] - off["median"], 4),
                planned_minus_constant_ms=round(on["median"] - off["median"], 4), live_episodes_at_end=live)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--E", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--n", type=int, default=10)
    ap.add_argument("--costs", nargs="+", default=["cvar", "mmd_opt"])
    ap.add_argument("--ticks", type=int, default=40)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mpc_vehicle_bench.json"))
    a = ap.parse_args()
    from optimizer import _native, cem, closed_loop as CL
    rows = [measure(cem, _native, CL, cost, a.n, E, a.ticks, a.reps) for cost in a.costs for E in a.E]
    out = dict(tool="mpc_vehicle_bench", variant="dynamic", B=B, H=H, O=O, maxiter_cem=T, rows=rows)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
