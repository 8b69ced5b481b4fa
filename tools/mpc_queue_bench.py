"""The scene queue of the synthetic closed loop: its own cost, and what it buys (GPU box).

    python tools/mpc_queue_bench.py [--E 1 8] [--n 10] [--costs cvar mmd_opt] [--ticks 40] [--reps 5]
                                    [--scenes 64] [--slots 8] [--out profiles/mpc_queue_bench.json]

B = 100, H = 30, O = 10, the scenes of ``optimizer.closed_loop``.  Two measurements, the sides
alternating in one process, median of ``--reps`` runs after one warm-up of each side, with min and max:

  own cost   static variant, constant-velocity vehicles, drawn variates.  *run*: ``Mpc.reset`` then
             ``Mpc.run(0, ticks)`` over E episodes.  *queue*: ``Mpc.queue_reset`` with N = E scenes
             of ``ticks`` ticks per episode, then ``Mpc.queue_run(0, ticks)``: no slot is ever
             refilled, every slot is solved on every tick on both sides, so the difference is the
             queue's two extra launches per tick (k_mpc_queue and the masked reset-mode step).
             The loop proper -- the call and the synchronisation behind it -- in ms per lockstep tick.
  campaign   section 23's cut-in scene (dynamic variant, planned vehicles, the driver's targets):
             ``--scenes`` scenes of ``--ticks`` ticks through ``--slots`` slots by
             ``CEM.run_campaign``, against the same scenes as batches of ``--slots`` by
             ``CEM.run_episodes``; end to end, in scenes per second, with the lockstep ticks each
             side solves (deterministic) and how the scenes ended.

Prints one JSON line and writes it to ``--out``.  Only figures of one session compare.
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


def _stats(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))


def own_cost(cem, native, CL, cost, n, E, ticks, reps):
    prob = cem.CEM(n, O, 0.1, H, "gaussian", 0.0, 0.0, num_batch=B, variant="static", maxiter_cem=T, max_configs=E)
    vehicles, keys = CL.scenario("static", E, O)
    starts = CL.starts_of("static", E)
    f32 = np.float32
    cov = np.diag([20.0] * 4 + [100.0] * 4).astype(f32)
    mean = np.tile(np.array([15.0] * 4 + [0.0] * 4, f32), (E, 1))
    vel = np.concatenate([starts[:, 2:4], np.zeros((E, 1))], 1).astype(f32)
    model = native.MpcModel(prob._cfg, cov, native.pop0_normals(prob._cfg), goal_x=1e6)   # nobody reaches it
    run_ctx, queue_ctx = native.Mpc(prob.handle, model, ticks), native.Mpc(prob.handle, model, ticks)
    run, queue = [], []
    for rep in range(reps + 1):
        run_ctx.reset(starts[:, :2], vel, vehicles, mean, cov, None, keys)
        prob.handle.sync()
        t0 = time.perf_counter()
        run_ctx.run(cost, 0, ticks, cov, 15.0)
        prob.handle.sync()
        run.append((time.perf_counter() - t0) * 1e3 / ticks)
        queue_ctx.queue_reset(E, ticks, starts[:, :2], vel, vehicles, mean, cov, 15.0, keys)
        prob.handle.sync()
        t0 = time.perf_counter()
        queue_ctx.queue_run(cost, 0, ticks, cov)
        prob.handle.sync()
        queue.append((time.perf_counter() - t0) * 1e3 / ticks)
    a, b = run_ctx.log(ticks), queue_ctx.log(ticks)
    same = all(np.array_equal(a[k], b[k]) for k in ("log_d", "log_f", "log_i", "cx", "cy", "mean"))
    run_ctx.close(), queue_ctx.close()
    prob.handle.close()
    r, q = _stats(run[1:]), _stats(queue[1:])
    return dict(cost=cost, n=n, E=E, ticks=ticks, reps=reps, run_ms_per_tick=r, queue_ms_per_tick=q,
                queue_minus_run_ms=round(q["median"] - r["median"], 4), same_log=bool(same))


def campaign(cem, CL, cost, n, scenes, slots, ticks, reps):
    prob = cem.CEM(n, O, 0.1, H, "gaussian", 0.0, 0.0, num_batch=B, variant="dynamic", maxiter_cem=T,
                   max_configs=slots)
    vehicles, keys = CL.scenario("dynamic", scenes, O)
    starts = CL.starts_of("dynamic", scenes)
    target = CL.vehicle_targets(scenes, O)
    camp, batch = [], []
    res = None
    for rep in range(reps + 1):
        prob.handle.sync()
        t0 = time.perf_counter()
        res = prob.run_campaign(cost, vehicles, starts, ticks, slots=slots, keys=keys, planned=dict(target=target))
        camp.append(scenes / (time.perf_counter() - t0))
        prob.handle.sync()
        t0 = time.perf_counter()
        done = []
        for b in range(0, scenes, slots):
            sl = slice(b, min(b + slots, scenes))
            out = prob.run_episodes(cost, vehicles[sl], starts[sl], ticks, chained=True, keys=keys[sl],
                                    planned=dict(target=target[sl]))
            done.append(out["done_tick"])
        batch.append(scenes / (time.perf_counter() - t0))
    prob.handle.close()
    done = np.concatenate(done)
    reasons = np.bincount(res["end_reason"], minlength=4)
    c, b = _stats(camp[1:]), _stats(batch[1:])
    return dict(cost=cost, n=n, scenes=scenes, slots=slots, ticks_per_episode=ticks, reps=reps,
                campaign_scenes_per_s=c, batches_scenes_per_s=b, ratio=round(c["median"] / b["median"], 3),
                campaign_lockstep_ticks=int(res["lockstep_ticks"]), batches_lockstep_ticks=-(-scenes // slots) * ticks,
                live_scene_ticks=int((res["end_tick"] + 1).sum()),
                ended=dict(zip(("unfinished", "collision", "goal", "tick_limit"), map(int, reasons))),
                same_ends=bool(np.array_equal(done, res["done_tick"])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--E", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--n", type=int, default=10)
    ap.add_argument("--costs", nargs="+", default=["cvar", "mmd_opt"])
    ap.add_argument("--ticks", type=int, default=40)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scenes", type=int, default=64)
    ap.add_argument("--slots", type=int, default=8)
    ap.add_argument("--campaign-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mpc_queue_bench.json"))
    a = ap.parse_args()
    from optimizer import _native, cem, closed_loop as CL
    rows, camps = [], []
    for cost in a.costs:
        for E in a.E:
            rows.append(own_cost(cem, _native, CL, cost, a.n, E, a.ticks, a.reps))
            print(json.dumps(rows[-1]), file=sys.stderr, flush=True)   # progress
    for cost in a.costs:
        camps.append(campaign(cem, CL, cost, a.n, a.scenes, a.slots, a.ticks, a.campaign_reps))
        print(json.dumps(camps[-1]), file=sys.stderr, flush=True)
    out = dict(tool="mpc_queue_bench", B=B, H=H, O=O, maxiter_cem=T, own_cost=rows, campaign=camps)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
