"""CARLA ticks from raw inputs to results: the host route against the tick route (GPU box).

    python tools/carla_tick_bench.py [--G 1 2 8] [--n 10] [--costs cvar mmd_opt] [--routes host tick]
                                     [--solves 10] [--out profiles/carla_tick_bench.json]

For every cost at B = 100, H = 60, O = 3, num_path = 600 on ticks of the
synthetic Town05 replay, and every G, the wall time of G ticks from the
recording to the results (median of ``--solves`` >= 10 after 2 warm-ups, with
min and max), and that time per tick:

  host  ``replay.tick_inputs`` of every tick (the host helpers: path smoothing,
        path parameters, Frenet obstacles, tracks), then ``carla_solve_batch``;
        the helpers' share is its own column (``prep_ms``)
  tick  ``replay.tick_raw_inputs`` of every tick, then ``Tick.solve_batch``
        (mpcmmd_carla_tick_solve_batch: the same preprocessing in k_tick.hip)

and for the tick route the ``mpcmmd_profile`` times of the two new kernels in
one more batch.  ``--routes host`` with MPCMMD_LIB pointing at a library built
from the parent commit gives the parent's host route in the same session: that
pair of host figures is the noise floor.  Prints one JSON line and writes it
to ``--out``.  Only figures of one session compare.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mpc-mmd_amd")]

import bench  # noqa: E402
from optimizer import _native as N  # noqa: E402

B, H, O, T, P = 100, 60, 3, 20, 600
MEAN = np.array([10.0] * 4 + [0.0] * 4, np.float32)
COV = np.diag([20.0] * 4 + [100.0] * 4).astype(np.float32)


def _stats(ms):
    return dict(median=round(statistics.median(ms), 3), min=round(min(ms), 3), max=round(max(ms), 3))


def measure(route, cost, n, G, rec, rep, helper, solves):
    cfg = N.make_config(n, O, 0.1, H, "gaussian", 0.0, 0.0, num_batch=B, maxiter_cem=T, variant="carla_town05")
    h = N.Handle(cfg, max_configs=G)
    idx = list(range(5, 5 + G))
    ticks = [40 + 10 * g for g in range(G)]
    prep = []
    if route == "host":
        def run():
            t0 = time.perf_counter()
            ins = [rep.tick_inputs(rec, k, helper, O) for k in ticks]
            prep.append((time.perf_counter() - t0) * 1e3)
            return h.carla_solve_batch(cost, idx, np.stack([i[0] for i in ins]), MEAN, COV,
                                       np.stack([i[1] for i in ins]), np.stack([i[2] for i in ins]), 10.0,
                                       [i[3] for i in ins])
    else:
        tick = N.Tick(h, P)

        def run():
            t0 = time.perf_counter()
            raw = [rep.tick_raw_inputs(rec, k, O) for k in ticks]
            prep.append((time.perf_counter() - t0) * 1e3)
            return tick.solve_batch(cost, idx, np.stack([r[0] for r in raw]), np.stack([r[1] for r in raw]),
                                    np.stack([r[2] for r in raw]), np.stack([r[3] for r in raw]), 0.1, MEAN, COV, 10.0)
    for _ in range(2):
        run()
    del prep[:]
    ms = []
    for _ in range(solves):
        t0 = time.perf_counter()
        run()
        ms.append((time.perf_counter() - t0) * 1e3)
    total, pre = _stats(ms), _stats(prep)
    row = dict(route=route, cost=cost, n=n, G=G, total_ms=total, prep_ms=pre,
               ms_per_tick=round(total["median"] / G, 3), prep_ms_per_tick=round(pre["median"] / G, 3), solves=solves)
    if route == "tick":
        h.profile(1)
        run()
        kt = h.kernel_times()
        h.profile(0)
        row["tick_kernel_ms"] = {k: round(kt[k][1], 4) for k in ("tick_path", "tick_setup")}
    h.close()
    return row


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--G", type=int, nargs="+", default=[1, 2, 8])
    ap.add_argument("--n", type=int, default=10)
    ap.add_argument("--costs", nargs="+", default=["cvar", "mmd_opt"], choices=["mmd_opt", "cvar", "det"])
    ap.add_argument("--routes", nargs="+", default=["host", "tick"], choices=["host", "tick"])
    ap.add_argument("--solves", type=int, default=10)
    ap.add_argument("--label", default="", help="stored in the output (e.g. which library was measured)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "carla_tick_bench.json"))
    a = ap.parse_args(argv)
    if a.solves < 10:
        ap.error("--solves must be >= 10")
    cem, rep = bench._carla_modules()
    helper = cem.Helper(num_prime=H)   # the drop-in's path helpers (cem_helper.py)
    rec = rep.record_synthetic(ticks=40 + 10 * max(a.G) + 1, num_path=P)
    rows = []
    for cost in a.costs:
        for G in a.G:
            for route in a.routes:
                r = measure(route, cost, a.n, G, rec, rep, helper, a.solves)
                rows.append(r)
                print(f"# {route} {cost} n={a.n} G={G}: {r['total_ms']['median']:.2f} ms "
                      f"[{r['total_ms']['min']:.2f}, {r['total_ms']['max']:.2f}], {r['ms_per_tick']:.2f} ms per tick, "
                      f"inputs {r['prep_ms']['median']:.2f} ms {r.get('tick_kernel_ms', '')}", file=sys.stderr, flush=True)
    out = dict(tool="carla_tick_bench", label=a.label, B=B, H=H, O=O, num_path=P, maxiter_cem=T, rows=rows)
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
