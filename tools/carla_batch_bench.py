"""Batched CARLA solves: wall time per tick against the batch size G (GPU box).

    python tools/carla_batch_bench.py [--G 1 2 4 5 8] [--n 10 22] [--costs mmd_opt cvar]
                                      [--solves 10] [--out profiles/carla_batch_bench.json]

For every cost and num_reduced_sqrt n at B = 100, H = 60, O = 3 on ticks of the
synthetic Town05 replay, and every G: the wall time of one
``carla_solve_batch`` of G different ticks (median of ``--solves`` >= 10 solves
after 2 warm-ups), that time per tick, and the ``mpcmmd_profile`` per-kernel
totals of one more batch (profiling runs every launch on one stream, so these
are per-kernel times, not the overlapped wall time).  G = 1 runs through
``carla_solve`` on a max_configs = 1 handle -- the path that existed before the
batch, so ``--G 1`` on an older checkout gives its figure in the same session.
Prints one JSON line and writes it to ``--out``.  Only figures of one session
compare.
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

B, H, O, T = 100, 60, 3, 20
MEAN = np.array([10.0] * 4 + [0.0] * 4, np.float32)
COV = np.diag([20.0] * 4 + [100.0] * 4).astype(np.float32)


def launch_path(h, cost, G, kt):
    """Which beta-CEM launch path the batch took (sequence.hip: run_beta_cem)."""
    if cost != "mmd_opt":
        return "no beta-CEM"
    if kt.get("bcem_small", (0, 0.0))[0] > 0:
        return "fused (k_bcem_small)"
    Bt = G * B
    if 64 <= Bt <= 256 and h.info("groups") > 1:
        return f"small groups ({min(h.info('groups'), 2)} streams)"
    if Bt >= 1024 and h.info("groups") > 1:
        return f"{h.info('groups')} groups"
    return "one stream"


def measure(cost, n, G, ins, solves):
    cfg = N.make_config(n, O, 0.1, H, "gaussian", 0.0, 0.0, num_batch=B, maxiter_cem=T, variant="carla_town05")
    h = N.Handle(cfg, max_configs=G)
    idx = list(range(5, 5 + G))
    if G == 1:
        init, xo, yo, path = ins[0]
        run = lambda: h.carla_solve(cost, idx[0], init, MEAN, COV, xo, yo, 10.0, path)
    else:
        inits = np.stack([i[0] for i in ins[:G]])
        xo = np.stack([i[1] for i in ins[:G]])
        yo = np.stack([i[2] for i in ins[:G]])
        paths = [i[3] for i in ins[:G]]
        run = lambda: h.carla_solve_batch(cost, idx, inits, MEAN, COV, xo, yo, 10.0, paths)
    for _ in range(2):
        run()
    ms = []
    for _ in range(solves):
        t0 = time.perf_counter()
        run()
        ms.append((time.perf_counter() - t0) * 1e3)
    h.profile(1)
    run()
    kt = {k: v for k, v in h.kernel_times().items() if v[0] > 0}
    h.profile(0)
    row = dict(cost=cost, n=n, G=G, candidates=G * B, solve_ms=round(statistics.median(ms), 3),
               ms_per_tick=round(statistics.median(ms) / G, 3), solve_ms_min=round(min(ms), 3),
               solve_ms_max=round(max(ms), 3), solves=solves, gen_wave=int(h.info("gen_wave")),
               path=launch_path(h, cost, G, kt),
               kernel_ms={k: round(v[1], 3) for k, v in sorted(kt.items(), key=lambda kv: -kv[1][1])},
               kernel_launches={k: v[0] for k, v in kt.items()})
    h.close()
    return row


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--G", type=int, nargs="+", default=[1, 2, 4, 5, 8])
    ap.add_argument("--n", type=int, nargs="+", default=[10, 22])
    ap.add_argument("--costs", nargs="+", default=["mmd_opt", "cvar"], choices=["mmd_opt", "cvar", "det"])
    ap.add_argument("--solves", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "carla_batch_bench.json"))
    a = ap.parse_args(argv)
    if a.solves < 10:
        ap.error("--solves must be >= 10")
    cem, rep = bench._carla_modules()
    helper = cem.Helper(num_prime=H)   # the drop-in's path helpers (cem_helper.py)
    Gmax = max(a.G)
    rec = rep.record_synthetic(ticks=40 + 10 * Gmax + 1)
    ins = [rep.tick_inputs(rec, 40 + 10 * g, helper, O) for g in range(Gmax)]
    rows = []
    for cost in a.costs:
        for n in a.n:
            for G in a.G:
                rows.append(measure(cost, n, G, ins, a.solves))
                r = rows[-1]
                print(f"# {cost} n={n} G={G}: {r['solve_ms']:.2f} ms per solve, {r['ms_per_tick']:.2f} ms per tick "
                      f"[{r['path']}, gen_wave={r['gen_wave']}]", file=sys.stderr, flush=True)
    out = dict(tool="carla_batch_bench", B=B, H=H, O=O, maxiter_cem=T, rows=rows)
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
