"""Time mpcmmd_validate_risk (GPU box).

    python tools/time_validate_risk.py [out.json]

Stage times (mpcmmd_validate_risk_args.elapsed_ms: HIP events around the
rollout, statistics and MMD stages) at K = 200, O = 10, H = 30, R = 100000,
S = 2 with the internal Philox streams, one warm-up call and three timed ones;
beside them the host wall time of mpcmmd_validate at the same shape (it has no
device timer: the time includes its uploads and read-back), and the number of
exp2 terms the pair kernel executes (whole 1024 x 1024 tiles, the diagonal and
the j-tiles after it) from the non-zero counts of the returned costs.  Then the
pair kernel alone on injected samples without a zero (K = 8, R = 100000): every
tile runs, terms / s of the MMD stage.  Prints one JSON line.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mpc-mmd_amd")]
from optimizer import _native  # noqa: E402

K, O, H, R, S = 200, 10, 30, 100000, 2
rs = np.random.RandomState(0)
j = np.arange(11) / 10.0
cx, cy, st, xo, yo = [], [], [], [], []
for k in range(K):
    a = 15.0 * (5.0 * j + 3.0 * j * j) + rs.normal(0, 0.2, 11)
    b = 1.75 + rs.normal(0, 0.4, 11)
    b[:3] = 1.75
    cx.append(a), cy.append(b), st.append([0.0, 1.75, 5.0, 0.0, 0.0, 0.0])
    xs = rs.choice(np.arange(15, 80, 5.0), O, replace=False)
    ys = rs.choice([-1.75, 1.75, 3.5], O)
    xo.append(np.repeat(xs[:, None], 100, 1).astype(np.float32))
    yo.append(np.repeat(ys[:, None], 100, 1).astype(np.float32))
cx, cy, st, xo, yo = (np.array(a) for a in (cx, cy, st, xo, yo))
keys = np.arange(K)
sig = np.array([0.01, 0.3], np.float32)
res = dict(shape=dict(K=K, O=O, H=H, R=R, S=S), risk=[], validate_wall_ms=[], risk_wall_ms=[])


def tiles(P):
    nt = -(-P // 1024)
    return nt * (nt + 1) // 2


for it in range(4):   # the first is the warm-up
    t0 = time.perf_counter()
    got = _native.validate_risk(cx, cy, st, xo, yo, keys, H, "gaussian", 0.1, 0.05, 0.01, num_rollouts=R, seed=3,
                                sigma=sig, timing=True, return_costs=(it == 0))
    t1 = time.perf_counter()
    if it == 0:
        cnt, lane = _native.validate(cx, cy, st, xo, yo, keys, H, "gaussian", 0.1, 0.05, 0.01, num_rollouts=R,
                                     seed=3)
        P = (got["costs"] != 0).sum(axis=2)
        res["nonzero_P"] = dict(mean=float(P.mean()), max=int(P.max()), channels_nonempty=int((P > 0).sum()))
        res["pair_exps_executed"] = int(S * 1024 * 1024 * sum(tiles(int(p)) for p in P.reshape(-1)))
        res["count_check"] = bool(np.all(cnt <= got["count_pos"][:, 0]))
        continue
    res["risk"].append([float(x) for x in got["elapsed_ms"]])
    res["risk_wall_ms"].append((t1 - t0) * 1e3)
    print(it, got["elapsed_ms"], (t1 - t0) * 1e3, flush=True)
for it in range(3):   # the yardstick in a loop of its own (the first call above warmed it up)
    t1 = time.perf_counter()
    _native.validate(cx, cy, st, xo, yo, keys, H, "gaussian", 0.1, 0.05, 0.01, num_rollouts=R, seed=3)
    res["validate_wall_ms"].append((time.perf_counter() - t1) * 1e3)
print("validate", res["validate_wall_ms"], flush=True)

# dense: every value non-zero, so the pair kernel runs every tile
Kd = 8
cin = rs.uniform(0.001, 3.0, (Kd, 3, R)).astype(np.float32)
res["dense"] = []
for it in range(4):
    got = _native.validate_risk(costs_in=cin, sigma=sig, timing=True)
    if it:
        exps = S * 1024 * 1024 * tiles(R) * 3 * Kd
        ms = float(got["elapsed_ms"][2])
        res["dense"].append(dict(mmd_stage_ms=ms, exps=exps, exps_per_s=exps / (ms * 1e-3),
                                 unique_pair_terms_per_s=S * (R * (R + 1) // 2) * 3 * Kd / (ms * 1e-3)))
        print("dense", res["dense"][-1], flush=True)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(res, f, indent=1)
print(json.dumps(res))
