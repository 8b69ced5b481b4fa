"""Time mpcmmd_validate_carla_risk beside mpcmmd_validate_carla (GPU box).

    python tools/time_validate_carla_risk.py [out.json] [--ticks 200] [--rollouts 1000] [--obs 3]

Both calls on the same inputs in one session: K ticks of the synthetic replay
(P = 600), det plans (n = 4, B = 24, T = 3), H = 60, R rollouts, given draws,
S = 2 bandwidths (0.01, 0.3).  HIP events (elapsed_ms of either call: the
counter reset and the kernels; for the risk call per stage: rollouts with costs
and counts, statistics, MMD), one warm-up call and three timed calls each, the
two calls alternating.  Also checks that the counts of the two calls are equal.
Prints one JSON line.
"""
import argparse
import importlib
import importlib.util
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mpc-mmd_amd")]
CARLA = os.path.join(ROOT, "mpc-mmd_amd", "carla")
MEAN = np.array([10.0] * 4 + [0.0] * 4, np.float32)
COV = np.diag([20.0] * 4 + [100.0] * 4).astype(np.float32)
H, P = 60, 600
SIGMA = (0.01, 0.3)


def _load(name, path, **kw):
    spec = importlib.util.spec_from_file_location(name, path, **kw)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--rollouts", type=int, default=1000)
    ap.add_argument("--obs", type=int, default=3)
    a = ap.parse_args()
    from optimizer import _native as N
    d = os.path.join(CARLA, "optimizer")
    _load("mpcmmd_carla_optimizer", os.path.join(d, "__init__.py"), submodule_search_locations=[d])
    Helper = importlib.import_module("mpcmmd_carla_optimizer.cem_helper").Helper
    rep = _load("mpcmmd_carla_replay", os.path.join(CARLA, "replay.py"))
    K, R, O = a.ticks, a.rollouts, a.obs
    rec = rep.record_synthetic(ticks=K)
    helper = Helper(num_prime=H)
    h = N.Handle(N.make_config(4, O, 0.1, H, "gaussian", 0.0, 0.0, num_batch=24, maxiter_cem=3,
                               variant="carla_town05"))
    plans = []
    for k in range(K):
        init, xo, yo, path = rep.tick_inputs(rec, k, helper, O)
        r = h.carla_solve("det", k, init, MEAN, COV, xo, yo, 10.0, path)
        plans.append(dict(init=init, xo=xo, yo=yo, path=path, v=r["v_best"].copy(), st=r["steering"].copy()))
    h.close()
    g = lambda n: [p[n] for p in plans]
    rng = np.random.default_rng(0)
    draws = rng.standard_normal((K, 3, R, H)).astype(np.float32)
    eps = rng.standard_normal((K, R, 4)).astype(np.float32)
    common = (g("init"), g("v"), g("st"), g("xo"), g("yo"), g("path"), np.arange(K), H, "gaussian", 0.1, 0.0, 0.0)
    res = dict(shape=dict(K=K, R=R, H=H, O=O, P=P, S=len(SIGMA)), validate_carla_ms=[], risk_ms=[])
    for it in range(4):   # the first round is the warm-up
        plain = N.validate_carla(*common, num_rollouts=R, draws=draws, init_eps=eps, timing=True)
        risk = N.validate_carla_risk(*common, num_rollouts=R, draws=draws, init_eps=eps, sigma=SIGMA, counts=True,
                                     timing=True)
        if it == 0:
            res["counts_equal"] = bool(all(np.array_equal(plain[k], risk[k])
                                           for k in ("count", "count_lane", "count_rows")))
            res["count_pos_obs_is_count_rows"] = bool(np.array_equal(risk["count_pos"][:, 0], risk["count_rows"]))
            res["channels_nonempty"] = int((risk["count_pos"] > 0).sum())
            res["mean_count_pos"] = [float(x) for x in risk["count_pos"].mean(axis=0)]
            continue
        res["validate_carla_ms"].append(round(float(plain["elapsed_ms"]), 4))
        res["risk_ms"].append([round(float(x), 4) for x in risk["elapsed_ms"]])
        print(it, plain["elapsed_ms"], risk["elapsed_ms"], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
