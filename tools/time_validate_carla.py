"""Time mpcmmd_validate_carla (GPU box) and its two yardsticks.

    python tools/time_validate_carla.py [--ticks 200] [--rollouts 1000] [--obs 10] [--reps 7]

The call: K ticks of the synthetic replay (P = 600), det plans (n = 4, B = 24,
T = 3: milliseconds each), H = 60, R rollouts; HIP events around the device
work (counter reset + the two kernels; mpcmmd_validate_carla_args.elapsed_ms),
2 warm-up calls, the median of --reps, with external draws and with the
internal Philox streams (gaussian and beta).

Yardsticks, measured in the same run:
  (a) the oracle composition (tests/carla_validation_ref.py) of the same shape
      on this machine's CPU threads, a few ticks, scaled to K;
  (b) the optimizer's own three-kernel chain -- roll_carla + frenet + risk_carla
      of mpcmmd_kernel_times of a cvar CARLA solve -- per (row x step) point.
Prints one JSON line.
"""
import argparse
import importlib.util
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mpc-mmd_amd"), os.path.join(ROOT, "tests")]
CARLA = os.path.join(ROOT, "mpc-mmd_amd", "carla")
MEAN = np.array([10.0] * 4 + [0.0] * 4, np.float32)
COV = np.diag([20.0] * 4 + [100.0] * 4).astype(np.float32)
H, P = 60, 600


def _carla_package():
    name = "mpcmmd_carla_optimizer"
    if name not in sys.modules:
        d = os.path.join(CARLA, "optimizer")
        spec = importlib.util.spec_from_file_location(name, os.path.join(d, "__init__.py"),
                                                      submodule_search_locations=[d])
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
    return name


def _replay():
    spec = importlib.util.spec_from_file_location("mpcmmd_carla_replay", os.path.join(CARLA, "replay.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--rollouts", type=int, default=1000)
    ap.add_argument("--obs", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only-call", action="store_true", help="skip the yardsticks")
    ap.add_argument("--oracle-ticks", type=int, default=3)
    ap.add_argument("--chain-n", type=int, default=1000, help="rows per candidate of the cvar solve of yardstick (b)")
    a = ap.parse_args()
    from optimizer import _native as N
    import importlib
    Helper = importlib.import_module(_carla_package() + ".cem_helper").Helper
    rep = _replay()
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

    def timed(noise, dr, ie):
        ms = []
        for i in range(2 + a.reps):
            out = N.validate_carla(g("init"), g("v"), g("st"), g("xo"), g("yo"), g("path"), np.arange(K), H, noise,
                                   0.1, 0.0, 0.0, num_rollouts=R, draws=dr, init_eps=ie, timing=True)
            if i >= 2:
                ms.append(out["elapsed_ms"])
        return float(np.median(ms)), [round(x, 3) for x in ms], out

    points = K * R * H
    res = dict(shape=dict(K=K, R=R, H=H, O=O, P=P), points=points)
    for label, noise, dr, ie in (("external_gaussian", "gaussian", draws, eps),
                                 ("internal_gaussian", "gaussian", None, None), ("internal_beta", "beta", None, None)):
        med, ms, out = timed(noise, dr, ie)
        res[label] = dict(ms=round(med, 3), all_ms=ms, points_per_s=round(points / (med * 1e-3), 1),
                          ns_per_point=round(med * 1e6 / points, 3),
                          ticks_with_hits=int((out["count_rows"] > 0).sum()))
    if a.only_call:
        print(json.dumps(res))
        return
    # (a) the oracle composition on the CPU
    import carla_validation_ref as ref
    from oracle import carla as KO
    ora = KO.CarlaCEM(4, 1, O, 0.1, H, "gaussian", "Town05", 0.0, 0.0, num_batch=24, maxiter_cem=3)
    t0 = time.perf_counter()
    for k in range(a.oracle_ticks):
        p = plans[k * (K // a.oracle_ticks)]
        ref.reference(ora, p["init"], p["v"], p["st"], p["xo"], p["yo"], p["path"], draws[k], eps[k])
    s_tick = (time.perf_counter() - t0) / a.oracle_ticks
    res["oracle_cpu"] = dict(s_per_tick=round(s_tick, 4), s_for_K=round(s_tick * K, 2),
                             ns_per_point=round(s_tick * 1e9 / (R * H), 1))
    # (b) the optimizer's chain: roll_carla + frenet + risk_carla of a cvar solve, per (row x step) point
    for n in (a.chain_n, 100):
        try:
            B, T = 100, 20
            hc = N.Handle(N.make_config(n, O, 0.1, H, "gaussian", 0.0, 0.0, num_batch=B, maxiter_cem=T,
                                        variant="carla_town05"))
            p = plans[K // 2]
            hc.carla_solve("cvar", 1, p["init"], MEAN, COV, p["xo"], p["yo"], 10.0, p["path"])   # warm-up
            hc.profile(True)
            hc.carla_solve("cvar", 1, p["init"], MEAN, COV, p["xo"], p["yo"], 10.0, p["path"])
            hc.sync()
            kt = hc.kernel_times()
            hc.profile(False)
            hc.close()
            chain = {k: kt[k] for k in ("roll_carla", "frenet", "risk_carla")}
            launches = chain["frenet"][0]
            pts = launches * B * n * H
            tot = sum(v[1] for v in chain.values())
            res["chain"] = dict(n=n, B=B, launches=int(launches), points=int(pts),
                                ms={k: round(v[1], 3) for k, v in chain.items()},
                                ns_per_point=round(tot * 1e6 / pts, 3), points_per_s=round(pts / (tot * 1e-3), 1))
            break
        except Exception as e:  # a shape the handle does not take: the smaller one
            res.setdefault("chain_errors", []).append(f"n={n}: {e}")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
