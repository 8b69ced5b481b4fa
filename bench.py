#!/usr/bin/env python3
"""Throughput bench of the CEM-projection optimizer hot path (BASELINE.json).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--workload mmd_opt|cvar|dynamic|configs0]
                    [--dump-outputs DIR] [--full]

One step = one outer CEM iteration (cem.py:221-315 body: initial guess,
projection, controls, noisy rollouts, risk reducer (beta-CEM for mmd_opt),
elite sorts, CEM update) over the whole batch, on device-resident inputs, with
the library's internal Philox noise.  Every 20 steps a new solve starts
(mpcmmd_begin: boundary vectors, initial population, obstacle upload), as in
the reference's 20-iteration compute_cem_* call; that host work is inside the
timed region.  ``value`` = K / elapsed of the K timed steps; the per-step
HIP-event durations give ``median_ms_per_step``.

N > 1: one process per GPU (torchrun).  Each rank solves its own obstacle
configuration (config k = rank, seeded like S/main_mpc.py:12,114), so per-GPU
work is fixed ("scaling": "weak"); RCCL is used for the barrier, the max of
the elapsed times and the final gather of the per-config results (§8e).

A plain run sets up, warms up, times the K steps and prints the result line.
--dump-outputs DIR then writes what the solve of the last timed step returns
(mpcmmd_finish after that step: cx, cy, cost_lane, cost_obs, sigma, res_beta,
beta) as DIR/<name>.npy in float32; the inputs and the Philox seed are fixed
by the arguments, so two builds can be compared output for output.

--full adds: "roofline" for the dominant kernel (HIP-event durations of the
library's launches on its stream, during a profiled pass of the same steps),
"cpu_baseline" (the NumPy oracle on a bounded sample of the same workload,
rank 0, N = 1 only) and, at N = 1, "extra_workloads": the other BASELINE
configurations this path runs on one GPU (configs[2] cvar/beta 0.3,
configs[3] dynamic obstacles per GPU, configs[0] n = 50 / M = 2500), each
with its own steps/s, median step and roofline.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(ROOT, "mpc-mmd_amd")
for _p in (ROOT, PKG):
    if _p not in sys.path:
        sys.path.insert(0, _p)

kF = 22  # beta-CEM features per mother row (cx | cy)
METRIC = "MPC optimizer steps/s (batch=1024,H=30,obs_samp=500) @1/2/4/8 GPU; % HBM roofline"

# BASELINE.json configs[1] (headline), configs[2], configs[3] (per GPU: one configuration per rank), configs[0]
WORKLOADS = {
    "mmd_opt": dict(desc="static obs, mmd_opt, batch=1024 rollouts, H=30, num_obs=10, obs_samples=484 (n=22, M=n^2)",
                    baseline="configs[1]", cost="mmd_opt", num_reduced=22, num_obs=10, num_prime=30,
                    noise="gaussian", level=0.1, num_batch=1024),
    "cvar": dict(desc="static obs, cvar, batch=1024 rollouts, H=30, num_obs=10, obs_samples=500, beta noise 0.3",
                 baseline="configs[2]", cost="cvar", num_reduced=500, num_obs=10, num_prime=30, noise="beta",
                 level=0.3, num_batch=1024),
    "dynamic": dict(desc="dynamic obs, mmd_opt, batch=1024 rollouts, H=50, num_obs=20, obs_samples=1024 (n=32, M=n^2)",
                    baseline="configs[3] (per GPU)", cost="mmd_opt", num_reduced=32, num_obs=20, num_prime=50,
                    noise="gaussian", level=0.1, num_batch=1024, variant="dynamic"),
    "configs0": dict(desc="static obs, mmd_opt, num_batch=100 (reference), H=20, num_obs=4, num_reduced=50 (M=2500)",
                     baseline="configs[0]", cost="mmd_opt", num_reduced=50, num_obs=4, num_prime=20,
                     noise="gaussian", level=0.1, num_batch=100),
}

# MI355X peaks (MI355X_MICROARCH.md): 1024 SIMDs at 2.4 GHz.  fp32 vector: one
# lane-op per lane per cycle (32 lanes/cycle/SIMD) = 78.6 T lane-ops/s;
# v_exp_f32 issues a wave64 instruction every 8 cycles (8 lanes/cycle/SIMD =
# 19.7 T exp/s); fp64 vector 39.3 T lane-FMA/s; fp64 MFMA 78.6 TFLOP/s.
SIMDS, CLOCK = 1024, 2.4e9
VALU_PEAK_TOPS = 78.6
VALU64_PEAK_TOPS = 39.3
MFMA64_PEAK_TFLOPS = 78.6
# exp-term floor of k_bkernel: per summed term one v_exp_f32 (8 cycles / 64
# lanes) + half a packed scale and half a packed add (2 cycles / 128 terms each)
EXP_TERM_CYCLES = 8 / 64 + 2 / 128 + 2 / 128
EXP_TERM_PEAK = SIMDS * CLOCK / EXP_TERM_CYCLES / 1e12   # 15.7 T terms/s
HBM_PEAK_GBS = 8000.0
# fp64 MFMA rate for the step roofline: v_mfma_f64_16x16x4 issue rate measured
# on one SIMD by tools/microbench.hip (profiles/r04_microbench.txt), x 1024
# SIMDs x 2.4 GHz; the guide has no fp64 MFMA figure
MFMA64_MEASURED_TFLOPS = 78.6


def kernel_work(w, name, launches, stats):
    """Algorithmic work of the profiled launches of kernel `name` (DESIGN.md
    §4): (bound, unit, amount, peak).
      bkernel  series row sums and K_red: its HBM bytes (K_red entries
               written, 4 B each (stats[3]); per series pair (stats[2]) the
               4-B selection read and the 4-B row sum written) against HBM
      bdirect  directly summed (sample, row) pairs (stats[1]) x M exp terms,
               against the exp-term issue floor (EXP_TERM_PEAK)
      bsample  per candidate and beta-iteration, per 16-position block and 89
               samples: T Z 16x16, U S 16x11, W^T Z 11x16 (2 flop each) +
               W U^T 16x16x11, on fp64 MFMA
      bqp      89 (n+1)-QPs per candidate: n^3/6 Cholesky + 2 n^2 solves in
               fp32 + n^2 cost FMAs in fp64 (each worth two fp32 issue
               slots), in fp32 lane-FMA equivalents against the fp32 rate
      bdist    M x M distances x 22 features x 2 (sub, abs-add) per candidate
      bmoment  the distance matrix read once (M x dist_stride(M) x 4 B per
               candidate) against HBM
      beta_planes  B x S x H x 2 Beta draws x 27 VALU issue slots (attempt 0
               of two gammas: 5 fp64 ops each; the combine: 6 fp64 ops and 11
               fp32 slots, the four transcendentals at their double issue
               cost) against one lane-slot per lane and cycle (39.3 T/s)
      risk_baseline  B x S rollouts x H steps x (bicycle 40 + 9 per obstacle);
               the Beta draws are k_beta_planes' work (its own model), the
               rollouts read them"""
    B, H, O = w["num_batch"], w["num_prime"], w["num_obs"]
    n = w["num_reduced"]
    M = n * n
    if name == "bkernel":
        return "hbm", "GB/s", stats[3] * 4 + stats[2] * 8, HBM_PEAK_GBS, 1e9
    if name == "bdirect":
        return "exp-issue", "T exp-terms/s", stats[1] * M, EXP_TERM_PEAK
    if name == "bsample":
        nblk = (((M + 1) + 31) // 32) * 2
        per = nblk * 89 * 2 * (16 * 16 + 16 * 11 + 11 * 16) + nblk * 16 * 16 * 11 * 2
        return "mfma-fp64", "TFLOP/s", launches * B * per, MFMA64_PEAK_TFLOPS
    if name == "bqp":
        per = 89 * (n ** 3 / 6 + 2 * n * n + 2 * n * n)
        return "valu-fp32", "T lane-FMA/s", launches * B * per, VALU_PEAK_TOPS
    if name == "bdist":
        return "valu", "T lane-ops/s", launches * B * M * M * kF * 2, VALU_PEAK_TOPS
    if name == "bmoment":
        return "hbm", "GB/s", launches * B * M * ((M + 255) // 256 * 256) * 4, HBM_PEAK_GBS, 1e9
    if name == "beta_planes":
        return "valu-issue", "T lane-slots/s", launches * B * n * H * 2 * 27, VALU64_PEAK_TOPS
    if name == "risk_baseline":
        return "valu", "T lane-ops/s", launches * B * n * H * (40 + O * 9), VALU_PEAK_TOPS
    return None


def alg_bytes_per_step(w):
    """SURVEY §8d algorithmic HBM bytes of one step (the planes a
    straightforward design writes once and reads once): cvar/saa/mmd_random
    16 B S H (x, y rollout planes) + noise rows + obstacles + controls +
    costbar + projection state (+ 16 B S H Beta planes); mmd_opt the mother
    x, y planes and 22 fit features written and read once + projection state."""
    B, S, H, O = w["num_batch"], w["num_reduced"], w["num_prime"], w["num_obs"]
    state = B * (8 + 22 + 22 + 198 + 600) * 4 * 2
    if w["cost"] == "mmd_opt":
        M = S * S
        return 2 * B * M * (2 * H + kF) * 4 + state + 2 * O * H * 4
    b = 16 * B * S * H + 3 * S * H * 4 + 2 * O * H * 4 + 2 * B * H * 4 * 2 + 2 * B * S * 4 + state
    if w["noise"] == "beta":
        b += 16 * B * S * H
    return b


def step_roofline(w, busy, profile_steps, stats, ms_per_step, workload):
    """Step-level roofline:
    t_lower = max(bytes_alg / HBM peak, VALU lane-slots / 78.6 T/s, fp64 MFMA
    flop / MFMA peak) per step, achieved = t_lower / measured step time,
    hbm_frac = PMC counter bytes per step / (t x 8 TB/s) and alg_hbm_frac =
    bytes_alg / (t x 8 TB/s) (the metric's "% HBM roofline").  VALU
    lane-slots (fp32 lane-op equivalents; fp64 FMA and v_exp_f32 at their
    issue cost):
      cvar/saa/mmd_random  SURVEY §8d: B S H 36 + B S O H 9 (+ B S H 160 beta)
      mmd_opt  this implementation's minimal work: k_bdist half matrix
               B M (M+1)/2 22 x 2; k_bmoment B M M 11 (packed powers/adds);
               QPs B x 89 x 20 x (n^3/6 + 4 n^2); series pairs x 28 (14 fp64
               FMA); K_red entries x 5 (exp + scale); directly summed pairs
               x M terms x 5
    MFMA: k_bsample's fp64 flops (kernel_work) x launches per step, against
    the fp64 MFMA rate measured by tools/microbench.hip
    (profiles/r04_microbench.txt)."""
    B, S, H, O = w["num_batch"], w["num_reduced"], w["num_prime"], w["num_obs"]
    per = 1.0 / profile_steps
    if w["cost"] == "mmd_opt":
        M = S * S
        slots = (B * M * (M + 1) / 2 * kF * 2 + B * M * M * 11 + B * 89 * 20 * (S ** 3 / 6 + 4 * S * S)
                 + (stats[2] * 28 + stats[3] * 5 + stats[1] * M * 5) * per)
        mflop = 0.0
        if "bsample" in busy:
            mflop = kernel_work(w, "bsample", busy["bsample"][0], stats)[2] * per
    else:
        slots = B * S * H * 36 + B * S * O * H * 9 + (B * S * H * 160 if w["noise"] == "beta" else 0)
        mflop = 0.0
    alg = alg_bytes_per_step(w)
    t_hbm = alg / (HBM_PEAK_GBS * 1e9)
    t_valu = slots / (VALU_PEAK_TOPS * 1e12)
    t_mfma = mflop / (MFMA64_MEASURED_TFLOPS * 1e12)
    t_lower = max(t_hbm, t_valu, t_mfma)
    t = ms_per_step / 1e3
    counter = 0.0
    have = True
    tags = set()
    for k, (launches, _) in busy.items():
        v, tag = pmc_traffic(workload, k, with_tag=True)
        if v is None:
            have = False
            continue
        tags.add(tag)
        counter += v * launches * per
    bound = {t_hbm: "hbm", t_valu: "valu", t_mfma: "mfma-fp64"}[t_lower]
    return {"t_lower_ms": t_lower * 1e3, "bound": bound, "achieved": t_lower / t, "t_hbm_ms": t_hbm * 1e3,
            "t_valu_ms": t_valu * 1e3, "t_mfma_ms": t_mfma * 1e3, "bytes_alg": alg,
            "alg_hbm_frac": alg / (t * HBM_PEAK_GBS * 1e9), "valu_lane_slots": slots, "mfma_flop": mflop,
            "counter_bytes": counter if have else None, "counter_profiles": sorted(tags),
            "hbm_frac": counter / (t * HBM_PEAK_GBS * 1e9) if have else None,
            "mfma_peak_tflops": MFMA64_MEASURED_TFLOPS}


def _pmc_files():
    """The committed PMC traffic files, newest first: profiles/rNN[x]_pmc_traffic.json
    ({workload: {kernel: bytes}}) and rNN[x]_pmc_traffic_<workload>.json
    ({kernel: bytes}; <workload> "mmdopt" = mmd_opt)."""
    import re
    pat = re.compile(r"^r(\d\d)([a-z]?)_pmc_traffic(?:_([a-z0-9]+))?\.json$")
    out = []
    try:
        names = os.listdir(os.path.join(ROOT, "profiles"))
    except OSError:
        return out
    for nm in names:
        m = pat.match(nm)
        if m:
            wl = {"mmdopt": "mmd_opt"}.get(m.group(3), m.group(3))
            out.append(((int(m.group(1)), m.group(2)), f"r{m.group(1)}{m.group(2)}", wl, nm))
    out.sort(key=lambda x: x[0], reverse=True)
    return out


def pmc_traffic(workload, kernel, with_tag=False):
    """HBM bytes per launch of `kernel` in `workload` from the newest committed
    PMC pass that measured it (2 x FETCH_SIZE + WRITE_SIZE per the MI355X
    guide's gfx950 correction), or None; with_tag: (bytes, profile tag)."""
    for _, tag, wl, nm in _pmc_files():
        if wl is not None and wl != workload:
            continue
        try:
            with open(os.path.join(ROOT, "profiles", nm)) as f:
                d = json.load(f)
            d = d if wl is not None else d.get(workload, {})
            v = d.get(kernel)
            if v is None:   # the library's kernel id names the family (beta_planes: k_beta_planes_c, ...)
                v = next((d[k] for k in sorted(d) if k.startswith(kernel + "_")), None)
        except (OSError, ValueError, AttributeError):
            continue
        if v is not None:
            return (v, tag) if with_tag else v
    return (None, None) if with_tag else None


def make_workload(w, rank):
    """Obstacle configuration k = rank: x without replacement from the
    extended grid {35, 40, ...}, y in {-1.75, 1.75} (S/main_mpc.py:10-21,
    SURVEY §8d), then idx_mpc = randint(1, 10000) (S/main_mpc.py:114)."""
    from optimizer.cem_helper import Helper  # noqa: F401  (drop-in package import check)
    O = w["num_obs"]
    init = np.array([0.0, 1.75, 5.0, 0.0, 0.0, 0.0], np.float32)          # S/main_mpc.py:46-54
    mean = np.array([15] * 4 + [0] * 4, np.float32)                       # S/main_mpc.py:58-71
    cov = np.diag([20.0] * 4 + [100.0] * 4).astype(np.float32)
    if w.get("variant") == "dynamic":
        # synthetic_dynamic_obs/main_mpc.py:34-41,106-129 (ego in the right lane; QP obstacle tracks)
        from optimizer.obs_data_generate_dynamic import dynamic_obstacles
        d = dynamic_obstacles(rank, O)
        init = np.array([0.0, -1.75, 5.0, 0.0, 0.0, 0.0], np.float32)
        return dict(idx_mpc=d["idx_mpc"], init=init, mean=mean, cov=cov, xo=d["x_traj"], yo=d["y_traj"],
                    v_des=15.0)
    rs = np.random.RandomState(rank)
    xs = np.arange(35, 35 + 5 * max(9, O), 5, dtype=np.float64)
    x = rs.choice(xs, O, replace=False)
    y = rs.choice(np.array([-1.75, 1.75]), O)
    idx_mpc = int(rs.randint(1, 10000))
    # static obstacles: constant position over the 100-point plan (cem_helper.py:366-378 with v = 0)
    xo = np.repeat(x[:, None], 100, axis=1).astype(np.float32)
    yo = np.repeat(y[:, None], 100, axis=1).astype(np.float32)
    return dict(idx_mpc=idx_mpc, init=init, mean=mean, cov=cov, xo=xo, yo=yo, v_des=15.0)


def cpu_baseline(w, inst, seconds):
    """NumPy oracle (the CPU restatement of the reference) on a bounded sample
    of one step of the same workload: the batch-wide stages (guess +
    projection + controls, elite sorts + CEM update) on all B candidates and
    the per-candidate risk stage on the first c candidates, scaled to B."""
    import oracle
    try:
        from threadpoolctl import threadpool_info
        threads = max([d.get("num_threads", 1) for d in threadpool_info()] + [1])
    except Exception:
        threads = 1
    B = w["num_batch"]
    ora = oracle.CEM(w["num_reduced"], w["num_obs"], w["level"], w["num_prime"], w["noise"], 0.0, 0.0,
                     num_batch=B, maxiter_cem=1, variant=w.get("variant", "static"))
    draws = oracle.Draws.philox(ora.prob, inst["idx_mpc"], seed=0, with_beta_cem=(w["cost"] == "mmd_opt"))
    st = ora.init_state(inst["init"], inst["mean"], inst["cov"], draws)
    t0 = time.perf_counter()
    pr, acc, steer = ora.front(st)
    t_front = time.perf_counter() - t0
    # risk on growing candidate counts until the time budget is spent
    c, t_risk = 0, 0.0
    obs = np.zeros(B, np.float32)
    lane = np.zeros(B, np.float32)
    while c < B and t_risk < seconds:
        step = 1 if w["cost"] == "mmd_opt" else min(B - c, 64)
        t0 = time.perf_counter()
        o, l, _ = ora.candidate_costs(w["cost"], st, acc[c:c + step], steer[c:c + step], inst["xo"], inst["yo"],
                                      draws, 0)
        t_risk += time.perf_counter() - t0
        obs[c:c + step], lane[c:c + step] = o, l
        c += step
    t0 = time.perf_counter()
    n = w["num_reduced"]
    extra = dict(beta=np.full((B, n), np.float32(1.0 / n)), sigma=np.full(B, np.float32(0.01)),
                 res_beta=np.zeros((B, 20), np.float32))
    ora.select(w["cost"], st, 0, pr, steer, obs, lane, np.float32(inst["v_des"]), draws, extra)
    t_select = time.perf_counter() - t0
    t_step = t_front + t_risk * (B / c) + t_select
    return {"value": 1.0 / t_step, "unit": "steps/s", "cores": int(threads), "kind": "port",
            "sample": (f"oracle (NumPy restatement of the reference) one CEM step: front+select on all {B} "
                       f"candidates ({t_front + t_select:.2f} s), risk stage on {c} of {B} candidates "
                       f"({t_risk:.1f} s) scaled x{B / c:.1f}; BLAS threads {threads}")}


def run_workload(name, steps, warmup, profile_steps, rank, world, local, dist=None, full=True):
    """Time `steps` steps of workload `name` on this rank's GPU.  Returns the
    timing record (rank-local elapsed time; the caller max-reduces it).
    full: also run the profiled pass (per-kernel times and the roofline)."""
    import torch
    from optimizer import _native

    w = WORKLOADS[name]
    inst = make_workload(w, rank)
    T = 20
    cfg = _native.make_config(w["num_reduced"], w["num_obs"], w["level"], w["num_prime"], w["noise"], 0.0, 0.0,
                              num_batch=w["num_batch"], maxiter_cem=T, device=local, seed=rank,
                              variant=w.get("variant", "static"))
    h = _native.Handle(cfg)
    stream = torch.cuda.Stream()  # a created stream (the legacy default stream cannot be graph-captured)
    h.set_stream(stream.cuda_stream)

    def run(k0, count, evs=None):
        for i in range(k0, k0 + count):
            t = i % T
            if t == 0:
                h.begin(w["cost"], inst["idx_mpc"], inst["init"], inst["mean"], inst["cov"], inst["xo"], inst["yo"],
                        inst["v_des"])
            h.iterate(t, 1)
            if evs is not None:
                evs[i - k0 + 1].record(stream)

    run(0, warmup)
    h.sync()
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    t0 = time.perf_counter()
    evs[0].record(stream)
    run(0, steps, evs)
    h.sync()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    step_ms = np.array([evs[i].elapsed_time(evs[i + 1]) for i in range(steps)])
    res = h.finish()
    if not full:
        h.close()
        return dict(w=w, elapsed=elapsed, step_ms=step_ms, res=res, inst=inst)
    # profiled pass (same steps, HIP events around every launch on the library's stream)
    h.write("stats", np.zeros(8, np.uint64))
    h.profile(True)
    run(0, profile_steps)
    h.sync()
    kt = h.kernel_times()
    h.profile(False)
    stats = h.read("stats", np.uint64).astype(np.int64)
    h.close()
    busy = {k: v for k, v in kt.items() if v[0] > 0}
    dom = max(busy, key=lambda k: busy[k][1])
    launches, tot_ms = busy[dom]
    avg_s = tot_ms / launches / 1e3
    roof = {"bound": None, "achieved": None, "peak": None, "unit": None, "frac": None}
    model = kernel_work(w, dom, launches, stats)
    if model is not None:
        bound, unit, amount, peak = model[:4]
        scale = model[4] if len(model) > 4 else 1e12  # unit of `achieved` (T/s; GB/s for HBM bounds)
        roof.update(bound=bound, unit=unit, peak=peak, achieved=amount / launches / avg_s / scale)
        roof["frac"] = roof["achieved"] / peak
    roof["traffic"], roof["traffic_profile"] = pmc_traffic(name, dom, with_tag=True)
    roof["kernel"] = dom
    roof["avg_us"] = avg_s * 1e6
    if w["cost"] == "mmd_opt":  # k_bkernel work counters over the profiled pass
        roof["bkernel_counts"] = {"direct_rows": int(stats[0]), "direct_pairs": int(stats[1]),
                                  "series_pairs": int(stats[2]), "kred_entries": int(stats[3])}
    roof["step"] = step_roofline(w, busy, profile_steps, stats, elapsed / steps * 1e3, name)
    return dict(w=w, elapsed=elapsed, step_ms=step_ms, res=res, roof=roof, inst=inst,
                kernels={k: v[1] / profile_steps for k, v in busy.items()})


CARLA = os.path.join(PKG, "carla")
# BASELINE configs[4]: the CARLA optimizer (carla/optimizer/cem.py), mmd_opt + cvar back to back per
# simulator tick at H = 60, num_batch 100 (cem.py:138), num_obs 3 (README CARLA commands), replayed ticks
CARLA_WORKLOAD = dict(desc="CARLA replay (synthetic Town05 recording), compute_cem_mmd + compute_cem_cvar back to "
                           "back per tick, H=60, num_batch=100, num_obs=3, num_reduced_set={n} (mmd: {M} mother rows)",
                      baseline="configs[4]", num_reduced=10, num_obs=3, num_prime=60, noise="gaussian", level=0.1,
                      num_batch=100, town="Town05", budget_ms=50.0)


def _carla_modules():
    """The CARLA drop-in package (named ``optimizer`` like the static one) and
    the replay module, loaded under aliases."""
    import importlib
    import importlib.util
    name = "mpcmmd_carla_optimizer"
    if name not in sys.modules:
        d = os.path.join(CARLA, "optimizer")
        spec = importlib.util.spec_from_file_location(name, os.path.join(d, "__init__.py"),
                                                      submodule_search_locations=[d])
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
    spec = importlib.util.spec_from_file_location("mpcmmd_carla_replay", os.path.join(CARLA, "replay.py"))
    rep = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rep)
    return importlib.import_module(name + ".cem"), rep


def run_carla(ticks, warmup, local, n=None, dump=None):
    """Per-tick time of the CARLA loop body on replayed ticks
    (carla/main_carla.py:345-382): the path / obstacle preprocessing through
    the drop-in's helpers, then the solve.  The reference's driver runs ONE
    cost per tick (``--costs`` picks func_cem = compute_cem_mmd, _cvar or _det,
    main_carla.py:188-194, called at :378-382), so a tick of cost c is the
    preprocessing + that solve, each cost carrying its own mean_param to the
    next tick (:378); wall clock (synchronous calls, as the driver makes
    them) against the 50 ms tick of carla_simulation.py:20.  The three solves
    are timed on the same ticks, back to back; "ms_per_tick_mmd_plus_cvar" is
    the stricter mmd + cvar sum earlier rounds reported."""
    import torch
    w = dict(CARLA_WORKLOAD)
    if n is not None:
        w["num_reduced"] = n
    cem, rep = _carla_modules()
    prob = cem.CEM(w["num_reduced"], 1, w["num_obs"], w["level"], w["num_prime"], w["noise"], w["town"], 0.0, 0.0,
                   device=local)
    stride = 5
    rec = rep.record_synthetic(ticks=(warmup + ticks) * stride + 1, town=w["town"])
    mean0 = np.array([10.0] * 4 + [0.0] * 4, np.float32)                  # main_carla.py:306-318
    cov = np.diag([20.0] * 4 + [100.0] * 4).astype(np.float32)
    means = {"mmd_opt": mean0.copy(), "cvar": mean0.copy(), "det": mean0.copy()}
    rows = []
    for i in range(warmup + ticks):
        k = i * stride
        t0 = time.perf_counter()
        init, xo, yo, path = rep.tick_inputs(rec, k, prob.cem_helper, w["num_obs"])
        t1 = time.perf_counter()
        args = (path["x_path"], path["y_path"], path["arc_vec"], path["Fx_dot"], path["Fy_dot"], path["kappa"])
        r1 = prob.compute_cem_mmd(k, init, means["mmd_opt"], cov, xo, yo, 10.0, *args)
        t2 = time.perf_counter()
        r2 = prob.compute_cem_cvar(k, init, means["cvar"], cov, xo, yo, 10.0, *args)
        t3 = time.perf_counter()
        # compute_cem_det (main_carla.py:194, --costs det): the deterministic
        # baseline of the same tick, timed on its own (not part of the
        # mmd + cvar tick)
        r3 = prob.compute_cem_det(k, init, means["det"], cov, xo, yo, 10.0, *args)
        t4 = time.perf_counter()
        means["mmd_opt"], means["cvar"], means["det"] = r1[4], r2[4], r3[4]
        if i >= warmup:
            rows.append((t1 - t0, t2 - t1, t3 - t2, t3 - t0, t4 - t3))
    if dump is not None:  # the last timed tick's result tuples
        names = ("cx", "cy", "v_best", "steering", "mean_param")
        dump_outputs(dump, {f"{c}_{nm}": v for c, r in (("mmd", r1), ("cvar", r2), ("det", r3))
                            for nm, v in zip(names, r)})
    torch.cuda.synchronize()
    a = np.array(rows) * 1e3
    # one profiled tick: per-kernel HIP-event times of both solves
    h = prob.handle
    h.profile(True)
    init, xo, yo, path = rep.tick_inputs(rec, 0, prob.cem_helper, w["num_obs"])
    args = (path["x_path"], path["y_path"], path["arc_vec"], path["Fx_dot"], path["Fy_dot"], path["kappa"])
    prob.compute_cem_mmd(0, init, mean0, cov, xo, yo, 10.0, *args)
    prob.compute_cem_cvar(0, init, mean0, cov, xo, yo, 10.0, *args)
    kt = {k: v for k, v in h.kernel_times().items() if v[0] > 0}
    h.profile(False)
    gpu_ms = sum(v[1] for v in kt.values())
    # the two solves of a tick are independent: a second handle runs cvar on
    # its own stream while the first runs mmd_opt (the driver's sequential
    # calls above are the reference's order)
    prob2 = cem.CEM(w["num_reduced"], 1, w["num_obs"], w["level"], w["num_prime"], w["noise"], w["town"], 0.0, 0.0,
                    device=local)
    h1, h2 = prob.handle, prob2.handle
    conc = []
    for i in range(warmup + ticks):
        k = i * stride
        t0 = time.perf_counter()
        init, xo, yo, path = rep.tick_inputs(rec, k, prob.cem_helper, w["num_obs"])
        h1.carla_begin("mmd_opt", k, init, mean0, cov, xo, yo, 10.0, path)
        h1.iterate(0, prob.maxiter_cem)
        h2.carla_begin("cvar", k, init, mean0, cov, xo, yo, 10.0, path)
        h2.iterate(0, prob2.maxiter_cem)
        h1.finish()
        h2.finish()
        if i >= warmup:
            conc.append(time.perf_counter() - t0)
    conc = np.array(conc) * 1e3
    desc = w["desc"].format(n=w["num_reduced"], M=w["num_reduced"] ** 2)
    tick = {c: a[:, 0] + a[:, j] for c, j in (("mmd_opt", 1), ("cvar", 2), ("det", 4))}
    per_cost = {c: {"ms_per_tick": float(np.mean(v)), "median_ms_per_tick": float(np.median(v)),
                    "p90_ms_per_tick": float(np.percentile(v, 90)),
                    "ticks_within_budget": float(np.mean(v <= w["budget_ms"]))} for c, v in tick.items()}
    return {"baseline": w["baseline"], "workload": desc, "num_reduced_set": w["num_reduced"], "ticks": ticks,
            "value": 1e3 / per_cost["mmd_opt"]["ms_per_tick"], "unit": "ticks/s (--costs mmd_opt)",
            "tick": "main_carla.py:188-194: one cost per tick = preprocessing + that solve",
            "per_cost": per_cost, "budget_ms": w["budget_ms"],
            "ms_per_tick_mmd_plus_cvar": float(np.mean(a[:, 3])),
            "ticks_within_budget_mmd_plus_cvar": float(np.mean(a[:, 3] <= w["budget_ms"])),
            "ms_preprocess": float(np.mean(a[:, 0])), "ms_mmd": float(np.mean(a[:, 1])),
            "ms_cvar": float(np.mean(a[:, 2])),
            "ms_det": float(np.mean(a[:, 4])), "median_ms_det": float(np.median(a[:, 4])),
            "ms_per_tick_two_streams": float(np.mean(conc)),
            "profiled_tick_gpu_ms": gpu_ms,
            "profiled_note": "profiled tick: HIP events around every launch serialise the candidate groups and add "
                             "gaps, so profiled_tick_gpu_ms / kernels_ms_per_tick exceed the wall-clock tick; the "
                             "rocprofv3 kernel trace (profiles/*_carla_tick_breakdown.txt) is the kernel-time evidence",
            "kernels_ms_per_tick": {k: v[1] for k, v in kt.items()},
            "launches_per_tick": int(sum(v[0] for v in kt.values()))}


def dump_outputs(path, arrays):
    """--dump-outputs: each array of `arrays` as <path>/<name>.npy in float32
    (float64 stays float64)."""
    os.makedirs(path, exist_ok=True)
    for name, v in arrays.items():
        v = np.asarray(v)
        np.save(os.path.join(path, f"{name}.npy"), v if v.dtype == np.float64 else v.astype(np.float32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workload", default="mmd_opt", choices=sorted(WORKLOADS) + ["carla"])
    ap.add_argument("--full", action="store_true",
                    help="also the profiled pass (roofline, per-kernel times), the CPU baseline and, at N = 1, the "
                         "other BASELINE workloads")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step's solve returns as DIR/<name>.npy")
    ap.add_argument("--cpu-seconds", type=float, default=15.0, help="--full: CPU baseline budget (0 = skip)")
    ap.add_argument("--profile-steps", type=int, default=20, help="--full: steps of the profiled pass")
    ap.add_argument("--extra", type=int, default=1,
                    help="--full, N = 1: also time the other BASELINE workloads (0 = skip)")
    ap.add_argument("--carla-n", type=int, default=10, help="--workload carla: num_reduced_set (10 or 22)")
    a = ap.parse_args()

    import torch
    import torch.distributed as dist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != a.gpus:
        raise SystemExit(f"--gpus {a.gpus} but WORLD_SIZE={world} (launch N>1 with torchrun)")
    torch.cuda.set_device(local)
    if a.workload == "carla":  # configs[4] alone (one GPU, a real-time tick loop: no sharding)
        print(json.dumps({"metric": "CARLA ticks/s (one compute_cem_* per tick, main_carla.py:188-194)",
                          **run_carla(a.steps, a.warmup, local, n=a.carla_n, dump=a.dump_outputs)}), flush=True)
        return
    if world > 1:
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    r = run_workload(a.workload, a.steps, a.warmup, a.profile_steps, rank, world, local, dist if world > 1 else None,
                     full=a.full)
    elapsed = r["elapsed"]
    res = r["res"]
    if world > 1:
        el = torch.tensor([elapsed], dtype=torch.float64, device="cuda")
        dist.all_reduce(el, op=dist.ReduceOp.MAX)
        elapsed = float(el.item())
        dist.barrier()
    # final gather of per-config results over RCCL (§8e)
    vec = np.concatenate([res["cx"], res["cy"], [res["cost_lane"], res["cost_obs"]]]).astype(np.float32)
    if world > 1:
        vt = torch.from_numpy(vec).cuda()
        allv = [torch.empty_like(vt) for _ in range(world)]
        dist.all_gather(allv, vt)
        gathered = torch.stack(allv).cpu().numpy()
    else:
        gathered = vec[None]
    if rank == 0:
        w = r["w"]
        T = 20
        value = a.steps * world / elapsed
        line = {
            "metric": METRIC, "value": value, "unit": "steps/s", "n_gpus": world, "steps": a.steps,
            "warmup": a.warmup, "ms_per_step": elapsed / a.steps * 1e3, "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "f32",
            "data": f"synthetic ({w.get('variant', 'static')} obstacle configs k=rank, internal Philox noise)",
            "config": {"workload": w["desc"], "baseline": w["baseline"], "cost": w["cost"],
                       "global_batch": w["num_batch"] * world, "num_batch": w["num_batch"],
                       "num_prime": w["num_prime"], "num_obs": w["num_obs"], "num_reduced": w["num_reduced"],
                       "noise": w["noise"], "noise_level": w["level"], "parallelism": f"config-sharded x{world}",
                       "solves_per_s": value / T,
                       # dtype f32 is the reference's arithmetic (JAX default); parts of the path run wider
                       "wider_arithmetic": ("beta-CEM sampler k_bsample: fp64 MFMA (v_mfma_f64_16x16x4); "
                                            "KKT / basis products, projection transcendentals, Beta sampling: fp64"
                                            if w["cost"] == "mmd_opt" else
                                            "KKT / basis products, projection transcendentals, Beta sampling: fp64")},
            "median_ms_per_step": float(np.median(r["step_ms"])),
            "results_gathered": int(gathered.shape[0]),
        }
        if a.dump_outputs:
            dump_outputs(a.dump_outputs, res)
        if a.full:
            line["roofline"] = r["roof"]
            line["kernels_ms_per_step"] = r["kernels"]
        if a.full and world == 1 and a.cpu_seconds > 0:
            line["cpu_baseline"] = cpu_baseline(w, r["inst"], a.cpu_seconds)
        if a.full and world == 1 and a.extra:
            extra = {}
            for name in WORKLOADS:
                if name == a.workload:
                    continue
                steps = max(20, a.steps // (5 if name == "configs0" else 1))
                x = run_workload(name, steps, 2, 20, rank, 1, local)
                extra[name] = {"baseline": x["w"]["baseline"], "workload": x["w"]["desc"],
                               "value": steps / x["elapsed"], "unit": "steps/s", "steps": steps,
                               "ms_per_step": x["elapsed"] / steps * 1e3,
                               "median_ms_per_step": float(np.median(x["step_ms"])),
                               "solves_per_s": steps / x["elapsed"] / T, "roofline": x["roof"],
                               "kernels_ms_per_step": x["kernels"]}
                if name == "cvar" and a.cpu_seconds > 0:   # configs[2]: the workload where 10k steps/s is reachable
                    extra[name]["cpu_baseline"] = cpu_baseline(x["w"], x["inst"], min(a.cpu_seconds, 10.0))
            for nn in (10, 22):  # configs[4]: num_reduced_set 10 (the line's workload) and 22 (configs[1]'s n)
                extra["carla" if nn == 10 else f"carla_n{nn}"] = run_carla(ticks=10, warmup=2, local=local, n=nn)
            line["extra_workloads"] = extra
        print(json.dumps(line), flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
