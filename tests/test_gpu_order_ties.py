"""Exact ties and special values in the device argsorts / argmins (DESIGN.md
section 5): the beta-CEM's top-n |beta| rows (select_walk: k_bselect, every
instantiation, and the fused k_bcem_small), k_belite's elite ranking and
argmin, and k_select's obstacle elites, cost elites and result row, driven
with the patterns of tie_patterns.py.  Every index comparison is exact
integer equality with the oracle's stable order (oracle.helper.argsort_stable,
oracle.beta_cem.select_top / argmin_nan): no near-tie excuse, no row skipped.
"""
import numpy as np
import pytest

import bench
import oracle
import tie_patterns as tp
from oracle import beta_cem as bc
from oracle import helper as Hh
from parity import DEFAULT_COV, DEFAULT_INIT, DEFAULT_MEAN, close, make_pair
from test_gpu_parity_mmdopt import _samples_from_elites

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
NAN = np.float32(np.nan)


# ------------------------------------------------------------------ beta-CEM
def _begin_mother(native, n, B, z0, beta_z=None, seed=3):
    """make_pair + begin + stages 1 and 4 (test_beta_cem_lockstep's _run_mother) with the given beta draws."""
    ora, nat, xo, yo = make_pair(native, "mmd_opt", "gaussian", n=n, O=3, H=10, B=B, T=2, acc_c=0.05, steer_c=0.01)
    draws = oracle.Draws.random(ora.prob, np.random.default_rng(seed), idx_mpc=11, seed=0, with_beta_cem=True)
    draws.beta_z0 = np.ascontiguousarray(z0, F32)
    if beta_z is not None:
        draws.beta_z = np.ascontiguousarray(beta_z, F32)
    nat.begin("mmd_opt", 11, DEFAULT_INIT, DEFAULT_MEAN, DEFAULT_COV, xo, yo, 15.0, draws)
    nat.run_stage(1, 0)
    nat.run_stage(4, 0)
    return ora, nat, draws


def _first_samples(z0, M):
    s0 = tp.scaled(z0)
    s0[:, M] = np.maximum(s0[:, M], F32(0.01))
    return s0


def _new_samples(nat, B, M):
    """The GPU's own new samples of the current beta-iteration (Params::ygen: [B][96][M + 1 rounded to 32])."""
    ys = (M + 1 + 31) & ~31
    return nat.read("ygen").reshape(-1, 96, ys)[:B, :89, :M + 1].copy()


@pytest.mark.parametrize("n", tp.BSELECT_N)
def test_bselect_first_iteration_patterns(native, n):
    """k_bselect<NQ, R, G> of every size class on 100 pattern rows (the nine
    patterns, fresh seeds, cycled): the window on every key, the group-maxima
    window, its overflow into the bisection, and emit_top's tie branch
    (test_tie_patterns.py shows which rows reach which).  begin and stages 1,
    4 and 5 only."""
    B, M = 20, n * n
    rows = []
    for k in range(12):
        rows += list(tp.beta_rows(M, n, np.random.default_rng(7919 * n + k)).values())
    z0 = np.stack(rows[:100])
    ora, nat, _ = _begin_mother(native, n, B, z0)
    try:
        nat.run_stage(5, 0)
        bsel = nat.read("bsel", np.int32).reshape(-1, 100, n)[:B]
        sel0 = nat.read("sel0", np.int32).reshape(100, n)
        bsig = nat.read("bsig").reshape(-1, 100)[:B]
    finally:
        nat.close()
    s0 = _first_samples(z0, M)
    want = bc.select_top(s0, M, n)
    names = (list(tp.beta_rows(M, n, np.random.default_rng(0))) * 12)[:100]
    for s in range(100):
        assert np.array_equal(bsel[0, s], want[s]), f"n={n} row {s} ({names[s]}): {bsel[0, s]} vs {want[s]}"
    assert np.array_equal(sel0, want), "sel0 (the host's copy of the first selection)"
    assert np.array_equal(bsig[0], s0[:, M]), "sigma column (clipped at 0.01)"
    for b in range(1, B):
        assert np.array_equal(bsel[b], bsel[0]) and np.array_equal(bsig[b], bsig[0]), f"candidate {b}"


TWO_LEVEL = [(6, "even_odd", "window_all"), (10, "even_odd", "window_group"), (10, "three_quarters", "overflow_ties"),
             (16, "even_odd", "overflow_ties"), (22, "even_odd", "overflow_ties")]   # test_tie_patterns.py's


@pytest.mark.parametrize("n,layout,path", TWO_LEVEL)
def test_beta_iterations_two_level_ties(native, n, layout, path):
    """Beta-iterations 0..3 in sub-stage lockstep on two-level draws with
    beta_z[0] = 0: every first sample has two tie classes, any elite mean keeps
    them, and the 89 new samples of iteration 1 equal that mean (``path``: the
    select_walk path of those rows, test_tie_patterns.py).  Selections exact
    against the oracle's samples and against the GPU's own; the tied samples'
    row sums, QP solutions and costs bit-identical; the elites those of the
    stable cost order."""
    B, M = 20, n * n
    rng = np.random.default_rng(100 + n)
    z0 = tp.two_level_z0(M, rng, layout)
    z = rng.standard_normal((20, 89, M + 1)).astype(F32)
    z[0] = 0.0
    ora, nat, _ = _begin_mother(native, n, B, z0, z)
    try:
        NQ, R, G = tp.bselect_instance(n)
        feat = nat.read("feat").reshape(-1, 22, M)[:B]
        Fb = {b: np.ascontiguousarray(feat[b].T) for b in (0, 7, 19)}   # the QP checks' candidates
        Db = {b: bc.distance_matrix(Fb[b]) if M > 256 else None for b in Fb}
        samples = np.broadcast_to(_first_samples(z0, M), (B, 100, M + 1)).copy()   # the oracle's
        own = samples.copy()                                                       # the GPU's
        for tb in range(4):
            nat.run_stage(5, tb)
            bsel = nat.read("bsel", np.int32).reshape(-1, 100, n)[:B]
            bsig = nat.read("bsig").reshape(-1, 100)[:B]
            if tb > 0:
                own[:, 11:] = _new_samples(nat, B, M)
            for b in range(B):
                assert np.array_equal(bsel[b], bc.select_top(own[b], M, n)), f"bsel[tb={tb}, b={b}] (own samples)"
                if tb <= 2:
                    assert np.array_equal(bsel[b], bc.select_top(samples[b], M, n)), f"bsel[tb={tb}, b={b}]"
                close(f"bsig[{tb},{b}]", bsig[b], samples[b][:, M], rtol=1e-6, atol=0)
            if tb == 1:
                assert np.array_equal(own[:, 11:], samples[:, 11:]), "new samples of iteration 1: the elite mean"
                assert all(tp.select_path(own[b, 11], M, n, NQ, R, G) == path for b in range(B))
            nat.run_stage(6, tb)
            btop = nat.read("btop").reshape(-1, 100, n)[:B]
            bcost = nat.read("bcost").reshape(-1, 100)[:B]
            brow = nat.read("brow").reshape(-1, 100, n)[:B]
            if tb == 1:   # 89 identical samples: nothing may depend on the sample slot
                for name, a in (("brow", brow), ("btop", btop), ("bcost", bcost[:, :, None])):
                    assert np.array_equal(a[:, 11:], np.broadcast_to(a[:, 11:12], a[:, 11:].shape), equal_nan=True), \
                        f"{name}: the tied samples of iteration 1 differ"
            for b in Fb:
                beta, cost, _, rowsum = bc.reduced_qp(ora.prob, Fb[b], bsel[b].astype(np.int64), bsig[b], M, Db[b])
                s_lo = 11 if tb > 0 else 0
                close(f"brow[{tb},{b}]", brow[b, s_lo:], rowsum[s_lo:], rtol=1e-5, atol=0)
                close(f"btop[{tb},{b}]", btop[b], beta, rtol=1e-3, atol=1e-4)
                close(f"bcost[{tb},{b}]", bcost[b], cost, rtol=1e-4, atol=1e-4)
            nat.run_stage(7, tb)
            bel = nat.read("belite").reshape(2, -1, 11, M + 1)[(tb + 1) & 1][:B]
            res_beta = nat.read("res_beta").reshape(-1, 20)[:B]
            for b in range(B):
                idx_e = Hh.argsort_stable(bcost[b])[:11]
                assert np.array_equal(bel[b], own[b][idx_e]), f"elites[tb={tb}, b={b}]: not the stable cost order's"
                if tb <= 1:
                    assert np.array_equal(bel[b], samples[b][idx_e]), f"elites[tb={tb}, b={b}] (oracle's samples)"
                assert res_beta[b, tb] == np.min(bcost[b])
                samples[b] = np.vstack([bel[b], _samples_from_elites(bel[b], z[tb], M)])
                own[b, :11] = bel[b]
    finally:
        nat.close()


def _tie_costs(rng, b):
    """A tie-heavy cost vector [100] for candidate b."""
    pool = np.array([0.0, -0.0, 1e-30, 2.5, np.inf, np.nan], F32)
    c = np.where(rng.random(100) < 0.6, pool[rng.integers(0, pool.size, 100)],
                 rng.standard_normal(100).astype(F32)).astype(F32)
    if b == 1:
        c[:] = F32(0.75)                    # all equal
    elif b == 2:
        c[:] = NAN                          # all NaN
    elif b == 3:
        c = rng.standard_normal(100).astype(F32)
        c[57] = NAN                         # one NaN
    elif b == 4:
        c = np.where(np.isnan(c), F32(2.5), c)   # ties and inf, no NaN
    elif b == 5:
        c[:] = F32(np.inf)
        c[rng.permutation(100)[:5]] = F32(-0.0)   # fewer finite costs than elites
    return c


def test_belite_ranking_ties(native):
    """k_belite on injected costs: the stable rank of 100 costs with +-0, tiny,
    equal, inf and NaN values (elites), the minimum or NaN (res_beta), and at
    the last iteration jnp.argmin's index (first NaN, else first minimum) for
    bestsel / beta / sigma.  Injection after stage 6 of iterations 0, 1 and 19;
    the iterations between run unmodified."""
    n, B = 6, 20
    M = n * n
    rng = np.random.default_rng(17)
    ora, nat, draws = _begin_mother(native, n, B, rng.standard_normal((100, M + 1)).astype(F32), seed=17)
    try:
        own = np.broadcast_to(_first_samples(draws.beta_z0, M), (B, 100, M + 1)).copy()
        for tb in range(20):
            nat.run_stage(5, tb)
            if tb > 0:
                own[:, 11:] = _new_samples(nat, B, M)
            nat.run_stage(6, tb)
            inject = tb in (0, 1, 19)
            if inject:
                costs = np.stack([_tie_costs(rng, b) for b in range(B)])
                nat.write("bcost", costs)
            bcost = nat.read("bcost").reshape(-1, 100)[:B].copy()
            if inject:
                assert np.array_equal(bcost.view(np.uint32), costs.view(np.uint32))
            bsel = nat.read("bsel", np.int32).reshape(-1, 100, n)[:B].copy()
            btop = nat.read("btop").reshape(-1, 100, n)[:B].copy()
            nat.run_stage(7, tb)
            bel = nat.read("belite").reshape(2, -1, 11, M + 1)[(tb + 1) & 1][:B]
            res_beta = nat.read("res_beta").reshape(-1, 20)[:B]
            for b in range(B):
                idx_e = Hh.argsort_stable(bcost[b])[:11]
                assert np.array_equal(bel[b], own[b][idx_e], equal_nan=True), f"elites[tb={tb}, b={b}]: {idx_e}"
                want = NAN if np.isnan(bcost[b]).any() else np.min(bcost[b])
                assert np.array_equal(res_beta[b, tb], want, equal_nan=True), f"res_beta[tb={tb}, b={b}]"
                own[b, :11] = bel[b]
            if tb == 19:
                best = nat.read("bestsel", np.int32).reshape(-1, n)[:B]
                beta = nat.read("beta").reshape(-1, n)[:B]
                sigma = nat.read("sigma")[:B]
                for b in range(B):
                    imin = bc.argmin_nan(bcost[b])
                    assert np.array_equal(best[b], bsel[b, imin]), f"bestsel[{b}]: not sample {imin}'s rows"
                    assert np.array_equal(beta[b], btop[b, imin], equal_nan=True), f"beta[{b}]"
                    # sigma_best: the argmin's slot of the NEXT samples (Q4) -- an elite row if imin < 11, else
                    # the new sample imin - 11 drawn with the updated generators (checked to the lockstep's tolerance)
                    nxt = np.vstack([bel[b], _samples_from_elites(bel[b], draws.beta_z[19], M)])
                    close(f"sigma_best[{b}]", sigma[b], nxt[imin, M], rtol=1e-6, atol=0)
                assert len({bc.argmin_nan(bcost[b]) for b in range(B)}) >= 6
                assert any(bc.argmin_nan(bcost[b]) >= 11 for b in range(B))
    finally:
        nat.close()


# ------------------------------------------------------------------ k_select
def _cvar(native, monkeypatch, prep, B, T=1):
    monkeypatch.setenv("MPCMMD_SELECT_PREP", prep)   # read when the handle is created
    w = dict(bench.WORKLOADS["cvar"], num_batch=B, num_reduced=16)
    inst = bench.make_workload(w, 0)
    cfg = native.make_config(16, w["num_obs"], w["level"], w["num_prime"], "gaussian", 0.0, 0.0, num_batch=B,
                             maxiter_cem=T)
    h = native.Handle(cfg)
    assert h.info("select_prep") == int(prep)

    def begin():   # a fresh solve: stages 0, 1, 2 of iteration 0 done, stage 3 pending
        h.begin("cvar", inst["idx_mpc"], inst["init"], inst["mean"], inst["cov"], inst["xo"], inst["yo"],
                inst["v_des"])
        for s in (0, 1, 2):
            h.run_stage(s, 0)
    return h, begin, (w["num_obs"], w["level"], w["num_prime"])


def _obs_patterns(rng, B):
    few = np.where(rng.random(B) < 0.5, F32(0.0), F32(-0.0)).astype(F32)
    k = min(19, B - 1)
    few[rng.permutation(B)[:k]] = rng.choice(np.array([0.5, 0.5, 1e-30, 3.0], F32), k)
    pool = np.array([0.0, -0.0, 1e-30, 0.25, 0.25, 7.0, np.inf, np.nan], F32)
    mixed = pool[rng.integers(0, pool.size, B)]
    heavy = np.full(B, NAN, F32)           # more than B - 20 NaNs: NaNs enter the elites
    heavy[rng.permutation(B)[:min(13, B - 1)]] = rng.choice(np.array([0.0, -0.0, 2.0, np.inf], F32), min(13, B - 1))
    return dict(zeros=np.zeros(B, F32), few_nonzero=few, mixed=mixed, nan_heavy=heavy)


@pytest.mark.parametrize("prep", ["1", "0"])
@pytest.mark.parametrize("B", [20, 21, 100, 777, 1024, 1500])
def test_obstacle_elites_ties(native, monkeypatch, B, prep):
    """k_select's 20 obstacle elites over the permuted batch on tied costs:
    block_smallest's window (20 <= B <= 1024; B = 20: fewer groups than elites)
    and the LDS bitonic network (B = 1500), with both select preparations."""
    h, begin, _ = _cvar(native, monkeypatch, prep, B)
    rng = np.random.default_rng(B)
    try:
        for name, obs in _obs_patterns(rng, B).items():
            begin()
            h.write("obs_cost", obs)
            h.run_stage(3, 0)
            h.sync()
            perm = h.read("tr_proj", np.int32)[:B].astype(np.int64)
            assert np.array_equal(np.sort(perm), np.arange(B))
            got = h.read("tr_obs", np.int32)[:20]
            want = perm[Hh.argsort_stable(obs[perm])][:20]
            assert np.array_equal(got, want), f"B={B} prep={prep} {name}: {got} vs {want}"
    finally:
        h.close()


def _cost20(res, cnorm, obs, lane, el, w_obs, w_lane):
    """oracle.helper.compute_cost's total (cem_helper.py:254-262) from the
    eleven norms the device keeps (Params::cnorm: des, st, sv, sa, v, sp, svp,
    ydd, xdd, des2, cen): fp64 in the reference's order, rounded once."""
    nk = cnorm[el]
    cobs = (F32(w_obs) * obs[el]).astype(F32).astype(F64)
    clane = (F32(w_lane) * lane[el]).astype(F32).astype(F64)
    with np.errstate(invalid="ignore"):
        tot = (res[el].astype(F64) + 0.1 * nk[:, 4] + 0.1 * (nk[:, 1] + nk[:, 2] + nk[:, 3])
               + 0.1 * (nk[:, 5] + nk[:, 6]) + 0.02 * nk[:, 7] + 0.02 * nk[:, 8] + 0.0 * nk[:, 0] + cobs + 0.0 * clane)
    return tot.astype(F32)


@pytest.mark.parametrize("prep", ["1", "0"])
@pytest.mark.parametrize("B", [100, 1500])
def test_cost_elites_and_result_ties(native, monkeypatch, B, prep):
    """The stable top 5 by total cost of the 20 obstacle elites and the result
    row (elite ``argmin_nan`` of those five) on tied totals: identical rows,
    three cost levels, NaN totals among the twenty, and so many NaNs that one
    is among the five (jnp.argmin: the first NaN)."""
    h, begin, (O, level, H) = _cvar(native, monkeypatch, prep, B)
    w_obs, w_lane = oracle.CEM(16, O, level, H, "gaussian", 0.0, 0.0, num_batch=B, maxiter_cem=1).weights("cvar")
    rng = np.random.default_rng(B + 1)
    mins = []
    try:
        for name in ("identical", "three_level", "nan_middle", "nan_most"):
            begin()
            cn = np.tile(rng.uniform(0.5, 2.0, 12), (B, 1))
            res = np.full(B, F32(0.125), F32)
            obs = np.zeros(B, F32)
            lane = np.full(B, F32(0.5), F32)
            if name != "identical":
                cn[:, 4] = rng.integers(1, 4, B).astype(F64)          # three levels of the velocity norm
                obs = rng.choice(np.array([0.0, -0.0, 1.0], F32), B, p=[0.45, 0.45, 0.1])
                res = rng.choice(np.array([0.125, 0.375], F32), B)
            # the obstacle elites these inputs give (the order of the residuals is known before stage 3)
            perm0 = h.read("tr_proj", np.int32)[:B].astype(np.int64) if prep == "1" else Hh.argsort_stable(res)
            el0 = perm0[Hh.argsort_stable(obs[perm0])][:20]
            if name == "nan_middle":   # 0 * NaN: a NaN total, at elite positions 7 and 12 and elsewhere
                lane[rng.random(B) < 0.2] = NAN
                lane[el0[:7]] = F32(0.5)
                lane[el0[[7, 12]]] = NAN
            if name == "nan_most":     # only elites 4 and 9 finite: three of the five are NaN
                lane[:] = NAN
                lane[el0[[4, 9]]] = F32(0.5)
            for k, v in (("cnorm", cn), ("res_norm", res), ("obs_cost", obs), ("lane_cost", lane)):
                h.write(k, v)
            h.run_stage(3, 0)
            h.sync()
            cn_g = h.read("cnorm", F64).reshape(-1, 12)[:B]
            res_g, obs_g, lane_g = (h.read(k)[:B] for k in ("res_norm", "obs_cost", "lane_cost"))
            assert np.array_equal(cn_g, cn) and np.array_equal(lane_g, lane, equal_nan=True)
            perm = h.read("tr_proj", np.int32)[:B].astype(np.int64)
            if prep == "0":   # sorted by k_select from the residuals written above
                assert np.array_equal(perm, Hh.argsort_stable(res_g))
            el = perm[Hh.argsort_stable(obs_g[perm])][:20]
            assert np.array_equal(h.read("tr_obs", np.int32)[:20], el) and np.array_equal(el, el0), name
            cost20 = _cost20(res_g, cn_g, obs_g, lane_g, el, w_obs, w_lane)
            idx = Hh.argsort_stable(cost20)[:5]
            got = h.read("tr_cem", np.int32)[:5]
            assert np.array_equal(got, idx), f"B={B} prep={prep} {name}: cost elites {got} vs {idx}; costs {cost20}"
            imin = bc.argmin_nan(cost20[idx])
            mins.append(imin)
            e = el[imin]
            row = h.read("results")[:24]
            cx, cy = h.read("cx").reshape(-1, 11)[e], h.read("cy").reshape(-1, 11)[e]
            want = np.concatenate([cx, cy, [lane_g[e], obs_g[e]]]).astype(F32)
            assert np.array_equal(row, want, equal_nan=True), f"B={B} prep={prep} {name}: result row of elite {imin}"
            if name == "identical":
                assert np.array_equal(idx, np.arange(5)) and np.unique(cost20).size == 1
            if name == "nan_middle":
                assert np.isnan(cost20).any() and not np.isnan(cost20[idx]).any()
        assert max(mins) > 0, "no case with a NaN among the five cost elites"
    finally:
        h.close()
