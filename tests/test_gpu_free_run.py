"""Unsynchronised end-to-end solves: the GPU and the oracle each run the whole
20-iteration CEM on their own carries (no state is copied between them),
from the same injected draws, on a scenario whose obstacles block the ego
lane inside the rollout horizon, so the optimum is not trivial (collisions
are possible and the CEM has to steer around them).

Per outer iteration the GPU's per-candidate costs and elite index sets are
read back and compared with the oracle's trace.  Every run must reach the
last iteration in lockstep -- identical elite sets in all 20 iterations --
and the results must agree: cx[11], cy[11], cost_obs, cost_lane (and beta,
sigma, res_beta for mmd_opt) within 1e-4 relative (S/opt/cem.py:320-333,
Q1: the result is the last iteration's obstacle-elite 0).  Exceptions, each
asserted narrowly:
  * mmd_opt: a candidate whose beta-CEM parted from the oracle's at the one
    near-tie that can explain it (tests/parity.py: beta_divergence) may have
    other costs; it must not change an elite set;
  * beta noise: rejection-sampled Beta draws may differ in ulps, which may
    move the costs of at most B / 20 candidates per iteration (never an
    elite set).
"""
import numpy as np
import pytest

import oracle
from oracle.helper import compute_obs_trajectories
from parity import DEFAULT_COV, DEFAULT_INIT, DEFAULT_MEAN, beta_cem_trace, beta_near_tie, close

pytestmark = pytest.mark.gpu

B, H, O, T = 32, 20, 3, 20


def blocking_scenario(prob):
    """Obstacles inside the 3 s horizon (the ego starts at x = 0, y = 1.75,
    at 5 m/s): one grazing the ego lane from the left, one on it, one on the
    other lane -- a share of every candidate's noisy rollouts collides at
    first, and the CEM has to find the gap."""
    x = np.array([13.0, 24.0, 18.0])
    y = np.array([4.4, 1.75, -1.75])
    z = np.zeros(O)
    xo, yo, _ = compute_obs_trajectories(prob, x, y, z, z, z)
    return xo, yo


def _per_candidate(nat, tr, cost, n):
    """(obstacle / lane costs agree, beta-CEM outputs agree) per candidate."""
    obs_g, lane_g = nat.read("obs_cost")[:B], nat.read("lane_cost")[:B]
    fl = 1e-2 if cost.startswith("mmd") else 1e-5
    ok = np.abs(obs_g - tr["obs"]) <= fl + 1e-4 * np.abs(tr["obs"])
    ok &= np.abs(lane_g - tr["lane"]) <= fl + 1e-4 * np.abs(tr["lane"])
    inner = np.ones(B, bool)
    if cost == "mmd_opt":
        res_g = nat.read("res_beta").reshape(B, 20)
        inner &= np.all(np.abs(res_g - tr["res_beta"]) <= 1e-4 * np.abs(tr["res_beta"]) + 1e-6, axis=1)
        inner &= np.abs(nat.read("sigma")[:B] - tr["sigma"]) <= 1e-6 * np.abs(tr["sigma"])
        beta_g = nat.read("beta").reshape(B, n)
        inner &= np.all(np.abs(beta_g - tr["beta"]) <= 1e-3 * np.abs(tr["beta"]) + 1e-4, axis=1)
    return ok, inner


@pytest.mark.parametrize("cost,noise,n", [("mmd_opt", "gaussian", 6), ("cvar", "gaussian", 24),
                                          ("saa", "gaussian", 24), ("mmd_random", "gaussian", 24),
                                          ("cvar", "beta", 24)])
def test_free_run(native, cost, noise, n):
    level = 0.1 if noise == "gaussian" else 0.3
    ora = oracle.CEM(n, O, level, H, noise, 0.0, 0.0, num_batch=B, maxiter_cem=T)
    nat = native.Handle(native.make_config(n, O, level, H, noise, 0.0, 0.0, num_batch=B, maxiter_cem=T))
    xo, yo = blocking_scenario(ora.prob)
    idx = 17
    # injected normals; Beta draws (beta noise) come from the same Philox streams on both sides
    draws = oracle.Draws.random(ora.prob, np.random.default_rng(21), idx_mpc=idx, with_beta_cem=(cost == "mmd_opt"))
    trace = []
    ref = ora.solve(cost, idx, DEFAULT_INIT, DEFAULT_MEAN, DEFAULT_COV, xo, yo, 15.0, draws=draws, trace=trace)
    nat.begin(cost, idx, DEFAULT_INIT, DEFAULT_MEAN, DEFAULT_COV, xo, yo, 15.0, draws)
    assert float(np.max(trace[0]["obs"])) > float(np.min(trace[0]["obs"])), "scenario does not separate candidates"
    parted, moved = {}, {}
    for t in range(T):
        nat.iterate(t, 1)
        nat.sync()
        tr = trace[t]
        ok, inner = _per_candidate(nat, tr, cost, n)
        if cost == "mmd_opt" and not inner.all():
            # a candidate's beta-CEM parted from the oracle's: only at the near-tie that explains it
            acc, steer = nat.read("acc").reshape(B, 100), nat.read("steer").reshape(B, 100)
            st = ora.init_state(DEFAULT_INIT, DEFAULT_MEAN, DEFAULT_COV, draws)
            res_g = nat.read("res_beta").reshape(B, 20)
            esum_g = nat.read("btrace").reshape(B, 20)
            for b in np.nonzero(~inner)[0]:
                _, tie, detail = beta_near_tie(beta_cem_trace(ora, st, acc[b], steer[b], draws, t), res_g[b], esum_g[b])
                assert tie, f"iteration {t} candidate {b}: beta-CEM differs without a qualifying near-tie ({detail})"
                parted[(t, int(b))] = detail
        if not ok.all():
            bad = np.nonzero(~ok)[0]
            if cost == "mmd_opt":  # a cost moves only through its beta-CEM parting (explained above)
                assert all((t, int(b)) in parted for b in bad), f"iteration {t}: costs of {bad} differ, beta-CEM equal"
            elif noise == "beta":
                # rejection-sampled Beta draws: ulp-level differences may move a sample's cost
                assert bad.size <= max(1, B // 20), f"iteration {t}: {bad.size} candidates differ"
                moved[t] = bad.tolist()
            else:
                raise AssertionError(f"iteration {t}: candidates {bad} differ: GPU "
                                     f"{nat.read('obs_cost')[:B][bad]} oracle {tr['obs'][bad]}")
        tp = nat.read("tr_proj", np.int32).reshape(T, B)[t]
        to = nat.read("tr_obs", np.int32).reshape(T, 20)[t]
        tc = nat.read("tr_cem", np.int32).reshape(T, 5)[t]
        # lockstep to the end: the elite sets must be identical every iteration
        assert np.array_equal(tp, tr["perm"]), f"iteration {t}: projection order differs"
        assert np.array_equal(to, tr["elite_obs"]), f"iteration {t}: obstacle elites {to} vs {tr['elite_obs']}"
        assert np.array_equal(tc, tr["elite_cem"]), f"iteration {t}: cost elites {tc} vs {tr['elite_cem']}"
    got = nat.finish(trace=True)
    close("cx", got["cx"], ref[0], rtol=1e-4, atol=1e-4)
    close("cy", got["cy"], ref[1], rtol=1e-4, atol=1e-4)
    e0 = int(got["elite_obs"][T - 1][0])
    if (T - 1, e0) not in parted and e0 not in moved.get(T - 1, []):
        fl = 1e-2 if cost.startswith("mmd") else 1e-5
        close("cost_lane", got["cost_lane"], ref[2], rtol=1e-4, atol=fl)
        close("cost_obs", got["cost_obs"], ref[3], rtol=1e-4, atol=fl)
        if cost == "mmd_opt":
            close("beta", got["beta"][:n], ref[4], rtol=1e-3, atol=1e-4)
            close("sigma", got["sigma"], ref[5], rtol=1e-6, atol=0)
            close("res_beta", got["res_beta"], ref[6], rtol=1e-4, atol=1e-6)
    print(f"{cost}/{noise}: 20 iterations in lockstep; cost_obs {float(got['cost_obs'])}; "
          f"explained beta-CEM partings {parted}; Beta-draw cost moves {moved}")


@pytest.mark.parametrize("cost,noise,n", [("cvar", "beta", 24), ("mmd_opt", "gaussian", 6)])
def test_iteration_graphs(native, cost, noise, n):
    """Single-iteration graph replay (mpcmmd_set_graphs, then iterate(t, 1):
    all T iterations captured at the first call) gives the bits of direct
    launches, and again when the captured graphs are reused by a new solve."""
    from parity import make_pair
    Tg = 6
    ora, nat, xo, yo = make_pair(native, cost, noise, n=n, O=O, H=10, B=B, T=Tg)

    def run(graphs):
        nat.set_graphs(graphs)
        nat.begin(cost, 3, DEFAULT_INIT, DEFAULT_MEAN, DEFAULT_COV, xo, yo, 15.0)
        for t in range(Tg):
            nat.iterate(t, 1)
        return nat.finish()

    ref = run(False)
    for rep in range(2):
        got = run(True)
        for k, v in ref.items():
            if isinstance(v, np.ndarray):
                assert np.array_equal(got[k], v, equal_nan=True), f"{k} differs with graphs (run {rep})"
            else:
                assert got[k] == v or (v != v and got[k] != got[k]), f"{k} differs with graphs (run {rep})"


@pytest.mark.parametrize("n", [6, 17])
def test_iteration_graphs_out_of_order_first(native, n):
    """A fresh handle whose first call is iterate(1, 1): with single-iteration
    graphs every iteration is captured at that call, so work the handle does
    once (the +inf pad columns of the distance matrix, k_dist_pad) must not
    be recorded into one iteration's graph -- replaying another iteration
    first would then sum exp(-0) = 1 per pad column into every direct row
    sum.  n = 6 (M = 36, 220 pad columns) runs the fused k_bcem_small, n = 17
    (M = 289, 223 pad columns) the per-iteration kernels.  Graph replay must
    give the bits of direct launches after each of iterate(1, 1),
    iterate(0, 1), iterate(1, 1), and every pad column must hold +inf."""
    from parity import make_pair
    M, Md = n * n, (n * n + 255) & ~255
    nats = []
    for graphs in (False, True):
        ora, nat, xo, yo = make_pair(native, "mmd_opt", "gaussian", n=n, O=O, H=10, B=B, T=3)
        nat.set_graphs(graphs)
        nat.begin("mmd_opt", 3, DEFAULT_INIT, DEFAULT_MEAN, DEFAULT_COV, xo, yo, 15.0)
        nats.append(nat)
    for step, t in enumerate((1, 0, 1)):
        for nat in nats:
            nat.iterate(t, 1)
            nat.sync()
        assert np.all(np.isfinite(nats[0].read("brow"))), f"call {step}: row sums of the direct launches not finite"
        for k in ("brow", "res_beta", "obs_cost", "lane_cost", "pop"):
            a, b = nats[0].read(k), nats[1].read(k)
            ne = np.flatnonzero((a != b) & ~(np.isnan(a) & np.isnan(b)))
            assert ne.size == 0, (f"call {step} (iterate({t}, 1)): {k} differs with graphs in {ne.size} elements; first "
                                  f"at {ne[0]}: {a[ne[0]]} (direct launches) vs {b[ne[0]]} (graphs)")
        for nat, what in zip(nats, ("direct launches", "graphs")):
            pad = nat.read("bdist", np.float32, (B, M, Md))[:, :, M:]
            assert np.all(np.isposinf(pad)), f"call {step} (iterate({t}, 1)), {what}: pad columns of bdist not +inf"
    for nat in nats:
        nat.close()


@pytest.mark.parametrize("cost,noise,n", [("cvar", "beta", 24), ("mmd_opt", "gaussian", 6)])
def test_draws_ahead(native, cost, noise, n, monkeypatch):
    """k_select of iteration t drawing iteration t + 1's noise and Beta attempt
    table (MPCMMD_AHEAD, on by default) changes no bit: in order, with an
    iteration re-run (its successor's draws come again), after a skipped
    iteration (drawn normally), with single-iteration graphs, and across a
    new solve whose key differs (begin drops the ahead draws)."""
    from parity import make_pair
    Tg = 6
    order = [0, 1, 1, 2, 4, 5, 3]

    def run(ahead, graphs, idx):
        monkeypatch.setenv("MPCMMD_AHEAD", "1" if ahead else "0")
        ora, nat, xo, yo = make_pair(native, cost, noise, n=n, O=O, H=10, B=B, T=Tg)
        nat.set_graphs(graphs)
        outs = []
        for k in idx:
            nat.begin(cost, k, DEFAULT_INIT, DEFAULT_MEAN, DEFAULT_COV, xo, yo, 15.0)
            for t in order:
                nat.iterate(t, 1)
                outs.append((nat.read("pop").copy(), nat.read("obs_cost").copy()))
            outs.append(nat.finish())
        nat.close()
        return outs

    ref = run(False, False, [3, 7])
    for ahead, graphs in [(True, False), (True, True)]:
        got = run(ahead, graphs, [3, 7])
        for i, (g, r) in enumerate(zip(got, ref)):
            if isinstance(r, tuple):
                assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(g, r)), \
                    f"step {i} differs (ahead={ahead}, graphs={graphs})"
            else:
                for k, v in r.items():
                    if isinstance(v, np.ndarray):
                        assert np.array_equal(g[k], v, equal_nan=True), f"{k} differs (ahead={ahead}, graphs={graphs})"
