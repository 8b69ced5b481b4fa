"""mpcmmd_validate_risk on the GPU against the oracle (risk_stats_ref.py):
the statistics kernels exactly on injected samples, the MMD within the
exp2-term bound, the whole pipeline on injected draws, and the internal Philox
streams against mpcmmd_validate's counts."""
import numpy as np
import pytest

import risk_stats_ref as ref
from oracle import costs as Cst
from oracle import validation as V
from oracle.problem import Problem

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
ALPHA = 0.98
STAT_R = (1, 2, 22, 257, 1025, 4099)
MMD_R = (1, 257, 1025, 2500)
SIGMA = (0.01, 1.0, 12.0)
# mmd: 2e-6 per exp2 term on q1 <= 1 and 2 q2 <= 2 gives 6e-3
# of ker_wt = 1000; the oracle's fp32 1 / R adds <= 2e-4
MMD_ATOL = 1e-2


def _same(a, b):
    """== (so -0 and +0 agree), or NaN on both sides."""
    a, b = np.asarray(a), np.asarray(b)
    return (a == b) | (np.isnan(a) & np.isnan(b))


def _same_bits(a, b):
    """The same fp32 bit pattern, or NaN on both sides."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


# ------------------------------------------------- 1. statistics on injected samples
@pytest.fixture(scope="module")
def stat_cases():
    """Per R: pattern names, samples [N][R] and the oracle's statistics, once."""
    out = {}
    for R in STAT_R:
        pat = ref.patterns(R, np.random.default_rng(R), ALPHA)
        names = sorted(pat)
        c = np.stack([pat[n] for n in names])
        out[R] = (names, c, ref.stats(c, ALPHA))
    return out


def _inject(native, c, **kw):
    """Samples [N][R] as N / 3 (padded) configurations of three channels."""
    N, R = c.shape
    K = -(-N // 3)
    cin = np.zeros((K * 3, R), F32)
    cin[:N] = c
    got = native.validate_risk(costs_in=cin.reshape(K, 3, R), alpha=ALPHA, **kw)
    return {k: v.reshape((K * 3,) + v.shape[2:])[:N] for k, v in got.items()
            if k in ("count_pos", "var", "cvar", "mean", "max", "mmd", "saa")}


@pytest.mark.parametrize("R", STAT_R)
def test_statistics_exact_on_injected_samples(native, stat_cases, R):
    names, c, exp = stat_cases[R]
    got = _inject(native, c)
    for i, n in enumerate(names):
        for k in ("var", "max", "count_pos"):
            assert _same(got[k][i], exp[k][i]), (R, n, k, got[k][i], exp[k][i])
        for k in ("cvar", "mean"):   # an fp64 sum of fp32 values in another order: 1 fp32 ulp
            assert ref.ulp_close(got[k][i], exp[k][i]), (R, n, k, got[k][i], exp[k][i])
    if R >= 257:   # the patterns are what they claim
        i = names.index("one_percent")
        assert exp["var"][i] == 0 and exp["count_pos"][i] > 0
        assert exp["var"][names.index("five_percent")] > 0
        assert np.isnan(exp["max"][names.index("three_nan")]) and np.isinf(exp["max"][names.index("inf_top")])
        lo, hi = ref.position(R, ALPHA)
        s = np.sort(c[names.index("tie_block")])
        assert s[max(lo - 1, 0)] == s[lo] == s[hi] == s[min(hi + 1, R - 1)]
        s = np.sort(c[names.index("one_ulp")])
        assert hi == lo or s[hi] == np.nextafter(s[lo], F32(np.inf))


def test_var_and_cvar_at_n_are_the_cvar_reducers(native, stat_cases):
    """At R = n = 22 the estimator is the optimizer's: bit-equal to oracle.costs.cvar."""
    from types import SimpleNamespace
    names, c, _ = stat_cases[22]
    got = _inject(native, c)
    want_cvar = Cst.cvar(SimpleNamespace(alpha_quant=ALPHA), c)
    want_var = Cst.quantile_linear(c, ALPHA)
    assert np.all(_same_bits(got["var"], want_var)), (names, got["var"], want_var)
    assert np.all(_same_bits(got["cvar"], want_cvar)), (names, got["cvar"], want_cvar)


def test_batched_configurations_equal_each_alone(native, stat_cases):
    names, c, _ = stat_cases[1025]
    K = 7
    cin = np.stack([c[(3 * k + np.arange(3)) % len(names)] for k in range(K)])
    cin[3] = 0.0
    sig = np.tile(np.array([[0.01, 1.0]], F32), (K, 1)) * (1.0 + np.arange(K, dtype=F32))[:, None]
    both = native.validate_risk(costs_in=cin, alpha=ALPHA, sigma=sig)
    for k in range(K):
        one = native.validate_risk(costs_in=cin[k:k + 1], alpha=ALPHA, sigma=sig[k:k + 1])
        for key in ("count_pos", "var", "cvar", "mean", "max", "mmd"):
            a, b = both[key][k], one[key][0]
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) if a.dtype == F32 else np.array_equal(a, b), \
                (k, key, a, b)


# ------------------------------------------------------------------------- 2. MMD
@pytest.fixture(scope="module")
def mmd_cases():
    out = {}
    for R in MMD_R:
        pat = ref.mmd_patterns(R, np.random.default_rng(1000 + R))
        if R == 2500:   # dense: all non-zero, three tiles, the last ragged; sparse / signed: fewer tiles than
            del pat["all_zero"]   # the launch has, so the workgroups at or beyond P exit
        names = sorted(pat)
        c = np.stack([pat[n] for n in names])
        out[R] = (names, c, ref.stats(c, ALPHA, SIGMA)["mmd"])
    return out


@pytest.mark.parametrize("R", MMD_R)
def test_mmd_against_oracle(native, mmd_cases, R):
    names, c, exp = mmd_cases[R]
    assert any((c[i] < 0).any() for i in range(len(names)))
    if R == 2500:
        nz = {n: int((c[i] != 0).sum()) for i, n in enumerate(names)}
        assert nz["dense"] == R and 0 < nz["sparse"] <= 1024 < nz["signed"] <= 2048, nz
    got = _inject(native, c, sigma=SIGMA)
    again = _inject(native, c, sigma=SIGMA)
    assert got["mmd"].shape == exp.shape == (len(names), len(SIGMA))
    for i, n in enumerate(names):
        err = np.abs(got["mmd"][i].astype(F64) - exp[i].astype(F64))
        print(f"mmd R={R} {n}: got {got['mmd'][i]} oracle {exp[i]} err {err}")
        assert np.all(err <= MMD_ATOL), (R, n, got["mmd"][i], exp[i])
    if "all_zero" in names:
        assert np.all(got["mmd"][names.index("all_zero")] == F32(-1000.0))
    assert np.array_equal(got["mmd"].view(np.uint32), again["mmd"].view(np.uint32)), "two calls, other bits"


# ------------------------------------------------------- 3. pipeline, injected draws
H, O = 20, 2
OBS_Y = (-1.0, -1.06, -1.12, -1.14, -1.16, -1.18, -1.2, -1.3)
OBS_POS_1000 = (292, 147, 121, 180, 164, 68, 18, 0)


def _plans(R):
    """The eight plans beside obstacle 0 and a ninth that drifts across y_ub."""
    j = np.arange(11) / 10.0
    cx, cy, st, xo, yo, dr = [], [], [], [], [], []
    for k, oy in enumerate(OBS_Y):
        c = 1.75 + 0.3 * np.sin(3.0 * j + k)
        c[:3] = 1.75
        cx.append(15.0 * (5.0 * j + 3.0 * j * j)), cy.append(c)
        st.append([0.0, 1.75, 5.0, 0.0, 0.0, 0.0])
        xo.append(np.stack([np.full(100, 14.0, F32), np.full(100, 500.0, F32)]))
        yo.append(np.stack([np.full(100, oy, F32), np.full(100, -1.75, F32)]))
        dr.append(np.random.RandomState(100 + k).standard_normal((3, R, H)))
    c = 2.1 + 0.3 * np.sin(3.0 * j)
    c[:3] = 2.1
    cx.append(15.0 * (5.0 * j + 3.0 * j * j)), cy.append(c)
    st.append([0.0, 2.1, 5.0, 0.0, 0.0, 0.0])
    xo.append(np.stack([np.full(100, 500.0, F32), np.full(100, 600.0, F32)]))
    yo.append(np.stack([np.full(100, -1.75, F32), np.full(100, -1.75, F32)]))
    dr.append(np.random.RandomState(7).standard_normal((3, R, H)))
    return tuple(np.array(a) for a in (cx, cy, st, xo, yo, dr))


@pytest.fixture(scope="module")
def pipeline_cases():
    prob = Problem(10, O, 0.1, H, "gaussian", 0.05, 0.01)
    out = {}
    for R in (257, 1000):
        cx, cy, st, xo, yo, dr = _plans(R)
        c = np.stack([ref.rollout_channels(prob, cx[k], cy[k], st[k], xo[k], yo[k], "gaussian", 0.1, 0.05, 0.01,
                                           dr[k]) for k in range(len(cx))])
        out[R] = ((cx, cy, st, xo, yo, dr), c, ref.stats(c, ALPHA, (0.01, 0.3)))
    return out


@pytest.mark.parametrize("R", [257, 1000])
def test_pipeline_on_injected_draws(native, pipeline_cases, R):
    (cx, cy, st, xo, yo, dr), c, exp = pipeline_cases[R]
    K = len(cx)
    pos = exp["count_pos"]
    # the case covers: partial with VaR > 0, partial with VaR = 0, none; a lane crossing
    if R == 1000:
        assert tuple(pos[:8, 0]) == OBS_POS_1000 and pos[8, 2] == 247
        assert exp["var"][0, 0] > 0 and exp["var"][6, 0] == 0 and pos[6, 0] > 0
    else:
        assert pos[6, 0] == 1 and pos[7, 0] == 0 and pos[8, 2] == 63 and exp["var"][0, 0] > 0
    got = native.validate_risk(cx, cy, st, xo, yo, np.arange(K), H, "gaussian", 0.1, 0.05, 0.01, num_rollouts=R,
                               draws=dr, alpha=ALPHA, sigma=(0.01, 0.3), return_costs=True)
    assert got["costs"].shape == c.shape
    assert np.all(ref.ulp_close(got["costs"], c)), np.abs(got["costs"] - c).max()
    assert np.array_equal(got["costs"] == 0, c == 0)
    assert np.array_equal(got["count_pos"], pos)
    for k in ("var", "cvar", "mean", "max", "saa"):
        assert np.allclose(got[k], exp[k], rtol=1e-5, atol=1e-6), (k, got[k], exp[k])
    assert np.all(np.abs(got["mmd"].astype(F64) - exp["mmd"]) <= MMD_ATOL), (got["mmd"], exp["mmd"])
    assert np.array_equal(got["cvar_lane"], got["cvar"][:, 1] + got["cvar"][:, 2])
    assert np.array_equal(got["mmd_lane"], got["mmd"][:, 1] + got["mmd"][:, 2])


# ---------------------------------------------------------- 4. internal streams
@pytest.mark.parametrize("noise,level", [("gaussian", 0.1), ("beta", 0.3)])
def test_internal_streams(native, noise, level):
    R = 1000
    prob = Problem(10, O, level, H, noise, 0.05, 0.01)
    cx, cy, st, xo, yo, _ = _plans(1)
    sel = [0, 3, 6, 8]
    cx, cy, st, xo, yo = (a[sel] for a in (cx, cy, st, xo, yo))
    keys = np.array([11, 12, 13, 14])
    got = native.validate_risk(cx, cy, st, xo, yo, keys, H, noise, level, 0.05, 0.01, num_rollouts=R, seed=7,
                               alpha=ALPHA)
    cnt, lane = native.validate(cx, cy, st, xo, yo, keys, H, noise, level, 0.05, 0.01, num_rollouts=R, seed=7)
    for k in range(len(sel)):
        acc, steer = V.controls(prob, cx[k], cy[k])
        d = V.draws_philox(prob, acc, steer, noise, R, H, keys[k], seed=7)
        c = ref.rollout_channels(prob, cx[k], cy[k], st[k], xo[k], yo[k], noise, level, 0.05, 0.01, d)
        want = (~(c <= 0)).sum(axis=1)
        assert np.all(np.abs(got["count_pos"][k] - want) <= R // 100), (k, got["count_pos"][k], want)
        # the same rollouts as mpcmmd_validate: a per-(obstacle, step) count never exceeds the per-rollout one
        assert cnt[k] <= got["count_pos"][k, 0], (k, cnt[k], got["count_pos"][k])
        assert lane[k] <= got["count_pos"][k, 1] + got["count_pos"][k, 2], (k, lane[k], got["count_pos"][k])
    assert got["count_pos"][:, 0].max() > 0 and got["count_pos"][:, 1:].max() > 0
