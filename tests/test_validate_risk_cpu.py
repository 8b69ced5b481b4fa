"""mpcmmd_validate_risk without a GPU: the symbol and the ABI version, the
argument checks that return before any HIP call, mpcmmd_quantile_position
against oracle.costs.quantile_linear's position, the expected-value helper
(risk_stats_ref.py) against an independent scalar loop, and the validation
script's risk_* keys with a fake risk function."""
import ctypes as C
import math

import numpy as np
import pytest

import risk_stats_ref as ref
from oracle import validation as V
from oracle.problem import Problem

F32, F64 = np.float32, np.float64


@pytest.fixture(scope="module")
def nat():
    from optimizer import _native
    _native.lib()
    return _native


def test_abi_and_symbols(nat):
    L = nat.lib()
    assert nat.ABI_VERSION == 5 and L.mpcmmd_abi_version() == 5
    for s in ("mpcmmd_validate_risk", "mpcmmd_quantile_position"):
        assert s in nat.SYMBOLS and hasattr(L, s)


def _args(nat, K_=1, O=3, H=30, R=8, S=2, noise=0, variant=0, alpha=0.98, sigma=None, costs_in=False):
    """Arguments with valid (zero) arrays: only the checked scalars vary."""
    k1, o1, r1, s1 = max(K_, 1), max(O, 1), max(min(R, 64), 1), max(min(S, 8), 1)
    keep = dict(c=np.zeros((k1, 11), F64), st=np.zeros((k1, 6), F64), xo=np.zeros((k1, o1, 100), F32),
                ks=np.zeros(k1, np.uint32), sg=np.full((k1, s1), 0.5, F32) if sigma is None else sigma,
                ci=np.zeros((k1, 3, r1), F32), cnt=np.zeros((k1, 3), np.int32), out=np.zeros((4, k1, 3), F32),
                mmd=np.zeros((k1, 3, s1), F32))
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    a = nat.ValidateRiskArgs(K_, O, H, R, noise, variant, 0.1, 0.0, 0.0, 0, 0, dp(keep["c"]), dp(keep["c"]),
                             dp(keep["st"]), fp(keep["xo"]), fp(keep["xo"]), None,
                             keep["ks"].ctypes.data_as(C.POINTER(C.c_uint32)), alpha, S, fp(keep["sg"]),
                             fp(keep["ci"]) if costs_in else None,
                             keep["cnt"].ctypes.data_as(C.POINTER(C.c_int32)), fp(keep["out"][0]), fp(keep["out"][1]),
                             fp(keep["out"][2]), fp(keep["out"][3]), fp(keep["mmd"]), None, None)
    return a, keep


BAD = [dict(O=0), dict(O=33), dict(H=1), dict(H=101), dict(R=0), dict(R=(1 << 20) + 1), dict(K_=-1), dict(K_=65536),
       dict(alpha=-0.01), dict(alpha=1.01), dict(alpha=float("nan")), dict(S=-1), dict(S=9), dict(noise=2),
       dict(sigma=np.array([[0.5, 0.0]], F32)), dict(sigma=np.array([[-1.0, 0.5]], F32)),
       dict(sigma=np.array([[0.5, np.inf]], F32)), dict(sigma=np.array([[np.nan, 0.5]], F32))]


@pytest.mark.parametrize("costs_in", [False, True])
@pytest.mark.parametrize("bad", BAD, ids=lambda b: "-".join(b))
def test_invalid_arguments_need_no_gpu(nat, bad, costs_in):
    """Every limit of include/mpcmmd.h: MPCMMD_E_INVALID with a message, before any HIP call."""
    a, keep = _args(nat, costs_in=costs_in, **bad)
    assert nat.lib().mpcmmd_validate_risk(C.byref(a)) == -1, bad
    assert nat.lib().mpcmmd_last_error()


def test_no_configuration_null_and_carla(nat):
    a, keep = _args(nat, K_=0)
    assert nat.lib().mpcmmd_validate_risk(C.byref(a)) == 0
    assert nat.lib().mpcmmd_validate_risk(None) == -1
    for variant in (2, 3):
        a, keep = _args(nat, variant=variant)
        assert nat.lib().mpcmmd_validate_risk(C.byref(a)) == -3
        assert nat.lib().mpcmmd_last_error()
    a, keep = _args(nat)
    a.count_pos = None
    assert nat.lib().mpcmmd_validate_risk(C.byref(a)) == -1
    out = nat.validate_risk(np.zeros((0, 11)), np.zeros((0, 11)), np.zeros((0, 6)), None, None, [], 30, sigma=[0.5])
    assert out["count_pos"].shape == (0, 3) and out["mmd"].shape == (0, 3, 1) and out["mmd_lane"].shape == (0, 1)


def _oracle_position(n, q):
    """lo, hi, lw, hw as oracle.costs.quantile_linear forms them."""
    pos = F32(q) * F32(n - 1)
    lo, hi = np.floor(pos), np.ceil(pos)
    hw = F32(pos - lo)
    lw = F32(F32(1) - hw)
    return int(min(max(lo, 0), n - 1)), int(min(max(hi, 0), n - 1)), lw, hw


def test_quantile_position_is_the_oracles(nat):
    for alpha in (0.0, 0.5, 0.9, 0.98, 1.0):
        for n in list(range(1, 5001)) + [1 << 20]:
            lo, hi, wl, wh = nat.quantile_position(n, alpha)
            elo, ehi, elw, ehw = _oracle_position(n, alpha)
            assert (lo, hi) == (elo, ehi), (n, alpha)
            assert wl.view(np.uint32) == elw.view(np.uint32) and wh.view(np.uint32) == ehw.view(np.uint32), (n, alpha)
    # and the position is the one quantile_linear uses: distinct integers make the value name it
    from oracle.costs import quantile_linear
    for n in (1, 2, 22, 1000):
        lo, hi, wl, wh = nat.quantile_position(n, 0.98)
        x = np.arange(n, dtype=F32)[np.random.default_rng(n).permutation(n)]
        assert quantile_linear(x, 0.98) == F32(F32(lo) * wl + F32(hi) * wh)
    L = nat.lib()
    i, f = C.c_int32(), C.c_float()
    for n, alpha in ((0, 0.5), (5, -0.1), (5, 1.5), (5, float("nan"))):
        assert L.mpcmmd_quantile_position(n, alpha, C.byref(i), C.byref(i), C.byref(f), C.byref(f)) == -1


# ---------------------------------------------------------------- the helper
def _brute_costs(prob, cx, cy, st, xo, yo, draws):
    """The per-rollout costs of include/mpcmmd.h as one scalar loop (gaussian noise)."""
    acc, steer = V.controls(prob, cx, cy)
    R, H, O = draws.shape[1], prob.num_prime, xo.shape[0]
    c = np.zeros((3, R), F32)
    for r in range(R):
        x, y, vx, vy = (float(u) for u in st[:4])
        psi = math.atan2(vy, vx)
        m = [0.0, 0.0, 0.0]
        for h in range(H):
            for o in range(O):
                wc, ws = x - float(xo[o, h]), y - float(yo[o, h])
                m[0] = max(m[0], -(wc * wc) / 18.0625 - (ws * ws) / 7.5625 + 1.0)
            m[1] = max(m[1], -y + prob.y_lb)
            m[2] = max(m[2], y - prob.y_ub)
            an = acc[h] + 0.1 * abs(acc[h]) * draws[0, r, h] + 0.05 * draws[2, r, h]
            sn = steer[h] + 0.1 * abs(steer[h]) * draws[1, r, h] + 0.01 * draws[2, r, h]
            v = math.sqrt(vx * vx + vy * vy) + an * 0.15
            psi = psi + v * math.tan(sn) / 2.5 * 0.15
            vx, vy = v * math.cos(psi), v * math.sin(psi)
            x, y = x + vx * 0.15, y + vy * 0.15
        c[:, r] = m
    return c


def _brute_stats(c, alpha, sigma):
    """The statistics of include/mpcmmd.h of samples c [3][R] as scalar loops."""
    R = c.shape[1]
    out = dict(count_pos=[], var=[], cvar=[], mean=[], max=[], mmd=[])
    for ch in c:
        s = sorted(float(u) for u in ch)
        pos = F32(alpha) * F32(R - 1)
        lo, hi = int(math.floor(pos)), int(math.ceil(pos))
        hw = F32(pos - F32(lo))
        var = F32(F32(F32(s[lo]) * F32(F32(1) - hw)) + F32(F32(s[hi]) * hw))
        tail = [u for u in ch if u >= var]
        out["count_pos"].append(sum(1 for u in ch if u > 0))
        out["var"].append(var)
        out["cvar"].append(F32(math.fsum(float(u) for u in tail) / len(tail)) if tail else F32(0))
        out["mean"].append(F32(math.fsum(float(u) for u in ch) / R))
        out["max"].append(F32(s[-1]))
        mm = []
        for sg in sigma:
            q1 = sum(float(np.exp(F32(-abs(F32(a - b))) / F32(sg))) for a in ch for b in ch) / R ** 2
            q2 = sum(float(np.exp(F32(-abs(a)) / F32(sg))) for a in ch) / R
            mm.append(1000.0 * (q1 - 2.0 * q2))
        out["mmd"].append(mm)
    return out


def test_helper_against_scalar_loop():
    R, H, O = 5, 12, 2
    prob = Problem(10, O, 0.1, H, "gaussian", 0.05, 0.01)
    j = np.arange(11) / 10.0
    cx = 15.0 * (5.0 * j + 3.0 * j * j)
    cy = 2.3 + 0.3 * np.sin(3.0 * j)
    st = np.array([0.0, 2.3, 5.0, 0.0, 0.0, 0.0])
    xo = np.stack([np.full(100, 6.0, F32), np.full(100, 500.0, F32)])
    yo = np.stack([np.full(100, -0.3, F32), np.full(100, 1.75, F32)])
    draws = np.random.RandomState(3).standard_normal((3, R, H))
    sigma = (0.01, 1.0)
    c = ref.rollout_channels(prob, cx, cy, st, xo, yo, "gaussian", 0.1, 0.05, 0.01, draws)
    got = ref.stats(c, 0.98, sigma)
    cb = _brute_costs(prob, cx, cy, st, xo, yo, draws)
    assert c.shape == (3, R) and c.dtype == F32
    assert np.all(ref.ulp_close(c, cb)), (c, cb)           # vectorised vs scalar fp64 transcendentals
    assert (c[0] > 0).any() and (c[2] > 0).any() and not (c[1] > 0).any(), "a degenerate case shows nothing"
    exp = _brute_stats(c, 0.98, sigma)
    assert got["count_pos"].tolist() == exp["count_pos"]
    for k in ("var", "max"):
        assert np.array_equal(got[k], np.array(exp[k], F32)), k
    for k in ("cvar", "mean"):
        assert np.all(ref.ulp_close(got[k], np.array(exp[k], F32))), k
    assert np.allclose(got["mmd"], np.array(exp["mmd"]), rtol=0, atol=2e-3)
    assert np.array_equal(got["saa"], got["count_pos"].astype(F32) / F32(R))


# ------------------------------------------------------- the validation script
def test_validate_files_risk_keys():
    from optimizer import validation as OV
    rs = np.random.RandomState(0)
    n = 4
    d = dict(init_state=rs.rand(n, 6), x_obs=rs.rand(n, 2), y_obs=rs.rand(n, 2), vx_obs=rs.rand(n, 2),
             vy_obs=rs.rand(n, 2), cx=rs.rand(n, 11), cy=rs.rand(n, 11))
    calls = []

    def stats_fn(dd, idx, keys):
        return np.arange(len(idx)), np.arange(len(idx)) + 10

    def risk_fn(dd, idx, keys):
        K = len(idx)
        calls.append((list(idx), list(keys)))
        base = np.arange(K * 3, dtype=F32).reshape(K, 3)
        out = dict(count_pos=base.astype(np.int32), mmd=np.stack([base, base + 100], axis=-1))
        out.update({k: base + i for i, k in enumerate(("var", "cvar", "mean", "max", "saa"))})
        out["cvar_lane"] = out["cvar"][:, 1] + out["cvar"][:, 2]
        out["mmd_lane"] = out["mmd"][:, 1] + out["mmd"][:, 2]
        return out

    plain = OV.validate_files(None, d, d, "gaussian", 0.1, 30, 2, stats_fn=stats_fn)
    today = ["coll_cvar", "coll_cvar_lane", "coll_mmd_opt", "coll_mmd_opt_lane", "coll_mmd_random",
             "coll_mmd_random_lane"]
    assert sorted(plain) == today and not calls
    out = OV.validate_files(None, d, d, "gaussian", 0.1, 30, 2, stats_fn=stats_fn, risk=True,
                            risk_sigma=[0.01, 0.3], risk_fn=risk_fn)
    assert all(np.array_equal(out[k], plain[k]) for k in today)
    assert len(calls) == 2 and all(sorted(i) == [0, 1, 2, 3] and k == [0, 1, 2, 3] for i, k in calls)
    want = {f"risk_{cost}_{ch}_{st}" for cost in ("cvar", "mmd_opt") for ch in ("obs", "lane_lb", "lane_ub")
            for st in ("count_pos", "saa", "var", "cvar", "mean", "max", "mmd")}
    want |= {f"risk_{cost}_lane_{st}" for cost in ("cvar", "mmd_opt") for st in ("cvar", "mmd")} | {"risk_sigma"}
    assert set(out) == set(today) | want
    assert np.array_equal(out["risk_sigma"], np.array([0.01, 0.3], F32))
    assert out["risk_cvar_obs_var"].shape == (n,) and out["risk_mmd_opt_lane_ub_mmd"].shape == (n, 2)
    assert np.array_equal(out["risk_cvar_lane_lb_cvar"], np.arange(n * 3, dtype=F32).reshape(n, 3)[:, 1] + 1)
    assert np.array_equal(out["risk_cvar_lane_cvar"], out["risk_cvar_lane_lb_cvar"] + out["risk_cvar_lane_ub_cvar"])
