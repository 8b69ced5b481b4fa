"""mpcmmd_validate_carla_risk without a GPU: the symbol, the argument checks
that return before any HIP call, the expected-value helper (carla_risk_ref.py)
against carla_validation_ref's counts on the shared fixture, and the replay
driver's risk accounting with fake solver, validator and risk function."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import carla_risk_ref as rref
import carla_validation_ref as vref
import risk_stats_ref as sref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CARLA = os.path.join(ROOT, "mpc-mmd_amd", "carla")
F32 = np.float32
INVALID, UNSUPPORTED = -1, -3


@pytest.fixture(scope="module")
def nat():
    from optimizer import _native
    _native.lib()
    return _native


def test_abi_and_symbol(nat):
    L = nat.lib()
    assert nat.ABI_VERSION == 5 and L.mpcmmd_abi_version() == 5
    assert "mpcmmd_validate_carla_risk" in nat.SYMBOLS and hasattr(L, "mpcmmd_validate_carla_risk")


def _args(nat, K_=1, O=3, H=60, R=8, P=600, S=2, noise=0, variant=2, alpha=0.98, sigma=None):
    """Arguments with valid (zero) arrays: only the checked scalars vary."""
    k1, s1 = max(K_, 1), max(min(S, 8), 1)
    keep = dict(st=np.zeros((k1, 6), F32), v=np.zeros((k1, 100), F32), xo=np.zeros((k1, max(O, 1), 100), F32),
                pa=np.zeros((k1, 6, max(P, 1)), F32), ks=np.zeros(k1, np.uint32),
                sg=np.full((k1, s1), 0.5, F32) if sigma is None else sigma, cnt=np.zeros((k1, 3), np.int32),
                out=np.zeros((4, k1, 3), F32), mmd=np.zeros((k1, 3, s1), F32))
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    a = nat.ValidateCarlaRiskArgs(K_, O, H, R, P, noise, variant, 0.1, 0.0, 0.0, 0, 0, fp(keep["st"]), fp(keep["v"]),
                                  fp(keep["v"]), fp(keep["xo"]), fp(keep["xo"]), fp(keep["pa"]), None, None,
                                  keep["ks"].ctypes.data_as(C.POINTER(C.c_uint32)), alpha, S, fp(keep["sg"]),
                                  keep["cnt"].ctypes.data_as(C.POINTER(C.c_int32)), fp(keep["out"][0]),
                                  fp(keep["out"][1]), fp(keep["out"][2]), fp(keep["out"][3]), fp(keep["mmd"]),
                                  None, None, None, None, None, None)
    return a, keep


BAD = [dict(S=9), dict(S=-1), dict(alpha=1.5), dict(alpha=-0.01), dict(alpha=float("nan")),
       dict(sigma=np.array([[0.5, 0.0]], F32)), dict(sigma=np.array([[-1.0, 0.5]], F32)),
       dict(sigma=np.array([[0.5, np.inf]], F32)), dict(sigma=np.array([[np.nan, 0.5]], F32)),
       dict(R=(1 << 20) + 1), dict(R=0), dict(O=33), dict(O=0), dict(P=3), dict(P=2049), dict(H=1), dict(H=101),
       dict(K_=-1), dict(K_=65536), dict(noise=2), dict(variant=0), dict(variant=1), dict(variant=4)]


@pytest.mark.parametrize("bad", BAD, ids=lambda b: "-".join(b))
def test_invalid_arguments_need_no_gpu(nat, bad):
    """Every limit of include/mpcmmd.h and a static / dynamic variant: MPCMMD_E_INVALID with a message."""
    a, keep = _args(nat, **bad)
    assert nat.lib().mpcmmd_validate_carla_risk(C.byref(a)) == INVALID, bad
    assert nat.lib().mpcmmd_last_error()


@pytest.mark.parametrize("field", ["init_state", "v", "steer", "x_obs", "y_obs", "path", "keys", "count_pos", "var",
                                   "cvar", "mean", "max", "sigma", "mmd"])
def test_null_arguments(nat, field):
    a, keep = _args(nat)
    setattr(a, field, None)
    assert nat.lib().mpcmmd_validate_carla_risk(C.byref(a)) == INVALID, field


def test_no_configuration_is_ok_without_gpu(nat):
    a, keep = _args(nat, K_=0)
    assert nat.lib().mpcmmd_validate_carla_risk(C.byref(a)) == 0
    assert nat.lib().mpcmmd_validate_carla_risk(None) == INVALID
    out = nat.validate_carla_risk(np.zeros((0, 6)), np.zeros((0, 100)), np.zeros((0, 100)), None, None, [], [], 60,
                                  "gaussian", 0.1, sigma=[0.5], counts=True, return_costs=True)
    assert out["count_pos"].shape == (0, 3) and out["mmd"].shape == (0, 3, 1) and out["mmd_lane"].shape == (0, 1)
    assert out["count_oh"].shape[0] == 0 and out["costs"].shape == (0, 3, 1000)


def test_missing_symbol_raises_native_error(nat, monkeypatch):
    class Old:
        pass
    monkeypatch.setattr(nat, "lib", lambda: Old())
    with pytest.raises(nat.NativeError, match="mpcmmd_validate_carla_risk"):
        nat.validate_carla_risk(np.zeros((1, 6)), np.zeros((1, 100)), np.zeros((1, 100)), np.zeros((1, 1, 100)),
                                np.zeros((1, 1, 100)), np.zeros((1, 6, 4), F32), [0], 60, "gaussian", 0.1)


# ---------------------------------------------------------------- the helper
@pytest.fixture(scope="module")
def fix():
    return rref.fixture_refs()


def test_fixture_table_and_counts(fix):
    """carla_risk_ref's channels against carla_validation_ref's counts, and the numbers of the fixture's table."""
    plans, draws, eps, refs = fix
    assert draws.shape == (3, 3, rref.FIX_R, rref.FIX_H) and np.array_equal(draws[0], draws[2])
    for i, r in enumerate(refs):
        c = rref.channels(r)
        assert c.shape == (3, rref.FIX_R) and c.dtype == F32 and not np.isnan(c).any()
        st = sref.stats(c, 0.98, (0.01, 0.3))
        assert tuple(st["count_pos"]) == rref.FIX_COUNT_POS[i]
        assert np.allclose(st["var"], rref.FIX_VAR[i], rtol=0, atol=5e-5), st["var"]
        assert int((c[0] > 0).sum()) == r["count_rows"]
        assert r["count"] <= st["count_pos"][0] and r["count_lane"] <= st["count_pos"][1] + st["count_pos"][2]
        # not degenerate: no decisive margin and no collision margin within TOL of zero
        assert not (np.abs(rref.decisive(r)) <= rref.TOL).any() and vref.near_share(r) == 0.0
        assert rref.check_costs(r, c, f"self {i}") == 1.0
    assert (refs[0]["count"], refs[0]["count_rows"]) == (222, 223)
    assert refs[1]["count_lane"] == 12 < 13
    st = sref.stats(rref.channels(refs[2]), 0.98, (0.01, 0.3))
    assert st["var"][2] == 0 and st["count_pos"][2] == 1 and abs(st["cvar"][2] - 1.04e-3) < 1e-5
    assert np.all(st["mmd"][:2] == F32(-1000.0))


def test_channels_propagate_nan_and_reject_wrong_costs(fix):
    plans, draws, eps, refs = fix
    r = dict(refs[1])
    r["m"] = r["m"].copy()
    r["m"][0, :, 1] = np.nan
    c = rref.channels(r)
    assert np.isnan(c[0]).all() and np.array_equal(c[1:], rref.channels(refs[1])[1:])
    assert sref.stats(c)["count_pos"][0] == rref.FIX_R
    good = rref.channels(refs[0])
    bad = good.copy()
    bad[0, np.argmax(good[0] > 0)] = 0.0           # a positive cost reported as zero
    with pytest.raises(AssertionError):
        rref.check_costs(refs[0], bad, "bad")
    with pytest.raises(AssertionError):
        rref.check_costs(refs[0], good + F32(3e-4), "shifted")


# ------------------------------------------------------------ replay driver
def _driver():
    spec = importlib.util.spec_from_file_location("mpcmmd_carla_validate_replay_r",
                                                  os.path.join(CARLA, "validate_replay.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_replay_driver_risk_accounting(tmp_path):
    D = _driver()
    rec = dict(ego=np.zeros((10, 6), F32))

    def inputs(rec_, prob, k):
        return np.full(6, k, F32), np.zeros((2, 100), F32), np.zeros((2, 100), F32), dict(tick=k)

    def solve(prob, cost, k, init, mean, cov, xo, yo, v_des, path):
        return None, None, np.full(100, k, F32), np.full(100, -k, F32), np.asarray(mean, F32) + F32(1)

    vcalls, rcalls = [], []

    def counts_of(plans):
        t = np.array([p["tick"] for p in plans])
        rows = np.where(t % 2 == 0, t, 0)
        return dict(count=rows // 2, count_rows=rows, count_lane=t + 100)

    def validate(prob, plans, num_rollouts, seed):
        vcalls.append([p["tick"] for p in plans])
        return counts_of(plans)

    def risk_fn(prob, plans, num_rollouts, seed, alpha, sigma):
        rcalls.append(([p["tick"] for p in plans], num_rollouts, seed, alpha, tuple(sigma)))
        n = len(plans)
        base = np.arange(n * 3, dtype=F32).reshape(n, 3)
        out = counts_of(plans)
        out.update(count_pos=np.stack([out["count_rows"], np.zeros(n, int), np.ones(n, int)], 1).astype(np.int32),
                   mmd=np.stack([base, base + 100], axis=-1))
        out.update({k: base + i for i, k in enumerate(("var", "cvar", "mean", "max"))})
        return out

    today = ["count", "count_lane", "count_rows", "num_rollouts", "tick"]
    kw = dict(costs=("cvar", "det"), ticks=range(3, 7), num_rollouts=8, seed=5, solve=solve, validate=validate,
              inputs=inputs)
    plain_lines, lines = [], []
    plain = D.validate_replay(rec, object(), out_dir=str(tmp_path / "plain"), log=plain_lines.append,
                              risk_fn=risk_fn, **kw)
    assert not rcalls and len(vcalls) == 2 and len(plain_lines) == 2
    res = D.validate_replay(rec, object(), out_dir=str(tmp_path / "risk"), log=lines.append, risk=True,
                            risk_sigma=(0.01, 0.3), risk_alpha=0.9, risk_fn=risk_fn, **kw)
    assert len(vcalls) == 2, "with risk the counts come from the risk call"
    assert [c[0] for c in rcalls] == [[3, 4, 5, 6]] * 2, "one risk call per cost with every tick"
    assert all(c[1:4] == (8, 5, 0.9) and np.allclose(c[4], (0.01, 0.3)) for c in rcalls)
    extra = ["risk_alpha", "risk_count_pos", "risk_cvar", "risk_max", "risk_mean", "risk_mmd", "risk_sigma",
             "risk_var"]
    for cost in ("cvar", "det"):
        with np.load(tmp_path / "plain" / f"validate_{cost}.npz") as z:
            assert sorted(z.files) == today and sorted(plain[cost]) == today
            base = {k: z[k] for k in z.files}
        with np.load(tmp_path / "risk" / f"validate_{cost}.npz") as z:
            assert sorted(z.files) == sorted(today + extra)
            assert all(np.array_equal(z[k], base[k]) for k in today)
            assert all(np.array_equal(z[k], res[cost][k]) for k in z.files)
            assert z["risk_count_pos"].dtype == np.int32 and z["risk_count_pos"].shape == (4, 3)
            assert np.array_equal(z["risk_count_pos"][:, 0], z["count_rows"])
            assert z["risk_mmd"].shape == (4, 3, 2) and z["risk_cvar"].dtype == F32
            assert np.array_equal(z["risk_cvar"], np.arange(12, dtype=F32).reshape(4, 3) + 1)
            assert np.array_equal(z["risk_sigma"], np.array([0.01, 0.3], F32)) and z["risk_alpha"] == F32(0.9)
    # per cost: today's line, then the risk line (mean obstacle CVaR = mean(1, 4, 7, 10), SAA = (4 + 6) / 8 / 4)
    assert len(lines) == 4 and lines[0] == plain_lines[0] and lines[2] == plain_lines[1]
    assert lines[1].startswith("cvar: risk") and lines[3].startswith("det: risk")
    assert "5.500000" in lines[1] and "0.312500" in lines[1]
