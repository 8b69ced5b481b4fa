"""mpcmmd_validate_carla without a GPU: the ABI, the argument checks that
return before any HIP call, the expected-count helper (carla_validation_ref.py)
against an independent scalar loop, and the replay driver's accounting with a
fake solver and validator."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import carla_validation_ref as ref
from oracle import carla as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CARLA = os.path.join(ROOT, "mpc-mmd_amd", "carla")
F32 = np.float32


@pytest.fixture(scope="module")
def nat():
    from optimizer import _native
    _native.lib()
    return _native


def test_abi_and_symbol(nat):
    L = nat.lib()
    assert nat.ABI_VERSION == 5 and L.mpcmmd_abi_version() == 5
    assert "mpcmmd_validate_carla" in nat.SYMBOLS and hasattr(L, "mpcmmd_validate_carla")


def _args(nat, K_=1, O=3, H=60, R=8, P=600, noise=0, variant=2):
    """Arguments with valid (zero) arrays: only the checked scalars vary."""
    keep = dict(st=np.zeros((max(K_, 1), 6), F32), v=np.zeros((max(K_, 1), 100), F32),
                xo=np.zeros((max(K_, 1), max(O, 1), 100), F32), pa=np.zeros((max(K_, 1), 6, max(P, 1)), F32),
                ks=np.zeros(max(K_, 1), np.uint32), out=np.zeros((3, max(K_, 1)), np.int32))
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    a = nat.ValidateCarlaArgs(K_, O, H, R, P, noise, variant, 0.1, 0.0, 0.0, 0, 0, fp(keep["st"]), fp(keep["v"]),
                              fp(keep["v"]), fp(keep["xo"]), fp(keep["xo"]), fp(keep["pa"]), None, None,
                              keep["ks"].ctypes.data_as(C.POINTER(C.c_uint32)), ip(keep["out"][0]),
                              ip(keep["out"][1]), ip(keep["out"][2]), None, None)
    return a, keep


@pytest.mark.parametrize("bad", [dict(O=0), dict(O=33), dict(H=1), dict(H=101), dict(P=3), dict(P=2049), dict(R=0),
                                 dict(K_=-1), dict(noise=2), dict(variant=0), dict(variant=1), dict(variant=4)])
def test_invalid_arguments_need_no_gpu(nat, bad):
    """Every shape limit and a non-CARLA variant: MPCMMD_E_INVALID before any HIP call."""
    a, keep = _args(nat, **bad)
    assert nat.lib().mpcmmd_validate_carla(C.byref(a)) == -1, bad
    assert nat.lib().mpcmmd_last_error()


def test_no_configuration_is_ok_without_gpu(nat):
    a, keep = _args(nat, K_=0)
    assert nat.lib().mpcmmd_validate_carla(C.byref(a)) == 0
    out = nat.validate_carla(np.zeros((0, 6)), np.zeros((0, 100)), np.zeros((0, 100)), None, None, [], [], 60,
                             "gaussian", 0.1)
    assert all(out[k].shape == (0,) for k in ("count", "count_lane", "count_rows"))
    assert nat.lib().mpcmmd_validate_carla(None) == -1


def test_validate_names_the_carla_entry_point(nat):
    """mpcmmd_validate on a CARLA variant points at mpcmmd_validate_carla."""
    z = np.zeros((1, 11))
    with pytest.raises(nat.NativeError, match="mpcmmd_validate_carla"):
        nat.validate(z, z, np.zeros((1, 6)), np.zeros((1, 2, 100)), np.zeros((1, 2, 100)), [0], 10, "gaussian", 0.1,
                     variant="carla_town05")


# ---------------------------------------------------------------- the helper
def _interp1(x, xp, fp):
    """jnp.interp of one value, scalar fp32 (oracle/carla.py: interp)."""
    P = len(xp)
    i = int(np.clip(np.searchsorted(xp, x, side="right"), 1, P - 1))
    dx, df, dl = F32(xp[i] - xp[i - 1]), F32(fp[i] - fp[i - 1]), F32(x - xp[i - 1])
    f = fp[i - 1] if abs(dx) <= np.spacing(np.finfo(F32).eps) else F32(fp[i - 1] + F32(F32(dl / dx) * df))
    if x < xp[0]:
        f = fp[0]
    if x > xp[-1]:
        f = fp[-1]
    return F32(f)


def _brute(p, init, v, steer, xo, yo, path, draws, eps):
    """The semantics of include/mpcmmd.h as one scalar loop per (row, step, obstacle)."""
    Hn, R, O = p.num_prime, draws.shape[1], xo.shape[0]
    cr = lambda fn, *a: F32(fn(*(np.float64(F32(u)) for u in a)))
    t, wb = F32(0.15), F32(2.875)
    oh = np.zeros((O, Hn), np.int64)
    rows_hit = 0
    nlb, nub = np.zeros(Hn, np.int64), np.zeros(Hn, np.int64)
    xp, yp, arc, Fxd, Fyd = (np.asarray(path[k], F32) for k in ("x_path", "y_path", "arc_vec", "Fx_dot", "Fy_dot"))
    for r in range(R):
        x = F32(F32(init[0]) + F32(F32(eps[r, 0] * F32(0.05)) + F32(0.3)))
        y = F32(F32(init[1]) + F32(F32(eps[r, 1] * F32(0.1)) + F32(0.0)))
        vx = F32(F32(init[2]) * cr(np.cos, init[4]))
        vy = F32(F32(init[2]) * cr(np.sin, init[4]))
        psi = cr(np.arctan2, vy, vx)
        any_hit = False
        for h in range(Hn):
            d2 = [F32(np.sqrt(F32(F32((xp[j] - x) * (xp[j] - x)) + F32((yp[j] - y) * (yp[j] - y)))))
                  for j in range(len(xp))]
            j = int(np.argmin(d2))
            s = arc[j]
            Fx, Fy = _interp1(s, arc, Fxd), _interp1(s, arc, Fyd)
            nx, ny = F32(-Fy), Fx
            nrm = F32(np.sqrt(F32(F32(nx * nx) + F32(ny * ny))))
            d = F32(F32(F32(1) / nrm) * F32(F32(nx * F32(x - xp[j])) + F32(ny * F32(y - yp[j]))))
            for o in range(O):
                ws, wd = F32(s - xo[o, h]), F32(d - yo[o, h])
                f = F32(F32(F32(-F32(ws * ws)) / F32(20.25) - F32(wd * wd) / F32(9.0)) + F32(1))
                if not f <= 0:
                    oh[o, h] += 1
                    any_hit = True
            nlb[h] += int(F32(-d + F32(p.y_lb)) > 0)
            nub[h] += int(F32(d - F32(p.y_ub)) > 0)
            vh = F32(v[h])
            vn = F32(v[h + 1]) if h + 1 < 100 else F32(v[99])
            a = F32(F32(vn - vh) / t)
            st = F32(steer[h])
            n0, n1, n2 = draws[0, r, h], draws[1, r, h], draws[2, r, h]
            if p.noise == "gaussian":
                ap = F32(F32(F32(p.sigma_acc) * abs(a)) * n0)
                sp = F32(F32(F32(p.sigma_steer) * abs(st)) * n1)
            else:
                ap = F32(F32(p.sigma_acc) * F32(F32(F32(2) * n0) - F32(1)))
                sp = F32(F32(p.K_steer * p.sigma_steer) * F32(F32(F32(2) * n1) - F32(1)))
            an = F32(F32(a + ap) + F32(F32(p.acc_const_noise) * n2))
            sn = F32(F32(st + sp) + F32(F32(p.steer_const_noise) * n2))
            sv = F32(np.sqrt(F32(F32(vx * vx) + F32(vy * vy))))
            sv = F32(sv + F32(an * t))
            psidot = F32(F32(sv * cr(np.tan, sn)) / wb)
            psi = F32(psi + F32(psidot * t))
            vx, vy = F32(sv * cr(np.cos, psi)), F32(sv * cr(np.sin, psi))
            x, y = F32(x + F32(vx * t)), F32(y + F32(vy * t))
        rows_hit += int(any_hit)
    return oh, rows_hit, int(nlb.max() + nub.max())


@pytest.mark.parametrize("noise", ["gaussian", "beta"])
def test_helper_against_scalar_loop(noise):
    R, Hn, O, P = 3, 4, 2, 9
    rng = np.random.default_rng(3)
    ora = K.CarlaCEM(4, 1, O, 0.3, Hn, noise, "Town05", 0.05, 0.01, num_batch=8, maxiter_cem=1)
    xs = np.linspace(0.0, 12.0, P).astype(F32)
    path = K.make_path(xs, (0.02 * xs * xs).astype(F32))
    init = np.array([0.5, 0.3, 6.0, 0.0, 0.1, 0.0], F32)
    v = (6.0 + 0.3 * np.arange(100)).astype(F32)
    steer = (0.05 * np.cos(np.arange(100))).astype(F32)
    xo = np.tile(np.array([[2.0], [6.0]], F32), (1, 100)) + F32(0.1) * np.arange(100, dtype=F32)
    yo = np.tile(np.array([[0.5], [-3.0]], F32), (1, 100))
    draws = rng.standard_normal((3, R, Hn)).astype(F32)
    if noise == "beta":
        draws[:2] = rng.random((2, R, Hn)).astype(F32)
    eps = rng.standard_normal((R, 4)).astype(F32)
    got = ref.reference(ora, init, v, steer, xo, yo, path, draws, eps)
    oh, rows_hit, lane = _brute(ora.prob, init, v, steer, xo, yo, path, draws, eps)
    assert np.array_equal(got["count_oh"], oh)
    assert 0 < oh.max() and oh.min() == 0, "a degenerate case shows nothing"
    assert got["count"] == oh.max() and got["count_rows"] == rows_hit and got["count_lane"] == lane
    assert lane > 0
    # the acceptance rule accepts the oracle's own counts and rejects one hit more than possible
    ok = dict(count=got["count"], count_rows=got["count_rows"], count_lane=got["count_lane"], count_oh=got["count_oh"])
    ref.check_counts(got, ok, R, "self")
    bad = dict(ok, count_oh=got["count_oh"] + (got["m"] > -ref.TOL).sum(axis=1).max() + 1)
    with pytest.raises(AssertionError):
        ref.check_counts(got, bad, R, "bad")


def test_philox_draws_layout():
    """Element r H + h of the [R][H] streams, r 4 + c of init_eps; distinct streams and keys."""
    ora = K.CarlaCEM(4, 1, 1, 0.1, 5, "gaussian", "Town05", 0.0, 0.0, num_batch=8, maxiter_cem=1)
    v, st = np.full(100, 5.0, F32), np.zeros(100, F32)
    d, e = ref.philox_draws(ora.prob, 7, 1, v, st, 6)
    assert d.shape == (3, 6, 5) and e.shape == (6, 4) and d.dtype == F32
    from oracle.rng import philox_normals
    assert np.array_equal(d[2].reshape(-1), philox_normals((7, 1), 34, 0, 30))
    assert not np.array_equal(d[0], d[1]) and not np.array_equal(d[0], ref.philox_draws(ora.prob, 8, 1, v, st, 6)[0][0])


# ------------------------------------------------------------ replay driver
def _driver():
    spec = importlib.util.spec_from_file_location("mpcmmd_carla_validate_replay",
                                                  os.path.join(CARLA, "validate_replay.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_replay_driver_accounting(tmp_path):
    D = _driver()
    rec = dict(ego=np.zeros((10, 6), F32))
    seen = []

    def inputs(rec_, prob, k):
        return np.full(6, k, F32), np.zeros((2, 100), F32), np.zeros((2, 100), F32), dict(tick=k)

    def solve(prob, cost, k, init, mean, cov, xo, yo, v_des, path):
        seen.append((cost, k, np.array(mean), float(v_des), float(init[0]), path["tick"]))
        assert np.array_equal(cov, D.COV)
        return None, None, np.full(100, k, F32), np.full(100, -k, F32), np.asarray(mean, F32) + F32(1)

    calls = []

    def validate(prob, plans, num_rollouts, seed):
        calls.append([p["tick"] for p in plans])
        assert all(p["key"] == p["tick"] and p["v_best"][0] == p["tick"] and p["steering"][0] == -p["tick"]
                   for p in plans)
        t = np.array([p["tick"] for p in plans])
        rows = np.where(t % 2 == 0, t, 0)           # even ticks collide in `tick` of the rollouts
        return dict(count=rows // 2, count_rows=rows, count_lane=t + 100)

    lines = []
    res = D.validate_replay(rec, object(), costs=("cvar", "det"), ticks=range(3, 7), num_rollouts=8,
                            out_dir=str(tmp_path), seed=5, solve=solve, validate=validate, inputs=inputs,
                            log=lines.append)
    # the ticks visited, in order, once per cost; mean_param restarts per cost and is carried between ticks
    assert [(c, k) for c, k, *_ in seen] == [(c, k) for c in ("cvar", "det") for k in (3, 4, 5, 6)]
    for i, (c, k, mean, v_des, x0, pk) in enumerate(seen):
        assert np.array_equal(mean, D.MEAN + F32(i % 4)) and v_des == 10.0 and x0 == k and pk == k
    assert calls == [[3, 4, 5, 6], [3, 4, 5, 6]], "one validation call per cost with every tick"
    for cost in ("cvar", "det"):
        with np.load(tmp_path / f"validate_{cost}.npz") as z:
            assert sorted(z.files) == ["count", "count_lane", "count_rows", "num_rollouts", "tick"]
            assert np.array_equal(z["tick"], [3, 4, 5, 6]) and int(z["num_rollouts"]) == 8
            assert np.array_equal(z["count_rows"], [0, 4, 0, 6]) and np.array_equal(z["count"], [0, 2, 0, 3])
            assert np.array_equal(z["count_lane"], [103, 104, 105, 106])
            assert all(np.array_equal(z[k], res[cost][k]) for k in z.files)
    # share of ticks with count_rows > 0 = 2 / 4, mean count_rows / R = (4 + 6) / 8 / 4
    assert len(lines) == 2 and lines[0].startswith("cvar:") and lines[1].startswith("det:")
    assert "0.5000" in lines[0] and "0.312500" in lines[0]
    with pytest.raises(ValueError):
        D.validate_replay(rec, object(), costs=("saa",), ticks=[0], solve=solve, validate=validate, inputs=inputs)
