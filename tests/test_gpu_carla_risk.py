"""mpcmmd_validate_carla_risk on the GPU: the per-rollout costs against the
oracle composition (carla_risk_ref.py states the acceptance rule), the
statistics of the returned costs against risk_stats_ref.py and bit for bit
against mpcmmd_validate_risk on the same samples, the counts against
mpcmmd_validate_carla, determinism, the shape limits, NaN propagation, the
internal Philox streams, the second town and the replay driver end to end.
"""
import importlib

import numpy as np
import pytest

import carla_risk_ref as rref
import carla_validation_ref as vref
import risk_stats_ref as sref
from test_gpu_carla import carla_package
from test_gpu_carla_validation import CONST, LEVEL, VARIANT, H, O, _call, _ext, _load, _straight
from test_gpu_carla_validation import world  # noqa: F401  (module-scoped fixture: recording, plans, oracles)
from test_gpu_validate_risk import MMD_ATOL

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
ALPHA, SIGMA = 0.98, (0.01, 0.3)
COUNTS = ("count", "count_lane", "count_rows", "count_oh")
STATS = ("count_pos", "var", "cvar", "mean", "max", "mmd")


def _risk(native, plans, noise, R, town="Town05", draws=None, init_eps=None, seed=0, num_prime=H, level=LEVEL,
          const=CONST, keys=None, sigma=SIGMA):
    g = lambda n: [p[n] for p in plans]
    return native.validate_carla_risk(g("init"), g("v_best"), g("steering"), g("xo"), g("yo"), g("path"),
                                      g("key") if keys is None else keys, num_prime, noise, level, const[0], const[1],
                                      num_rollouts=R, variant=VARIANT[town], draws=draws, init_eps=init_eps,
                                      seed=seed, alpha=ALPHA, sigma=sigma, return_costs=True, counts=True)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == F32 else a


def _same_outputs(a, b, keys=STATS + COUNTS + ("costs",)):
    return [k for k in keys if not np.array_equal(_bits(a[k]), _bits(b[k]))]


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return (a == b) | (np.isnan(a) & np.isnan(b))


def _check_stats(native, got, label):
    """Rule 2: the statistics of the GPU's own returned costs."""
    c = got["costs"]
    exp = sref.stats(c, ALPHA, SIGMA)
    for k in ("var", "max", "count_pos"):
        assert np.all(_same(got[k], exp[k])), (label, k, got[k], exp[k])
    for k in ("cvar", "mean"):
        assert np.all(sref.ulp_close(got[k], exp[k])), (label, k, got[k], exp[k])
    finite = ~np.isnan(c).any(axis=-1)           # the MMD of a channel with a NaN sample is NaN on both sides
    err = np.abs(got["mmd"].astype(F64) - exp["mmd"].astype(F64))
    print(f"{label}: mmd max err {np.nanmax(err[finite]) if finite.any() else 0.0:.3e}")
    assert np.all(err[finite] <= MMD_ATOL), (label, got["mmd"], exp["mmd"])
    zero = (c == 0).all(axis=-1)
    assert np.all(got["mmd"][zero] == F32(-1000.0)), (label, got["mmd"][zero])
    same = native.validate_risk(costs_in=c, alpha=ALPHA, sigma=SIGMA)
    assert not _same_outputs(got, same, STATS), (label, _same_outputs(got, same, STATS))
    assert np.array_equal(got["saa"], got["count_pos"].astype(F32) / F32(c.shape[-1]))


def _check_counts(native, got, plain, label):
    """Rule 3: the counts are mpcmmd_validate_carla's."""
    for k in COUNTS:
        assert np.array_equal(got[k], plain[k]), (label, k, got[k], plain[k])
    assert np.array_equal(got["count_pos"][:, 0], got["count_rows"]), (label, got["count_pos"], got["count_rows"])
    assert np.all(got["count_lane"] <= got["count_pos"][:, 1] + got["count_pos"][:, 2]), label


def _check_all(native, got, plain, refs, label):
    for i, r in enumerate(refs):
        rref.check_costs(r, got["costs"][i], f"{label} tick {i}")
    _check_stats(native, got, label)
    _check_counts(native, got, plain, label)


# ------------------------------------------------------------------ the fixture
@pytest.fixture(scope="module")
def fix(native):
    """The three synthetic ticks: (plans, draws, eps, refs, the risk call, the plain validation call)."""
    plans, draws, eps, refs = rref.fixture_refs()
    kw = dict(draws=draws, init_eps=eps, num_prime=rref.FIX_H)
    got = _risk(native, plans, "gaussian", rref.FIX_R, **kw)
    plain = _call(native, plans, "gaussian", rref.FIX_R, **kw)
    return plans, draws, eps, refs, got, plain


def test_fixture_is_not_degenerate(fix):
    plans, draws, eps, refs, got, plain = fix
    for i, r in enumerate(refs):
        st = sref.stats(rref.channels(r), ALPHA)
        assert tuple(st["count_pos"]) == rref.FIX_COUNT_POS[i]
        assert not (np.abs(rref.decisive(r)) <= rref.TOL).any() and vref.near_share(r) == 0.0


def test_costs_against_reference(fix):
    plans, draws, eps, refs, got, plain = fix
    assert got["costs"].shape == (3, 3, rref.FIX_R) and got["costs"].dtype == F32
    for i, r in enumerate(refs):
        rref.check_costs(r, got["costs"][i], f"fixture tick {i}")
    assert np.all(got["costs"] >= 0) and not np.signbit(got["costs"]).any()


def test_statistics_of_returned_costs(native, fix):
    plans, draws, eps, refs, got, plain = fix
    _check_stats(native, got, "fixture")
    assert tuple(map(tuple, got["count_pos"])) == rref.FIX_COUNT_POS    # the reference's, no margin near zero
    assert got["var"][2, 2] == 0 and got["count_pos"][2, 2] == 1 and got["cvar"][2, 2] > 0
    assert np.all(got["mmd"][2, :2] == F32(-1000.0)) and np.all(got["mmd"][0, 2] == F32(-1000.0))
    assert np.array_equal(got["cvar_lane"], got["cvar"][:, 1] + got["cvar"][:, 2])
    assert np.array_equal(got["mmd_lane"], got["mmd"][:, 1] + got["mmd"][:, 2])


def test_counts_are_validate_carlas(native, fix):
    plans, draws, eps, refs, got, plain = fix
    _check_counts(native, got, plain, "fixture")
    assert (int(got["count"][0]), int(got["count_rows"][0])) == (222, 223)
    assert int(got["count_lane"][1]) == 12 < got["count_pos"][1, 2] == 13


def test_deterministic_and_batch_independent(native, fix):
    plans, draws, eps, refs, got, plain = fix
    again = _risk(native, plans, "gaussian", rref.FIX_R, draws=draws, init_eps=eps, num_prime=rref.FIX_H)
    assert not _same_outputs(got, again), _same_outputs(got, again)
    for i in range(3):
        one = _risk(native, plans[i:i + 1], "gaussian", rref.FIX_R, draws=draws[i:i + 1], init_eps=eps[i:i + 1],
                    num_prime=rref.FIX_H)
        diff = [k for k in STATS + COUNTS + ("costs",) if not np.array_equal(_bits(one[k][0]), _bits(got[k][i]))]
        assert not diff, (i, diff)


@pytest.mark.parametrize("P,num_obs,Hn,R,length", [(37, 1, 2, 1, 36.0), (2048, 32, 100, 65, 300.0)])
def test_shape_limits(native, world, P, num_obs, Hn, R, length):  # noqa: F811
    """The smallest shape and the LDS maximum (now with the cost table; R no multiple of 64)."""
    plans = [_straight(P, Hn, num_obs, length)]
    draws, eps = _ext(np.random.default_rng(13), "gaussian", 1, R, Hn)
    got = _risk(native, plans, "gaussian", R, draws=draws, init_eps=eps, num_prime=Hn)
    plain = _call(native, plans, "gaussian", R, draws=draws, init_eps=eps, num_prime=Hn)
    p = plans[0]
    r = vref.reference(world.ora("gaussian", "Town05", num_obs=num_obs, num_prime=Hn), p["init"], p["v_best"],
                       p["steering"], p["xo"], p["yo"], p["path"], draws[0], eps[0])
    _check_all(native, got, plain, [r], f"P={P} O={num_obs} H={Hn} R={R}")
    assert got["count_pos"][0, 0] > 0


def test_nan_propagates(native, fix):
    plans, draws, eps, refs, got, plain = fix
    R = rref.FIX_R
    p = dict(plans[1])
    p["xo"] = p["xo"].copy()
    p["xo"][0, 1] = np.nan
    bad = _risk(native, [p], "gaussian", R, draws=draws[1:2], init_eps=eps[1:2], num_prime=rref.FIX_H)
    c = bad["costs"][0]
    assert np.all(c[0].view(np.uint32) == np.uint32(0x7fc00000)), "one canonical quiet NaN per row"
    assert bad["count_pos"][0, 0] == R == bad["count_rows"][0] and np.isnan(bad["max"][0, 0])
    assert np.array_equal(_bits(c[1:]), _bits(got["costs"][1, 1:])), "the lane channels do not see the obstacle"
    for k in STATS:
        assert np.array_equal(_bits(bad[k][0, 1:]), _bits(got[k][1, 1:])), k
    _check_stats(native, bad, "nan")


@pytest.mark.parametrize("noise", ["gaussian", "beta"])
def test_internal_streams(native, world, noise):  # noqa: F811
    """draws = init_eps = NULL: the Philox streams of mpcmmd_validate_carla, reproduced by the oracle's generators."""
    p = world.plan(100)
    key, seed, R = 4242, 9, 250
    got = _risk(native, [p], noise, R, seed=seed, keys=[key])
    plain = _call(native, [p], noise, R, seed=seed, keys=[key])
    d, e = vref.philox_draws(world.ora(noise).prob, key, seed, p["v_best"], p["steering"], R)
    r = vref.reference(world.ora(noise), p["init"], p["v_best"], p["steering"], p["xo"], p["yo"], p["path"], d, e)
    rref.check_costs(r, got["costs"][0], f"internal {noise}")
    _check_counts(native, got, plain, f"internal {noise}")
    other = _risk(native, [p], noise, R, seed=seed, keys=[key + 1])
    assert not np.array_equal(_bits(other["costs"]), _bits(got["costs"]))
    assert (got["costs"] > 0).any(), "a degenerate case shows nothing"


def test_town10hd_lane_bounds(native, world):  # noqa: F811
    plans = [world.plan(170, "Town10HD")]
    draws, eps = _ext(np.random.default_rng(14), "gaussian", 1, 250, H)
    got = _risk(native, plans, "gaussian", 250, town="Town10HD", draws=draws, init_eps=eps)
    p = plans[0]
    r = vref.reference(world.ora("gaussian", "Town10HD"), p["init"], p["v_best"], p["steering"], p["xo"], p["yo"],
                       p["path"], draws[0], eps[0])
    rref.check_costs(r, got["costs"][0], "Town10HD")
    other = _risk(native, plans, "gaussian", 250, town="Town05", draws=draws, init_eps=eps)
    assert not np.array_equal(_bits(other["costs"][0, 1:]), _bits(got["costs"][0, 1:])), "the lane bounds differ"
    assert np.array_equal(_bits(other["costs"][0, 0]), _bits(got["costs"][0, 0])), "the town changes the lanes only"


def test_validate_replay_end_to_end(native, world, tmp_path):  # noqa: F811
    """validate_replay(risk=True) on ticks 58..61, det, R = 64: its arrays are those of a direct call."""
    D = _load("mpcmmd_carla_validate_replay_risk", "validate_replay.py")
    cem = importlib.import_module(carla_package() + ".cem")
    prob = cem.CEM(4, 1, O, LEVEL, H, "gaussian", "Town05", CONST[0], CONST[1], num_batch=24, maxiter_cem=3)
    lines = []
    kw = dict(costs=("det",), ticks=range(58, 62), num_rollouts=64, seed=3)
    res = D.validate_replay(world.rec, prob, out_dir=str(tmp_path / "risk"), log=lines.append, risk=True,
                            risk_sigma=(0.3,), **kw)["det"]
    D.validate_replay(world.rec, prob, out_dir=str(tmp_path / "plain"), log=lambda s: None, **kw)
    plans = D.solve_ticks(prob, world.rec, "det", range(58, 62))
    prob.handle.close()
    direct = _risk(native, plans, "gaussian", 64, seed=3, sigma=(0.3,))
    today = ["count", "count_lane", "count_rows", "num_rollouts", "tick"]
    with np.load(tmp_path / "risk" / "validate_det.npz") as z:
        assert sorted(z.files) == sorted(today + ["risk_" + k for k in STATS] + ["risk_sigma", "risk_alpha"])
        for k in ("count", "count_rows", "count_lane"):
            assert np.array_equal(z[k], direct[k]) and np.array_equal(res[k], direct[k]), k
        for k in STATS:
            assert np.array_equal(_bits(z["risk_" + k]), _bits(direct[k])), k
        assert np.array_equal(z["risk_sigma"], np.array([0.3], F32)) and z["risk_alpha"] == F32(0.98)
        assert np.array_equal(z["tick"], [58, 59, 60, 61]) and int(z["num_rollouts"]) == 64
        with np.load(tmp_path / "plain" / "validate_det.npz") as z0:
            assert sorted(z0.files) == today and all(np.array_equal(z0[k], z[k]) for k in today)
    assert len(lines) == 2 and lines[0].startswith("det: 4 ticks") and lines[1].startswith("det: risk")
