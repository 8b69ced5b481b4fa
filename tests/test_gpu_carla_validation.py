"""mpcmmd_validate_carla on the GPU against the oracle composition of
carla_validation_ref.py (its docstring states the acceptance rule).

Plans come from the library itself: a det solve (n = 4, B = 24, T = 3) of
ticks of the synthetic recording, inputs through ``tick_inputs`` as
test_gpu_carla.py's ``_tick``.  The recording, the inputs, the plans and the
oracle objects are made once per module.
"""
import importlib
import importlib.util
import os

import numpy as np
import pytest

import carla_validation_ref as ref
from oracle import carla as K
from test_gpu_carla import COV, MEAN, carla_package

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CARLA = os.path.join(ROOT, "mpc-mmd_amd", "carla")
F32 = np.float32
TICKS = (60, 100, 170)
O, H, LEVEL, CONST = 3, 60, 0.3, (0.05, 0.01)
VARIANT = {"Town05": "carla_town05", "Town10HD": "carla_town10hd"}
# seed of the det solves: with it the oracle's det plan of tick 60 has 238 of 250 rows in collision under case
# 1's draws (seeds 0..11 scanned on the CPU; the others give 250 of 250 at every tick)
PLAN_SEED = 8


def _load(name, fname):
    spec = importlib.util.spec_from_file_location(name, os.path.join(CARLA, fname))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class World:
    """Recording, per-tick inputs and det plans, each made once."""

    def __init__(self, native):
        self.native = native
        self.R = _load("mpcmmd_carla_replay_v", "replay.py")
        self.helper = importlib.import_module(carla_package() + ".cem_helper").Helper(num_prime=H)
        self.rec = self.R.record_synthetic(ticks=171)
        self._inputs, self._plans, self._ora = {}, {}, {}

    def inputs(self, k):
        if k not in self._inputs:
            self._inputs[k] = self.R.tick_inputs(self.rec, k, self.helper, O)
        return self._inputs[k]

    def plan(self, k, town="Town05"):
        """Per-tick dict as validation.validate_plans takes it."""
        if (k, town) not in self._plans:
            init, xo, yo, path = self.inputs(k)
            N = self.native
            h = N.Handle(N.make_config(4, O, LEVEL, H, "gaussian", 0.0, 0.0, num_batch=24, maxiter_cem=3,
                                       variant=VARIANT[town], seed=PLAN_SEED))
            r = h.carla_solve("det", k, init, MEAN, COV, xo, yo, 10.0, path)
            h.close()
            self._plans[(k, town)] = dict(init=init, xo=xo, yo=yo, path=path, v_best=r["v_best"].copy(),
                                          steering=r["steering"].copy(), key=k, tick=k)
        return self._plans[(k, town)]

    def ora(self, noise, town="Town05", num_obs=O, num_prime=H, level=LEVEL, const=CONST):
        key = (noise, town, num_obs, num_prime, level, const)
        if key not in self._ora:
            self._ora[key] = K.CarlaCEM(4, 1, num_obs, level, num_prime, noise, town, const[0], const[1],
                                        num_batch=24, maxiter_cem=3)
        return self._ora[key]


@pytest.fixture(scope="module")
def world(native):
    return World(native)


def _call(native, plans, noise, R, town="Town05", draws=None, init_eps=None, seed=0, num_prime=H, level=LEVEL,
          const=CONST, keys=None):
    g = lambda n: [p[n] for p in plans]
    return native.validate_carla(g("init"), g("v_best"), g("steering"), g("xo"), g("yo"), g("path"),
                                 g("key") if keys is None else keys, num_prime, noise, level, const[0], const[1],
                                 num_rollouts=R, variant=VARIANT[town], draws=draws, init_eps=init_eps, seed=seed,
                                 count_oh=True)


def _tick_of(out, i):
    return dict(count=out["count"][i], count_rows=out["count_rows"][i], count_lane=out["count_lane"][i],
                count_oh=out["count_oh"][i])


def _ext(rng, noise, K_, R, Hn):
    d = rng.standard_normal((K_, 3, R, Hn)).astype(F32)
    if noise == "beta":
        d[:, :2] = rng.beta(2.0, 2.0, (K_, 2, R, Hn)).astype(F32)   # symmetric: the rows stay near the plan
    return d, rng.standard_normal((K_, R, 4)).astype(F32)


def _check(world, out, plans, noise, draws, eps, R, town="Town05", **kw):
    refs = []
    for i, p in enumerate(plans):
        r = ref.reference(world.ora(noise, town, **kw), p["init"], p["v_best"], p["steering"], p["xo"], p["yo"],
                          p["path"], draws[i], eps[i])
        ref.check_counts(r, _tick_of(out, i), R, f"tick {p['tick']} {noise} {town} R={R}")
        refs.append(r)
    return refs


@pytest.fixture(scope="module")
def three_ticks(world):
    """Case 1's call, shared with the K = 1 comparison: (plans, draws, eps, out)."""
    plans = [world.plan(k) for k in TICKS]
    draws, eps = _ext(np.random.default_rng(11), "gaussian", 3, 250, H)
    return plans, draws, eps, _call(world.native, plans, "gaussian", 250, draws=draws, init_eps=eps)


def test_three_ticks_external_gaussian(world, three_ticks):
    """K = 3 ticks in one call, R = 250 (no multiple of the 64 rows of a workgroup)."""
    plans, draws, eps, out = three_ticks
    refs = _check(world, out, plans, "gaussian", draws, eps, 250)
    assert any(0 < r["count_rows"] < 250 for r in refs), "degenerate: every tick hits with no row or with every row"
    assert any(0 < int(c) < 250 for c in out["count_rows"])


def test_tick_of_batch_equals_single_call(world, three_ticks):
    plans, draws, eps, out = three_ticks
    for i in range(3):
        one = _call(world.native, plans[i:i + 1], "gaussian", 250, draws=draws[i:i + 1], init_eps=eps[i:i + 1])
        for k in ("count", "count_rows", "count_lane", "count_oh"):
            assert np.array_equal(one[k][0], out[k][i]), (k, i)


def test_thousand_rollouts(world):
    """R = 1000: 16 row blocks, the last with 40 rows."""
    plans = [world.plan(100)]
    draws, eps = _ext(np.random.default_rng(12), "gaussian", 1, 1000, H)
    out = _call(world.native, plans, "gaussian", 1000, draws=draws, init_eps=eps)
    _check(world, out, plans, "gaussian", draws, eps, 1000)


def _straight(P, Hn, num_obs, length):
    """A plan along a straight path of P points with num_obs obstacles beside it."""
    xs = np.linspace(0.0, length, P).astype(F32)
    path = K.make_path(xs, np.zeros(P, F32))
    h = np.arange(100, dtype=F32)
    o = np.arange(num_obs, dtype=F32)[:, None]
    xo = (F32(1.5) + F32(3.0) * o + F32(0.3) * h[None, :]).astype(F32)
    yo = np.broadcast_to(np.where(o % 2 == 0, F32(-1.0), F32(1.5)), xo.shape).astype(F32)
    return dict(init=np.array([0.0, 0.0, 8.0, 0.0, 0.02, 0.0], F32), xo=xo, yo=yo, path=path,
                v_best=(F32(8.0) + F32(0.2) * np.sin(F32(0.3) * h)).astype(F32),
                steering=(F32(0.03) * np.cos(F32(0.2) * h)).astype(F32), key=1, tick=0)


@pytest.mark.parametrize("P,num_obs,Hn,R,length", [(37, 1, 2, 1, 36.0), (2048, 32, 100, 65, 300.0)])
def test_shape_limits(world, P, num_obs, Hn, R, length):
    """The smallest and the largest accepted shape (the largest: 130 KiB of LDS per workgroup)."""
    plans = [_straight(P, Hn, num_obs, length)]
    draws, eps = _ext(np.random.default_rng(13), "gaussian", 1, R, Hn)
    out = _call(world.native, plans, "gaussian", R, draws=draws, init_eps=eps, num_prime=Hn)
    refs = _check(world, out, plans, "gaussian", draws, eps, R, num_obs=num_obs, num_prime=Hn)
    assert refs[0]["count"] > 0


def test_town10hd_lane_bounds(world):
    plans = [world.plan(170, "Town10HD")]
    draws, eps = _ext(np.random.default_rng(14), "gaussian", 1, 250, H)
    out = _call(world.native, plans, "gaussian", 250, town="Town10HD", draws=draws, init_eps=eps)
    refs = _check(world, out, plans, "gaussian", draws, eps, 250, town="Town10HD")
    other = _call(world.native, plans, "gaussian", 250, town="Town05", draws=draws, init_eps=eps)
    assert refs[0]["count_lane"] > 0 and int(other["count_lane"][0]) != int(out["count_lane"][0])
    assert np.array_equal(other["count_oh"], out["count_oh"]), "the town changes the lane bounds only"


def test_beta_external(world):
    plans = [world.plan(100)]
    draws, eps = _ext(np.random.default_rng(15), "beta", 1, 250, H)
    out = _call(world.native, plans, "beta", 250, draws=draws, init_eps=eps)
    _check(world, out, plans, "beta", draws, eps, 250)


@pytest.mark.parametrize("noise", ["gaussian", "beta"])
def test_internal_streams(world, noise):
    """draws = init_eps = NULL: the documented Philox streams, reproduced by the oracle's generators."""
    p = world.plan(100)
    key, seed, R = 4242, 9, 250
    out = _call(world.native, [p], noise, R, seed=seed, keys=[key])
    d, e = ref.philox_draws(world.ora(noise).prob, key, seed, p["v_best"], p["steering"], R)
    _check(world, out, [p], noise, d[None], e[None], R)
    again = _call(world.native, [p], noise, R, seed=seed, keys=[key])
    other = _call(world.native, [p], noise, R, seed=seed, keys=[key + 1])
    for k in ("count", "count_rows", "count_lane", "count_oh"):
        assert np.array_equal(out[k], again[k]), k
    assert not np.array_equal(out["count_oh"], other["count_oh"])
    # one of the two tensors given, the other internal
    mixed = _call(world.native, [p], noise, R, seed=seed, keys=[key], draws=d[None])
    assert np.array_equal(mixed["count_oh"], out["count_oh"])


def test_validate_replay_end_to_end(world, tmp_path):
    """validate_replay on ticks 58..61, det, R = 64: its arrays are those of a direct call on the same plans."""
    D = _load("mpcmmd_carla_validate_replay_v", "validate_replay.py")
    cem = importlib.import_module(carla_package() + ".cem")
    prob = cem.CEM(4, 1, O, LEVEL, H, "gaussian", "Town05", CONST[0], CONST[1], num_batch=24, maxiter_cem=3)
    lines = []
    res = D.validate_replay(world.rec, prob, costs=("det",), ticks=range(58, 62), num_rollouts=64,
                            out_dir=str(tmp_path), seed=3, log=lines.append)["det"]
    plans = D.solve_ticks(prob, world.rec, "det", range(58, 62))
    prob.handle.close()
    assert [p["tick"] for p in plans] == [58, 59, 60, 61]
    assert not np.array_equal(plans[1]["mean_param"], plans[0]["mean_param"])
    direct = _call(world.native, plans, "gaussian", 64, seed=3)
    with np.load(tmp_path / "validate_det.npz") as z:
        for k in ("count", "count_rows", "count_lane"):
            assert np.array_equal(z[k], direct[k]) and np.array_equal(res[k], direct[k]), k
        assert np.array_equal(z["tick"], [58, 59, 60, 61]) and int(z["num_rollouts"]) == 64
    assert len(lines) == 1 and lines[0].startswith("det: 4 ticks")
