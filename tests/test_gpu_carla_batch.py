"""Batched CARLA solves (mpcmmd_carla_solve_batch): every tick of a batch is
bit-equal to the same tick solved alone by mpcmmd_carla_solve on a
max_configs = 1 handle, the oracle-checked path (tests/test_gpu_carla.py).

Inputs are ticks of a synthetic replay (mpc-mmd_amd/carla/replay.py) through
the library's own path helpers.  Every comparison is np.array_equal on cx, cy,
cost_lane, cost_obs, sigma, res_beta, beta, steering, v_best and mean_param:
no tolerance, the contract mpcmmd_solve_batch states.  Every case keeps
G * B <= 512, so both handles have gen_wave = 1.  H = 60, O = 3, internal RNG.
"""
import ctypes as C
import importlib
import importlib.util
import os

import numpy as np
import pytest

from test_gpu_carla import COV, MEAN, carla_package

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CARLA = os.path.join(ROOT, "mpc-mmd_amd", "carla")
H, O = 60, 3
KEYS = ("cx", "cy", "cost_lane", "cost_obs", "sigma", "res_beta", "beta", "steering", "v_best", "mean_param")
F32 = np.float32


def _load(name, fname):
    spec = importlib.util.spec_from_file_location(name, os.path.join(CARLA, fname))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class World:
    """Recordings, per-tick inputs and the results of ticks solved alone, each made once."""

    def __init__(self):
        self.R = _load("mpcmmd_carla_replay_b", "replay.py")
        self.helper = importlib.import_module(carla_package() + ".cem_helper").Helper(num_prime=H)
        self._rec, self._inputs, self._alone = {}, {}, {}

    def rec(self, town="Town05", ticks=91):
        if (town, ticks) not in self._rec:
            self._rec[(town, ticks)] = self.R.record_synthetic(ticks=ticks, town=town)
        return self._rec[(town, ticks)]

    def inputs(self, k, town="Town05"):
        if (town, k) not in self._inputs:
            self._inputs[(town, k)] = self.R.tick_inputs(self.rec(town), k, self.helper, O)
        return self._inputs[(town, k)]


@pytest.fixture(scope="module")
def world():
    return World()


def _cfg(native, n, B, noise="gaussian", level=0.1, T=3, town="Town05"):
    return native.make_config(n, O, level, H, noise, 0.0, 0.0, num_batch=B, maxiter_cem=T,
                              variant="carla_town10hd" if town == "Town10HD" else "carla_town05")


def _means(G):
    """MEAN with the speeds scaled by 0.9, 1.0, 1.1, ..."""
    out = np.tile(MEAN, (G, 1))
    out[:, :4] *= (F32(0.9) + F32(0.1) * np.arange(G, dtype=F32))[:, None]
    return out.astype(F32)


def _batch_args(world, ticks, town="Town05"):
    ins = [world.inputs(k, town) for k in ticks]
    return (np.stack([i[0] for i in ins]), np.stack([i[1] for i in ins]), np.stack([i[2] for i in ins]),
            [i[3] for i in ins])


def _same(got, want, what):
    for k in KEYS:
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), (what, k, got[k], want[k])


def _alone(native, world, cost, cfg_args, ticks, idx, means, town="Town05"):
    """The ticks solved one by one on a max_configs = 1 handle."""
    h = native.Handle(_cfg(native, town=town, **cfg_args))
    assert h.info("gen_wave") == 1 and h.max_configs == 1
    out = []
    for k, i, m in zip(ticks, idx, means):
        init, xo, yo, path = world.inputs(k, town)
        out.append(h.carla_solve(cost, i, init, m, COV, xo, yo, 10.0, path))
    h.close()
    return out


def _batch_equals_alone(native, world, cost, cfg_args, ticks, idx, town="Town05", then_partial=False):
    G = len(ticks)
    means = _means(G)
    alone = _alone(native, world, cost, cfg_args, ticks, idx, means, town)
    assert any(not np.array_equal(alone[0]["cx"], a["cx"]) for a in alone[1:]), "ticks with equal plans show nothing"
    hb = native.Handle(_cfg(native, town=town, **cfg_args), max_configs=G)
    assert hb.info("gen_wave") == 1 and hb.info("capacity") == G * cfg_args["B"] <= 512
    inits, xo, yo, paths = _batch_args(world, ticks, town)
    got = hb.carla_solve_batch(cost, idx, inits, means, COV, xo, yo, 10.0, paths)
    assert len(got) == G
    for g in range(G):
        _same(got[g], alone[g], f"{cost} tick {ticks[g]} of {G}")
    if then_partial:  # a partly filled handle, with the previous batch's state in every buffer
        got2 = hb.carla_solve_batch(cost, idx[1:], inits[1:], means[1:], COV, xo[1:], yo[1:], 10.0, paths[1:])
        assert len(got2) == G - 1
        for g in range(1, G):
            _same(got2[g - 1], alone[g], f"{cost} tick {ticks[g]} of the partly filled handle")
    hb.close()
    return alone


@pytest.mark.parametrize("cost,n", [("mmd_opt", 4), ("cvar", 12), ("det", 4)])
def test_batch_equals_alone(native, world, cost, n):
    """G = 3: three ticks with different paths, obstacles, ego states and means; then ticks (60, 90) as
    n_cfg = 2 on the same handle."""
    _batch_equals_alone(native, world, cost, dict(n=n, B=24), (40, 60, 90), [5, 6, 7], then_partial=True)


@pytest.mark.parametrize("cost,n", [("cvar", 12), ("det", 4)])
def test_batch_straddling_blocks(native, world, cost, n):
    """B = 22 (B % 4 == 2), G = 3: a four-candidate block of k_front over candidates 20..23 would span two
    configurations; the configuration-aligned launch stages each block's own path and det tracks."""
    _batch_equals_alone(native, world, cost, dict(n=n, B=22), (40, 60, 90), [5, 6, 7])


def test_batch_per_iteration_kernels(native, world):
    """mmd_opt at n = 18 (M = 324 > 256: no k_bcem_small): the batch's 72 candidates run the beta-CEM as
    small groups on two streams, each tick alone (24 candidates) on one stream."""
    _batch_equals_alone(native, world, "mmd_opt", dict(n=18, B=24, T=2), (40, 60, 90), [5, 6, 7])


@pytest.mark.parametrize("cost,n", [("cvar", 12), ("mmd_opt", 4)])
def test_batch_beta_noise(native, world, cost, n):
    """Beta noise at level 0.3: the CARLA Beta planes (cvar) and the mother rows' Beta draws (mmd_opt)
    with a configuration axis."""
    _batch_equals_alone(native, world, cost, dict(n=n, B=24, noise="beta", level=0.3), (40, 60), [5, 6])


def test_batch_town10hd(native, world):
    _batch_equals_alone(native, world, "cvar", dict(n=12, B=24), (40, 60), [5, 6], town="Town10HD")


def test_batch_graph(native, world):
    """Whole-solve graphs: the capture and the replay both equal the launched sequence."""
    ticks, idx = (40, 60), [5, 6]
    means = _means(2)
    alone = _alone(native, world, "cvar", dict(n=12, B=24), ticks, idx, means)
    hb = native.Handle(_cfg(native, 12, 24), max_configs=2)
    inits, xo, yo, paths = _batch_args(world, ticks)
    plain = hb.carla_solve_batch("cvar", idx, inits, means, COV, xo, yo, 10.0, paths)
    hb.set_graphs(1)
    for what in ("capture", "replay"):
        got = hb.carla_solve_batch("cvar", idx, inits, means, COV, xo, yo, 10.0, paths)
        for g in range(2):
            _same(got[g], plain[g], f"graph {what} vs launched, tick {ticks[g]}")
            _same(got[g], alone[g], f"graph {what} vs alone, tick {ticks[g]}")
    hb.close()


def _raw_begin_batch(native, h, n_cfg, cost, inits, means, xo, yo, paths):
    """mpcmmd_carla_begin_batch as the C caller sees it: (status, mpcmmd_last_error)."""
    L = native.lib()
    G = len(paths)
    f = lambda a: np.ascontiguousarray(np.asarray(a, F32))
    keep = dict(idx=np.arange(5, 5 + G, dtype=np.int32), init=f(inits), mean=f(means), cov=f(np.tile(COV.reshape(-1), G)),
                xo=f(xo), yo=f(yo), vd=np.full(G, 10.0, F32))
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    pths = (native.Path * G)(*paths)
    rc = L.mpcmmd_carla_begin_batch(h._h, n_cfg, native.COST[cost], keep["idx"].ctypes.data_as(C.POINTER(C.c_int32)),
                                    fp(keep["init"]), fp(keep["mean"]), fp(keep["cov"]), fp(keep["xo"]),
                                    fp(keep["yo"]), fp(keep["vd"]), pths)
    return rc, L.mpcmmd_last_error().decode()


def test_batch_arguments(native, world):
    ticks = (40, 60, 90, 60)
    inits, xo, yo, pdicts = _batch_args(world, ticks)
    means = _means(4)
    made = [native.make_path(p) for p in pdicts]      # (Path, keep): 600 points each
    paths = [m[0] for m in made]
    E_INVALID = -1
    # a static handle
    hs = native.Handle(native.make_config(4, O, 0.1, H, "gaussian", 0.0, 0.0, num_batch=24, maxiter_cem=3), max_configs=3)
    rc, msg = _raw_begin_batch(native, hs, 3, "cvar", inits[:3], means[:3], xo[:3], yo[:3], paths[:3])
    assert rc == E_INVALID and "CARLA" in msg, (rc, msg)
    hs.close()
    hb = native.Handle(_cfg(native, 12, 24), max_configs=3)
    # n_cfg = 4 on max_configs = 3 (and 0)
    for bad in (4, 0):
        rc, msg = _raw_begin_batch(native, hb, bad, "cvar", inits, means, xo, yo, paths)
        assert rc == E_INVALID and "max_configs" in msg, (bad, rc, msg)
    # paths of 600 and 599 points in one batch
    short, keep_short = native.make_path({k: np.asarray(v)[:599] for k, v in pdicts[1].items()})
    assert paths[0].num_path == 600 and short.num_path == 599
    rc, msg = _raw_begin_batch(native, hb, 3, "cvar", inits[:3], means[:3], xo[:3], yo[:3], [paths[0], short, paths[2]])
    assert rc == E_INVALID and "same num_path" in msg, (rc, msg)
    # a path with a NULL array (the last configuration's), and num_path out of range
    broken = native.Path(600, paths[2].x_path, paths[2].y_path, paths[2].arc_vec, None, paths[2].Fy_dot, paths[2].kappa)
    rc, msg = _raw_begin_batch(native, hb, 3, "cvar", inits[:3], means[:3], xo[:3], yo[:3], [paths[0], paths[1], broken])
    assert rc == E_INVALID and "six arrays" in msg, (rc, msg)
    tiny = native.Path(3, *[getattr(paths[0], k) for k in native.PATH_KEYS])
    rc, msg = _raw_begin_batch(native, hb, 3, "cvar", inits[:3], means[:3], xo[:3], yo[:3], [tiny, tiny, tiny])
    assert rc == E_INVALID and "num_path" in msg, (rc, msg)
    # a null array, a null path list
    L = native.lib()
    assert L.mpcmmd_carla_begin_batch(hb._h, 1, 2, None, None, None, None, None, None, None, (native.Path * 1)(paths[0])) \
        == E_INVALID and "null" in L.mpcmmd_last_error().decode()
    rc, _ = _raw_begin_batch(native, hb, 3, "cvar", inits[:3], means[:3], xo[:3], yo[:3], paths[:3])
    assert rc == 0, "the same arguments with three good paths begin"
    hb.sync()
    # the single-tick carla_solve on the batch handle equals the default handle's
    alone = _alone(native, world, "cvar", dict(n=12, B=24), (60,), [6], [means[1]])
    init, xo1, yo1, path = world.inputs(60)
    got = hb.carla_solve("cvar", 6, init, means[1], COV, xo1, yo1, 10.0, path)
    _same(got, alone[0], "carla_solve on a max_configs = 3 handle")
    hb.close()


def test_dropin_batch(native, world, tmp_path):
    """CEM(max_configs=3).compute_cem_batch returns the tuples of three compute_cem_cvar calls on a default
    CEM; validate_replay(replicas=3): [3, 3] arrays whose chain 0 is the replicas=1 result."""
    cem = importlib.import_module(carla_package() + ".cem")
    args = (12, 1, O, 0.1, H, "gaussian", "Town05", 0.0, 0.0)
    one = cem.CEM(*args, num_batch=24, maxiter_cem=3)
    three = cem.CEM(*args, num_batch=24, maxiter_cem=3, max_configs=3)
    assert one.max_configs == 1 and three.handle.max_configs == 3
    ticks, idx = (40, 60, 90), [5, 6, 7]
    means = _means(3)
    inits, xo, yo, paths = _batch_args(world, ticks)
    got = three.compute_cem_batch("cvar", idx, inits, means, COV, xo, yo, 10.0, paths)
    assert len(got) == 3
    for g in range(3):
        p = paths[g]
        want = one.compute_cem_cvar(idx[g], inits[g], means[g], COV, xo[g], yo[g], 10.0, p["x_path"], p["y_path"],
                                    p["arc_vec"], p["Fx_dot"], p["Fy_dot"], p["kappa"])
        assert len(got[g]) == len(want) == 5
        for a, b in zip(got[g], want):
            assert np.array_equal(a, b), (g, a, b)
    with pytest.raises(ValueError):
        three.compute_cem_batch("saa", idx, inits, means, COV, xo, yo, 10.0, paths)
    D = _load("mpcmmd_carla_validate_replay_b", "validate_replay.py")
    rec = world.rec(ticks=61)
    l1, l3 = [], []
    r1 = D.validate_replay(rec, one, costs=("cvar",), ticks=range(58, 61), num_rollouts=64,
                           out_dir=str(tmp_path / "one"), log=l1.append)["cvar"]
    r3 = D.validate_replay(rec, three, costs=("cvar",), ticks=range(58, 61), replicas=3, num_rollouts=64,
                           out_dir=str(tmp_path / "three"), log=l3.append)["cvar"]
    one.handle.close()
    three.handle.close()
    for k in ("count", "count_rows", "count_lane", "tick"):
        assert r3[k].shape == (3, 3) and r1[k].shape == (3,), k
        assert np.array_equal(r3[k][0], r1[k]), (k, r3[k], r1[k])
    assert int(r3["replica_key_stride"]) == 100000 and "replica_key_stride" not in r1
    assert len(l3) == 1 and "3 ticks x 3 replicas" in l3[0] and "+-" in l3[0] and "+-" not in l1[0]
    with np.load(tmp_path / "three" / "validate_cvar.npz") as z:
        assert z["count_rows"].shape == (3, 3) and np.array_equal(z["count_rows"], r3["count_rows"])
