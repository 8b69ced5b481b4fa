"""The CARLA tick route on the GPU (mpcmmd_carla_tick_begin_batch /
mpcmmd_carla_tick_solve_batch): the per-tick path smoothing, path parameters,
obstacle tracks, noisy rows and KKT columns made by k_tick.hip from the raw
tick data.

The reference of every comparison is the host route of the same library: the
host helpers (``replay.tick_inputs``), then ``carla_begin_batch`` /
``carla_solve_batch`` on a second handle of the same configuration
(tests/test_gpu_carla.py and tests/test_carla_host.py hold that route to the
oracle).  The contract is bit equality, buffer for buffer and result for
result: floats are compared by their bit patterns, no tolerance anywhere.
H = 60, O = 3, T = 3; G * B <= 512 on every handle, so gen_wave matches.
"""
import ctypes as C
import importlib

import numpy as np
import pytest

from test_carla_tick_cpu import World, _load, carla_package, edge_inputs, helper_chain, same_bits
from test_gpu_carla import COV, MEAN
from test_gpu_carla_batch import KEYS

pytestmark = pytest.mark.gpu

H, O, T = 60, 3, 3
F32 = np.float32
SETUP_BUFFERS = ("path", "st0r", "obs", "solve_c", "st0", "pop", "mean", "cov")


@pytest.fixture(scope="module")
def world():
    return World()


def _cfg(native, n, B, noise="gaussian", level=0.1, town="Town05", num_obs=O):
    return native.make_config(n, num_obs, level, H, noise, 0.0, 0.0, num_batch=B, maxiter_cem=T,
                              variant="carla_town10hd" if town == "Town10HD" else "carla_town05")


def _means(G):
    out = np.tile(MEAN, (G, 1))
    out[:, :4] *= (F32(0.9) + F32(0.1) * np.arange(G, dtype=F32))[:, None]
    return out.astype(F32)


class Ticks:
    """The raw inputs of some ticks and the host helpers' outputs for them."""

    def __init__(self, world, raws):
        self.init = np.stack([r[0] for r in raws])
        self.xw = np.stack([r[1] for r in raws])
        self.yw = np.stack([r[2] for r in raws])
        self.ob = np.stack([r[3] for r in raws])
        host = [helper_chain(world, r[1], r[2], r[3]) for r in raws]
        self.xo = np.stack([h[0] for h in host])
        self.yo = np.stack([h[1] for h in host])
        self.paths = [h[2] for h in host]
        self.G = len(raws)

    def sub(self, sl):
        t = object.__new__(Ticks)
        for k in ("init", "xw", "yw", "ob", "xo", "yo", "paths"):
            setattr(t, k, getattr(self, k)[sl])
        t.G = len(t.paths)
        return t

    def raw(self):
        return self.init, self.xw, self.yw, self.ob, 0.1


_cache = {}


def ticks_of(world, ticks, town="Town05", num_path=600):
    key = (tuple(ticks), town, num_path)
    if key not in _cache:
        rec = world.rec(town, num_path)
        _cache[key] = Ticks(world, [world.R.tick_raw_inputs(rec, k, O) for k in ticks])
    return _cache[key]


def _buffers_equal(native, tk, cost, cfg_args, num_path=600, Gmax=None):
    """Tick.begin_batch on one handle, carla_begin_batch on a second: the setup buffers are equal."""
    G = tk.G
    Gmax = Gmax or G
    idx = list(range(5, 5 + G))
    means = _means(G)
    hd = native.Handle(_cfg(native, **cfg_args), max_configs=Gmax)
    hh = native.Handle(_cfg(native, **cfg_args), max_configs=Gmax)
    assert hd.info("gen_wave") == hh.info("gen_wave") == 1 and hd.info("capacity") <= 512
    tick = native.Tick(hd, num_path)
    tick.begin_batch(cost, idx, *tk.raw(), means, COV, 10.0)
    hh.carla_begin_batch(cost, idx, tk.init, means, COV, tk.xo, tk.yo, 10.0, tk.paths)
    names = SETUP_BUFFERS + (("obs_full",) if cost == "det" else ())
    for name in names:
        nb = hd.buffer_bytes(name)
        assert nb == hh.buffer_bytes(name)
        per = nb // (2 if name == "pop" else 1)
        a = hd.read(name, np.uint8).reshape(-1, per)[:, : per // Gmax * G]
        b = hh.read(name, np.uint8).reshape(-1, per)[:, : per // Gmax * G]
        assert a.size and np.array_equal(a, b), (cost, name, int((a != b).sum()))
    # the path read back through Tick.path is the host helpers' path
    for g in range(G):
        got = tick.path(g)
        for k in native.PATH_KEYS:
            assert same_bits(got[k], tk.paths[g][k]), (g, k)
    hd.close()
    hh.close()


@pytest.mark.parametrize("cost,n", [("mmd_opt", 4), ("cvar", 12), ("det", 4)])
def test_setup_buffers(native, world, cost, n):
    """G = 3 Town05 ticks at B = 22: path (padding included), st0r, obs, obs_full (det), solve_c, st0,
    pop, mean, cov after the two begins."""
    tk = ticks_of(world, (0, 60, 90))
    assert not same_bits(tk.paths[0]["y_path"], tk.paths[1]["y_path"]) and \
        not same_bits(tk.paths[1]["y_path"], tk.paths[2]["y_path"]) and \
        not same_bits(tk.paths[0]["y_path"], tk.paths[2]["y_path"]), "equal inputs show nothing"
    _buffers_equal(native, tk, cost, dict(n=n, B=22))


@pytest.mark.parametrize("num_path", [4, 37, 1025])
def test_path_lengths(native, world, num_path):
    """cvar n = 4, G = 2 at the shortest path, a length that is no multiple of the wave or the Frenet
    batch of 8, and one with more than 1024 rows (two rows per thread of k_tick_path)."""
    tk = ticks_of(world, (60, 90), num_path=num_path)
    _buffers_equal(native, tk, "cvar", dict(n=4, B=22), num_path=num_path)


def test_partly_filled_handle(native, world):
    """G = 2 ticks on a max_configs = 3 handle: the first two slices."""
    _buffers_equal(native, ticks_of(world, (60, 90)), "cvar", dict(n=4, B=22), Gmax=3)


def test_edge_inputs(native, world):
    """No obstacle kept (the three placeholders 300 m away) and a NaN obstacle x (the first-NaN
    closest index): the buffers are equal, NaNs included."""
    tk = Ticks(world, [raw for _, raw in edge_inputs(world)])
    assert np.isnan(tk.yo[1]).any()
    for cost, n in (("cvar", 4), ("det", 4)):
        _buffers_equal(native, tk, cost, dict(n=n, B=22))


def _same(got, want, what):
    for k in KEYS:
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), (what, k, got[k], want[k])
        assert same_bits(got[k], want[k]), (what, k)


def _solves_equal(native, world, cost, cfg_args, ticks, town="Town05", graphs=False):
    tk = ticks_of(world, ticks, town)
    G = tk.G
    idx = list(range(5, 5 + G))
    means = _means(G)
    cfg_args = dict(cfg_args, town=town)
    hd = native.Handle(_cfg(native, **cfg_args), max_configs=G)
    hh = native.Handle(_cfg(native, **cfg_args), max_configs=G)
    assert hd.info("gen_wave") == hh.info("gen_wave") == 1 and hd.info("capacity") == G * cfg_args["B"] <= 512
    tick = native.Tick(hd, 600)
    want = hh.carla_solve_batch(cost, idx, tk.init, means, COV, tk.xo, tk.yo, 10.0, tk.paths)
    assert any(not np.array_equal(want[0]["cx"], w["cx"]) for w in want[1:]), "ticks with equal plans show nothing"
    got = tick.solve_batch(cost, idx, *tk.raw(), means, COV, 10.0)
    assert len(got) == G
    for g in range(G):
        _same(got[g], want[g], f"{cost} tick {ticks[g]}")
    if graphs:
        hd.set_graphs(1)
        for what in ("capture", "replay"):
            got = tick.solve_batch(cost, idx, *tk.raw(), means, COV, 10.0)
            for g in range(G):
                _same(got[g], want[g], f"{cost} graph {what}, tick {ticks[g]}")
    else:  # a second batch of two ticks on the same context and handle: no stale state
        t2 = tk.sub(slice(1, None))
        want2 = hh.carla_solve_batch(cost, idx[1:], t2.init, means[1:], COV, t2.xo, t2.yo, 10.0, t2.paths)
        got2 = tick.solve_batch(cost, idx[1:], *t2.raw(), means[1:], COV, 10.0)
        assert len(got2) == G - 1
        for g in range(G - 1):
            _same(got2[g], want2[g], f"{cost} second batch, tick {ticks[g + 1]}")
    hd.close()
    hh.close()


@pytest.mark.parametrize("cost,n", [("mmd_opt", 4), ("cvar", 12), ("det", 4)])
def test_solves(native, world, cost, n):
    _solves_equal(native, world, cost, dict(n=n, B=24), (0, 60, 90))


def test_solves_beta_noise(native, world):
    _solves_equal(native, world, "cvar", dict(n=12, B=24, noise="beta", level=0.3), (0, 60, 90))


def test_solves_town10hd(native, world):
    _solves_equal(native, world, "cvar", dict(n=12, B=24), (10, 20, 30), town="Town10HD")


def test_solves_graphs(native, world):
    """Whole-solve graphs behind the tick begin: capture and replay give the launched sequence's bits."""
    _solves_equal(native, world, "mmd_opt", dict(n=4, B=24), (0, 60, 90), graphs=True)


def test_single_tick(native, world):
    """n_cfg = 1 on a max_configs = 1 handle equals carla_solve of the tick alone."""
    tk = ticks_of(world, (60,))
    hd = native.Handle(_cfg(native, 12, 24))
    hh = native.Handle(_cfg(native, 12, 24))
    assert hd.max_configs == 1
    want = hh.carla_solve("cvar", 6, tk.init[0], MEAN, COV, tk.xo[0], tk.yo[0], 10.0, tk.paths[0])
    got = native.Tick(hd, 600).solve_batch("cvar", [6], *tk.raw(), MEAN, COV, 10.0)
    assert len(got) == 1
    _same(got[0], want, "n_cfg = 1")
    hd.close()
    hh.close()


def _raw_begin(native, tick_ptr, n_cfg, cost, tk, threshold=0.1, drop=None):
    """mpcmmd_carla_tick_begin_batch as the C caller sees it: (status, mpcmmd_last_error)."""
    L = native.lib()
    G = tk.G
    f = lambda a: np.ascontiguousarray(np.asarray(a, F32))
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    keep = dict(idx=np.arange(5, 5 + G, dtype=np.int32), init_state=f(tk.init), x_wp=f(tk.xw), y_wp=f(tk.yw),
                obstacles=f(tk.ob), mean=f(_means(G)), cov=f(np.tile(COV.reshape(-1), G)), vd=np.full(G, 10.0, F32))
    arrs = {k: (None if k == drop else fp(keep[k])) for k in ("init_state", "x_wp", "y_wp", "obstacles")}
    tin = native.TickInputs(arrs["init_state"], arrs["x_wp"], arrs["y_wp"], arrs["obstacles"], threshold)
    rc = L.mpcmmd_carla_tick_begin_batch(tick_ptr, n_cfg, native.COST[cost],
                                         keep["idx"].ctypes.data_as(C.POINTER(C.c_int32)), C.byref(tin),
                                         fp(keep["mean"]), fp(keep["cov"]), fp(keep["vd"]))
    return rc, L.mpcmmd_last_error().decode()


def test_errors_before_any_hip_call(native, world):
    E_INVALID, E_UNSUPPORTED = -1, -3
    L = native.lib()
    tk = ticks_of(world, (0, 60, 90))
    # a static-variant handle has no tick route
    hs = native.Handle(native.make_config(4, O, 0.1, H, "gaussian", 0.0, 0.0, num_batch=24, maxiter_cem=T), max_configs=3)
    out = C.c_void_p()
    assert L.mpcmmd_tick_create(hs._h, 600, C.byref(out)) == E_INVALID and "CARLA" in L.mpcmmd_last_error().decode()
    assert not out.value
    with pytest.raises(native.NativeError):
        native.Tick(hs, 600)
    hs.close()
    hb = native.Handle(_cfg(native, 12, 24), max_configs=3)
    for bad in (3, 2049):
        assert L.mpcmmd_tick_create(hb._h, bad, C.byref(out)) == E_INVALID and "num_path" in L.mpcmmd_last_error().decode()
    tick = native.Tick(hb, 600)
    for bad in (0, 4):
        rc, msg = _raw_begin(native, tick._t, bad, "cvar", tk)
        assert rc == E_INVALID and "max_configs" in msg, (bad, rc, msg)
    for drop in ("init_state", "x_wp", "y_wp", "obstacles"):
        rc, msg = _raw_begin(native, tick._t, 3, "cvar", tk, drop=drop)
        assert rc == E_INVALID and "null" in msg, (drop, rc, msg)
    rc, msg = _raw_begin(native, tick._t, 3, "cvar", tk, threshold=float("nan"))
    assert rc == E_INVALID and "threshold" in msg, (rc, msg)
    rc, msg = _raw_begin(native, tick._t, 3, "saa", tk)
    assert rc == E_INVALID and "compute_cem" in msg, (rc, msg)
    rc, msg = _raw_begin(native, tick._t, 3, "cvar", tk)
    assert rc == 0, "the same arguments, all good, begin"
    hb.sync()
    hb.close()
    # det on a 33-obstacle handle
    h33 = native.Handle(_cfg(native, 4, 24, num_obs=33), max_configs=1)
    t33 = native.Tick(h33, 600)
    one = tk.sub(slice(0, 1))
    one.ob = np.repeat(one.ob, 11, axis=1)
    rc, msg = _raw_begin(native, t33._t, 1, "det", one)
    assert rc == E_UNSUPPORTED and "num_obs" in msg, (rc, msg)
    h33.close()


def test_dropin_tick_batch(native, world, tmp_path):
    """CEM.compute_cem_tick_batch returns the tuples of compute_cem_batch and each tick's path dict;
    validate_replay(device_setup=True) over 4 synthetic ticks writes npz arrays equal to the host
    route's, single chain and replicas."""
    cem = importlib.import_module(carla_package() + ".cem")
    args = (12, 1, O, 0.1, H, "gaussian", "Town05", 0.0, 0.0)
    host = cem.CEM(*args, num_batch=24, maxiter_cem=T, max_configs=3)
    dev = cem.CEM(*args, num_batch=24, maxiter_cem=T, max_configs=3)
    tk = ticks_of(world, (0, 60, 90))
    idx, means = [5, 6, 7], _means(3)
    want = host.compute_cem_batch("cvar", idx, tk.init, means, COV, tk.xo, tk.yo, 10.0, tk.paths)
    got, paths = dev.compute_cem_tick_batch("cvar", idx, tk.init, tk.xw, tk.yw, tk.ob, 0.1, means, COV, 10.0)
    assert len(got) == len(paths) == 3
    for g in range(3):
        assert len(got[g]) == len(want[g]) == 5
        for a, b in zip(got[g], want[g]):
            assert same_bits(a, b), (g, a, b)
        for k in native.PATH_KEYS:
            assert same_bits(paths[g][k], tk.paths[g][k]), (g, k)
    with pytest.raises(ValueError):
        dev.compute_cem_tick_batch("saa", idx, tk.init, tk.xw, tk.yw, tk.ob, 0.1, means, COV, 10.0)
    D = _load("mpcmmd_carla_validate_replay_tick", "validate_replay.py")
    rec = world.rec("Town05", 600)
    for replicas in (1, 3):
        rh = D.validate_replay(rec, host, costs=("cvar",), ticks=range(58, 62), num_rollouts=64, replicas=replicas,
                               out_dir=str(tmp_path / f"host{replicas}"), log=lambda s: None)["cvar"]
        rd = D.validate_replay(rec, dev, costs=("cvar",), ticks=range(58, 62), num_rollouts=64, replicas=replicas,
                               out_dir=str(tmp_path / f"dev{replicas}"), log=lambda s: None, device_setup=True)["cvar"]
        assert set(rh) == set(rd)
        with np.load(tmp_path / f"host{replicas}" / "validate_cvar.npz") as zh, \
                np.load(tmp_path / f"dev{replicas}" / "validate_cvar.npz") as zd:
            assert set(zh.files) == set(zd.files)
            for k in zh.files:
                assert zh[k].shape == zd[k].shape and np.array_equal(zh[k], zd[k]), (replicas, k)
    dev.close()
    host.handle.close()
