"""Closed-loop episodes on the GPU (CEM.run_episodes, carla/closed_loop.py): the
chained run (mpcmmd_world_run: begin, CEM and k_world_step enqueued per tick,
nothing crossing the host) and the loop stepped by k_world_step through the
host against the same loop stepped by the host twin -- every log row, every
tick's cx, cy, steering and mean_param and the final device path bit-equal --
a run split in two, an episode alone against the same key inside a batch of 3,
and a sanity run on an open road.  Small shapes: num_batch 20, maxiter_cem 3, num_prime 8, 2
obstacles, 37 waypoints, 5 vehicles, 3 episodes x 6 ticks."""
import importlib

import numpy as np
import pytest

import world_model as wm
from test_carla_tick_cpu import carla_package

pytestmark = pytest.mark.gpu

F32 = np.float32
OUT = ("log_d", "log_f", "log_i", "done_tick", "collided", "goal", "cx", "cy", "steering", "mean_param")
E, T, P = 3, 6, 37


@pytest.fixture(autouse=True)
def pin_generators(monkeypatch):
    """MPCMMD_GENWAVE is read when a handle is created: every handle of these tests gets the same
    beta-CEM generators whatever its capacity, so runs of 1 and of 3 episodes compare bit for bit."""
    monkeypatch.setenv("MPCMMD_GENWAVE", "1")


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def make_prob(n, noise="gaussian", max_configs=E):
    cem = importlib.import_module(carla_package() + ".cem")
    return cem.CEM(n, 1, 2, 0.1, 8, noise, "Town05", 0.05, 0.01, num_batch=20, maxiter_cem=3, max_configs=max_configs)


@pytest.fixture(scope="module")
def world():
    """The synthetic route, 5 vehicles around its first 60 m, 3 starts 4 m apart."""
    (rx, ry, *_), len_path = wm.synthetic_route()
    vehicles = np.array([[25, 0.2, 0, 0, 0], [40, -3.5, 1.0, 0, 0], [55, 0, 0, 0, 0.1], [-20, 0, 0, 0, 0],
                         [70, 4, 0, 0.5, 1.0]], F32)
    starts = np.array([[0, 0, 3.0, 0], [4, -0.5, 5.0, 0.05], [8, 0.5, 1.0, -0.05]], float)
    return (rx, ry), len_path - 1, vehicles, starts


@pytest.mark.parametrize("cost,n,noise", [("cvar", 4, "gaussian"), ("det", 4, "beta"), ("mmd", 4, "gaussian")])
def test_device_stepped_loop_equals_host_stepped_loop(native, world, cost, n, noise):
    route, goal, vehicles, starts = world
    # cvar: given variates (the override); det, mmd: drawn by the library after each tick's solve -- for
    # Beta noise from that tick's controls, which only a draw inside the step can do
    u = np.random.default_rng(3).standard_normal((T, E, 4)) if cost == "cvar" else None
    prob = make_prob(n, noise)
    try:
        kw = dict(goal_index=goal, num_path=P, u=u)
        chain = prob.run_episodes(cost, route, vehicles, starts, T, chained=True, **kw)
        path_chain = prob.handle.read("path").copy()
        halves = prob.run_episodes(cost, route, vehicles, starts, T, chained=(3, 3), **kw)
        dev = prob.run_episodes(cost, route, vehicles, starts, T, device_step=True, **kw)
        host = prob.run_episodes(cost, route, vehicles, starts, T, device_step=False, **kw)
        path_host = prob.handle.read("path").copy()
        alone = [prob.run_episodes(cost, route, vehicles, starts[e:e + 1], T, chained=True, goal_index=goal,
                                   num_path=P, u=None if u is None else u[:, e:e + 1], key_base=100000 * e)
                 for e in range(E)]
    finally:
        prob.close()
    for k in OUT:
        assert same(dev[k], host[k]), k
        assert same(chain[k], host[k]), ("chained", k, np.argwhere(chain[k] != host[k])[:4])
        assert same(halves[k], host[k]), ("run(0, 3) + run(3, 3)", k)
    assert same(path_chain, path_host) and np.abs(path_host).sum() > 0
    # the loop is closed: the ego moved, the plans differ from tick to tick and between the episodes
    assert (dev["log_d"][-1, :, 0] > starts[:, 0] + 0.3).all()
    assert not same(dev["cx"][0], dev["cx"][T - 1]) and not same(dev["cx"][:, 0], dev["cx"][:, 1])
    uu = dev["log_f"][:, :, 7:11]
    if u is not None:
        assert same(uu, u.astype(F32))
    else:
        assert np.unique(uu[:, :, 2]).size == T * E, "every (tick, episode) its own variates"
        if noise == "beta":
            assert ((uu[:, :, :2] >= 0) & (uu[:, :, :2] <= 1)).all() and np.unique(uu[:, :, 0]).size > T
    # every episode alone, under its own key, equals its slot in the batch of 3
    for e in range(E):
        for k in OUT:
            a = alone[e][k]
            assert same(a[:, 0] if a.ndim > 1 else a[0], dev[k][:, e] if dev[k].ndim > 1 else dev[k][e]), (e, k)


def test_open_road_sanity(native):
    """det, 40 ticks, no vehicle near: the arc of the closest route point never decreases, no flag
    is raised and the ego stays inside the lane bounds."""
    (rx, ry, *_), len_path = wm.synthetic_route()
    prob = make_prob(4, max_configs=2)
    try:
        out = prob.run_episodes("det", (rx, ry), np.array([[1e4, 1e4, 0, 0, 0]], F32),
                                np.array([[0, 0, 2.0, 0], [10, -0.2, 4.0, 0]], float), 40, goal_index=len_path - 1,
                                num_path=P, chained=True)
    finally:
        prob.close()
    arc, d = out["log_d"][:, :, 2], out["log_f"][:, :, 12]
    assert (np.diff(arc, axis=0) >= 0).all() and (arc[-1] > arc[0] + 2).all()
    assert not out["log_i"][:, :, 1:].any() and (out["done_tick"] == -1).all()
    assert (d > prob.y_lb).all() and (d < prob.y_ub).all()


def test_world_context_errors(native, world):
    """A run before a reset is a state error; a model that does not match the tick context, too many
    episodes, a covariance that is not positive definite and a tick range past max_ticks are invalid."""
    route, goal, vehicles, starts = world
    syn, _ = wm.synthetic_route()
    cfg = native.make_config(4, 2, 0.1, 8, "gaussian", 0.05, 0.01, num_batch=20, variant="carla_town05", maxiter_cem=3)
    handle = native.Handle(cfg, max_configs=E)
    cov = np.diag([20.0] * 4 + [100.0] * 4).astype(F32)
    try:
        pdot = native.host_constant(cfg, "Pdot").reshape(-1, 11)[:4]
        model = wm.native_model(native, wm.small_world(syn, goal, num_path=P, num_obs=2, total_obs=5), pdot)
        tk = native.Tick(handle, P)
        for bad in (dict(num_path=64), dict(num_obs=3)):
            other = wm.native_model(native, wm.small_world(syn, goal, **{**dict(num_path=P, num_obs=2), **bad}), pdot)
            with pytest.raises(native.NativeError):
                native.World(tk, other, 4)
        w = native.World(tk, model, 4)
        with pytest.raises(native.NativeError, match="before mpcmmd_world_reset"):
            w.run("cvar", 0, 1, cov, 10.0)
        st = (starts[:, :2], np.zeros((E, 3)), np.tile(vehicles[None], (E, 1, 1)), np.zeros((E, 8)))
        with pytest.raises(native.NativeError, match="positive definite"):
            w.reset(*st, -cov, np.zeros((4, E, 4)), np.arange(E))
        with pytest.raises(native.NativeError, match="n_episodes"):
            w.reset(np.zeros((E + 1, 2)), np.zeros((E + 1, 3)), np.zeros((E + 1, 5, 5)), np.zeros((E + 1, 8)), cov,
                    np.zeros((4, E + 1, 4)), np.arange(E + 1))
        w.reset(*st, cov, None, 100000 * np.arange(E))
        with pytest.raises(native.NativeError, match="tick range"):
            w.run("cvar", 3, 2, cov, 10.0)
        w.close()
    finally:
        handle.close()
