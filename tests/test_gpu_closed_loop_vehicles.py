"""Closed-loop CARLA episodes with routed vehicles on the GPU (CEM.run_episodes(
routed=)): the chained run (mpcmmd_world_route_vehicles +
mpcmmd_world_run), the run split in two and the loop stepped by the routed kernel
through the host against the loop stepped by mpcmmd_world_step_host_routed --
every log row, every tick's plan and the vehicle log bit-equal -- once with the
validation stage on, an episode alone against its slot in the batch of 3, a
policy turned on and off again against the constant-velocity run, and the
context's error cases.  Small shapes: num_batch 20, maxiter_cem 3, num_prime 8, 2
obstacles, 37 waypoints, 5 vehicles, 3 episodes x 6 ticks."""
import importlib

import numpy as np
import pytest

import world_model as wm
import world_vehicle_model as vm
from test_carla_tick_cpu import carla_package

pytestmark = pytest.mark.gpu

F32 = np.float32
OUT = ("log_d", "log_f", "log_i", "done_tick", "collided", "goal", "cx", "cy", "steering", "mean_param", "veh")
VAL = ("val_counts", "val_count_pos", "val_var", "val_cvar", "val_mean", "val_max", "val_mmd", "val_est")
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


def prob_native():
    """The binding the drop-in package loaded (by file path: its own module object, so its own ctypes classes)."""
    return importlib.import_module(carla_package() + "._lib").native()


@pytest.fixture(scope="module")
def world():
    """The synthetic route (it starts along +x: s is x there), 3 starts 4 m apart and 5 routed vehicles:
    a slow one and a parked one ahead on the ego's lane, two on the right lane, a fast one behind the
    egos, whose leader an ego is."""
    (rx, ry, *_), len_path = wm.synthetic_route()
    starts = np.array([[0, 0, 3.0, 0], [4, -0.5, 5.0, 0.05], [8, 0.5, 1.0, -0.05]], float)
    traffic = dict(s=np.array([25.0, 40.0, 55.0, -20.0, 70.0]), v=np.array([2.0, 3.0, 0.0, 4.0, 1.0], F32),
                   d=np.array([0.0, -3.5, 0.0, 0.25, -3.5], F32), v0=np.array([4.0, 5.0, 0.0, 9.0, 3.3], F32))
    return (rx, ry), len_path - 1, traffic, starts


@pytest.mark.parametrize("cost,noise,given,validate", [("cvar", "gaussian", True, None), ("det", "beta", False, None),
                                                       ("cvar", "gaussian", False, dict(rollouts=64, sigma=(0.5,)))])
def test_routed_loops_equal_the_host_stepped_loop(native, world, cost, noise, given, validate):
    route, goal, traffic, starts = world
    u = np.random.default_rng(3).standard_normal((T, E, 4)) if given else None
    prob = make_prob(4, noise)
    try:
        kw = dict(goal_index=goal, num_path=P, u=u, routed=traffic, validate=validate)
        chain = prob.run_episodes(cost, route, None, starts, T, chained=True, **kw)
        halves = prob.run_episodes(cost, route, None, starts, T, chained=(3, 3), **kw)
        dev = prob.run_episodes(cost, route, None, starts, T, device_step=True, **kw)
        host = prob.run_episodes(cost, route, None, starts, T, device_step=False, **kw)
        alone = [] if validate else [
            prob.run_episodes(cost, route, None, starts[e:e + 1], T, chained=True, goal_index=goal, num_path=P,
                              u=None if u is None else u[:, e:e + 1], key_base=100000 * e, routed=traffic)
            for e in range(E)]
    finally:
        prob.close()
    for k in OUT + (VAL if validate else ()):
        assert same(dev[k], host[k]), k
        assert same(chain[k], host[k]), ("chained", k, np.argwhere(chain[k] != host[k])[:4])
        assert same(halves[k], host[k]), ("run(0, 3) + run(3, 3)", k)
    # the loop is closed and the traffic is live, on the host's answers
    veh = host["veh"]
    assert veh.shape == (T, E, 5, 3) and (host["log_d"][-1, :, 0] > starts[:, 0] + 0.3).all()
    assert (veh[-1, :, [0, 1, 3, 4], 0] > traffic["s"][[0, 1, 3, 4], None]).all() and (veh[:, :, 2, 0] == 55.0).all()
    assert not same(veh[:, 0], veh[:, 1]), "the egos differ, so does the vehicle behind them"
    sc = vm.scalars()
    free = vm.accel(sc, traffic["v"][3], traffic["v0"][3], None)
    assert (veh[0, :, 3, 2] < float(free)).all(), "an ego is the leader of the vehicle behind"
    for e in range(len(alone)):   # every episode alone, under its own key, equals its slot in the batch of 3
        for k in OUT:
            a = alone[e][k]
            assert same(a[:, 0] if a.ndim > 1 else a[0], dev[k][:, e] if dev[k].ndim > 1 else dev[k][e]), (e, k)


def test_mmd_once(native, world):
    route, goal, traffic, starts = world
    prob = make_prob(4, "gaussian", max_configs=2)
    try:
        kw = dict(goal_index=goal, num_path=P, routed=traffic)
        chain = prob.run_episodes("mmd", route, None, starts[:2], 4, chained=True, **kw)
        host = prob.run_episodes("mmd", route, None, starts[:2], 4, device_step=False, **kw)
    finally:
        prob.close()
    for k in OUT:
        assert same(chain[k], host[k]), k


def test_policy_on_and_off_again(native, world):
    """route_vehicles(...) then route_vehicles(None): the next reset and run give the bits of a context that
    never had the policy."""
    route, goal, traffic, starts = world
    vehicles = np.array([[25, 0.2, 0, 0, 0], [40, -3.5, 1.0, 0, 0], [55, 0, 0, 0, 0.1], [-20, 0, 0, 0, 0],
                         [70, 4, 0, 0.5, 1.0]], F32)
    prob, native = make_prob(4), prob_native()
    cov = np.diag([20.0] * 4 + [100.0] * 4).astype(F32)
    try:
        plain = prob.run_episodes("cvar", route, vehicles, starts, T, chained=True, goal_index=goal, num_path=P)
        model, tk = prob.world_model(route, 5, goal, P, cov)
        w = native.World(tk, model, T)
        per = lambda a: np.tile(np.asarray(a)[None], (E, 1))
        args = (starts[:, :2], np.stack([starts[:, 2], starts[:, 3], np.zeros(E)], 1), np.tile(vehicles[None], (E, 1, 1)),
                np.tile(np.array([10.0] * 4 + [0.0] * 4, F32), (E, 1)), cov, None, 100000 * np.arange(E))
        w.route_vehicles(per(traffic["s"]), per(traffic["v"]), np.stack([per(traffic["d"]), per(traffic["v0"])], -1))
        w.reset(args[0], args[1], None, *args[3:])
        w.run("cvar", 0, T, cov, 10.0)
        on = w.log(T)
        first = w.vehicle_log(T)
        w.reset(args[0], args[1], None, *args[3:])   # every reset starts from the staged states again
        w.run("cvar", 0, T, cov, 10.0)
        assert same(w.vehicle_log(T), first) and same(w.log(T)["log_f"], on["log_f"])
        w.route_vehicles(None)
        with pytest.raises(native.NativeError, match="before mpcmmd_world_reset"):
            w.run("cvar", 0, 1, cov, 10.0)
        with pytest.raises(native.NativeError, match="without routed vehicles"):
            w.vehicle_log(1)
        w.reset(*args)
        w.run("cvar", 0, T, cov, 10.0)
        off = w.log(T)
        w.close()
    finally:
        prob.close()
    for k in ("log_d", "log_f", "log_i", "done_tick", "cx", "cy", "steering", "mean_param"):
        assert same(off[k], plain[k]), k
    assert not same(on["log_f"], plain["log_f"]) or not same(on["cx"], plain["cx"])


def test_context_errors(native, world):
    import ctypes as C
    route, goal, traffic, starts = world
    prob, native = make_prob(4), prob_native()
    cov = np.diag([20.0] * 4 + [100.0] * 4).astype(F32)
    try:
        model, tk = prob.world_model(route, 5, goal, P, cov)
        w = native.World(tk, model, 4)
        per = lambda a, n=E: np.tile(np.asarray(a)[None], (n, 1))
        rt = lambda n=E: (per(traffic["s"], n), per(traffic["v"], n),
                          np.stack([per(traffic["d"], n), per(traffic["v0"], n)], -1))
        st = lambda n=E: (np.zeros((n, 2)), np.zeros((n, 3)), None, np.zeros((n, 8)), cov, None, np.arange(n))
        w.route_vehicles(*rt())   # the reset's vehicles may be None from here on
        w.reset(*st())
        w.route_vehicles(*rt())   # a new policy: the next run needs a reset
        with pytest.raises(native.NativeError, match="before mpcmmd_world_reset"):
            w.run("cvar", 0, 1, cov, 10.0)
        with pytest.raises(native.NativeError, match="n_episodes is not the one"):
            w.reset(*st(2))
        with pytest.raises(native.NativeError, match="n_episodes"):
            w.route_vehicles(*rt(E + 1))
        for bad in (dict(acc_max=0.0), dict(brake=-1.0), dict(gap_min=0.0), dict(acc_min=0.0), dict(lane_tol=-1.0)):
            with pytest.raises(native.NativeError, match="acc_max > 0"):
                w.route_vehicles(*rt(), **bad)
        L, dp, fp = native.lib(), C.POINTER(C.c_double), C.POINTER(C.c_float)
        s, v, p = (np.ascontiguousarray(a) for a in rt())
        sc = native.routed_scalars({})
        ptr = lambda a, t: a.ctypes.data_as(t)
        assert L.mpcmmd_world_route_vehicles(w._w, E, ptr(s, dp), None, ptr(p, fp), ptr(sc, fp)) == -1
        assert L.mpcmmd_world_route_vehicles(w._w, E, ptr(s, dp), ptr(v, fp), ptr(p, fp), None) == -1
        w.route_vehicles(*rt())
        w.reset(*st())
        with pytest.raises(native.NativeError, match="tick range"):
            w.vehicle_log(5)
        assert L.mpcmmd_world_vehicle_log(w._w, 1, None, None) == -1
        assert w.vehicle_log(0).shape == (0, E, 5, 3)
        w.close()
    finally:
        prob.close()
