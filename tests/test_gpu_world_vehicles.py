"""The routed instantiation of k_world_step on the GPU
(mpcmmd_world_step_device_routed: one launch, a workgroup per episode, wave 0 a
lane per vehicle) against mpcmmd_world_step_host_routed: every word the step
writes -- the vehicles' states and log, their rows, the ego's state, the next
tick's inputs, the first population and the log row -- is bit-equal.  Three
episodes per launch, one of them frozen, and the same states through a
reset-mode launch; total_obs 0 / 1 / 5 / 64, a 37-point arc, the 130-point
hairpin and the 21 k-point synthetic route, both noise kinds, given and drawn
variates; then the constructed tie, lane-edge, parked, NaN and past-the-end
cases of test_world_vehicles_host.py in one launch.  The host step itself is
held against the NumPy restatement there."""
import math

import numpy as np
import pytest

import world_model as wm
import world_vehicle_model as vm
from world_vehicle_model import routed, straight_route, traffic

pytestmark = pytest.mark.gpu

F32 = np.float32
KEYS = ("pos", "ego", "vehicles", "done_tick", "init_state", "x_wp", "y_wp", "obstacles", "pop", "log_d", "log_f",
        "log_i", "veh_s", "veh_v", "veh_log")
PLAN = ("cx", "cy", "steer", "u", "mean", "pos", "ego", "done_tick")
# route, total_obs, noise, drawn variates
CASES = [("arc37", 0, "gaussian", False), ("arc37", 5, "beta", True), ("hairpin", 1, "beta", False),
         ("hairpin", 5, "gaussian", True), ("hairpin", 64, "beta", True), ("hairpin", 64, "gaussian", False),
         ("synthetic", 5, "gaussian", False)]


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def routes():
    syn, len_path = wm.synthetic_route()
    hp, _ = wm.hairpin_route()
    th = np.linspace(0.0, np.pi / 2, 37)   # a quarter circle of radius 60 m: num_route 37
    arc37 = wm.route_splines(60.0 * np.sin(th), 60.0 * (1.0 - np.cos(th)))
    return dict(synthetic=(syn, len_path - 1), hairpin=(hp, 129), arc37=(arc37, 36))


@pytest.fixture(scope="module")
def pdot4(native):
    cfg = native.make_config(4, 2, 0.1, 8, "gaussian", 0.0, 0.0, num_batch=20, variant="carla_town05", maxiter_cem=3)
    return native.host_constant(cfg, "Pdot").reshape(-1, 11)[:4]


def step(native, model, tick, ins, rt, device, keys=None):
    plan = {k: ins[k] for k in PLAN}
    if keys is not None:
        plan["u"] = None
    return native.world_step(model, tick, vehicles=None, device=device, routed=rt, keys=keys, **plan)


def compare(got, want):
    for k in KEYS:
        for e in range(got[k].shape[0]):
            assert same(got[k][e], want[k][e]), (k, e, got[k][e], want[k][e])


@pytest.mark.parametrize("route,total,noise,drawn", CASES)
def test_device_step_equals_host_step(native, routes, pdot4, route, total, noise, drawn):
    r, goal = routes[route]
    w = wm.small_world(r, goal, num_path=37, num_obs=2, total_obs=total, noise=noise, B=20, seed=total + 1)
    model = wm.native_model(native, w, pdot4, seed=13)
    rng = np.random.default_rng(31 + total)
    E = 3
    ins = wm.random_inputs(rng, w, E)
    ins["done_tick"][1] = 2
    s, v, param = traffic(rng, w, ins, E)
    if total >= 5:   # an exact tie of two candidates and a parked vehicle in every episode
        s[:, 1] = s[:, 2] = s[:, 0] + 12.0
        param[:, :3, 0] = (0.0, 0.5, -0.5)
        param[:, 3, 1] = 0.0
    rt = routed(s, v, param, vm.scalars())
    keys = 100000 * np.arange(E) + 7 if drawn else None
    want = step(native, model, 5, ins, rt, None, keys)
    got = step(native, model, 5, ins, rt, 0, keys)
    compare(got, want)
    # the launch is what it claims, on the host's answers
    assert same(want["veh_s"][1], s[1]) and same(want["pos"][1], ins["pos"][1]), "episode 1 is frozen"
    assert not same(want["pos"][0], ins["pos"][0])
    if total:
        moving = param[0, :, 1] > 0
        assert (want["veh_s"][0][moving] >= s[0][moving]).all() and not same(want["veh_s"][0], s[0])
        assert np.abs(np.hypot(want["vehicles"][0, :, 2], want["vehicles"][0, :, 3]) - want["veh_v"][0]).max() < 1e-5
    if drawn:
        assert np.unique(want["log_f"][:, 9]).size == E
    # the reset-mode launch of the same states
    want = step(native, model, -1, ins, rt, None, keys)
    got = step(native, model, -1, ins, rt, 0, keys)
    compare(got, want)
    assert same(want["veh_s"], s) and same(want["pos"], ins["pos"]) and not want["log_f"].any()


def _quiet(x, y, v_ego=0.0):
    return dict(cx=np.zeros((1, 11), F32), cy=np.zeros((1, 11), F32), steer=np.zeros((1, 4), F32),
                u=np.zeros((1, 4), F32), mean=np.zeros((1, 8), F32), pos=np.array([[x, y]], float),
                ego=np.array([[v_ego, 0.0, 0.0]], F32), done_tick=np.full(1, -1, np.int32))


def test_constructed_cases(native, pdot4):
    """One launch, an episode per case, on a straight route (x = s, y = d); V = 4."""
    nan = math.nan
    far, near = (700.0, 30.0), (120.0, 0.25)
    cases = [  # name, ego, s, v, d, v0
        ("tie", far, [100.0, 120.0, 120.0, 300.0], [8.0, 1.0, 6.0, 0.0], [0.0, 0.5, -0.5, 30.0], [9.0, 9.0, 9.0, 0.0]),
        ("tie_swapped", far, [100.0, 120.0, 120.0, 300.0], [8.0, 6.0, 1.0, 0.0], [0.0, 0.5, -0.5, 30.0], [9.0, 9.0, 9.0, 0.0]),
        ("ego_tie", near, [100.0, 120.0, 300.0, 310.0], [8.0, 5.0, 0.0, 0.0], [0.0, -1.0, 30.0, 30.0], [9.0, 0.0, 0.0, 0.0]),
        ("ego_alone", near, [100.0, 120.0, 300.0, 310.0], [8.0, 5.0, 0.0, 0.0], [0.0, 30.0, 30.0, 30.0], [9.0, 0.0, 0.0, 0.0]),
        ("lane_edge", far, [100.0, 120.0, 300.0, 310.0], [8.0, 1.0, 0.0, 0.0], [0.0, 1.75, 30.0, 30.0], [9.0, 0.0, 0.0, 0.0]),
        ("gap_min", far, [100.0, 102.0, 300.0, 305.0], [8.0, 1.0, 0.0, 0.0], [0.0, 0.0, 30.0, 30.0], [9.0, 0.0, 9.0, 0.0]),
        ("parked", far, [100.0, 200.0, 300.0, 80.0], [3.0, 4.0, 5.0, 6.0], [0.0, 0.0, 0.0, 0.0], [0.0, -2.0, nan, 9.0]),
        ("nan_s", far, [100.0, nan, 300.0, 80.0], [3.0, 4.0, 5.0, 6.0], [0.0, 0.0, 0.0, 0.0], [9.0, 9.0, 9.0, 9.0]),
        ("nan_d_v", far, [100.0, 120.0, 300.0, 80.0], [3.0, nan, 5.0, 6.0], [0.0, 0.0, nan, 0.0], [9.0, 9.0, 9.0, 9.0]),
        ("past_the_end", far, [900.0, -50.0, 797.9, 80.0], [5.0, 5.0, 5.0, 6.0], [1.0, 1.0, 1.0, 0.0], [9.0, 9.0, 9.0, 9.0]),
    ]
    w = wm.small_world(straight_route(), 399, num_path=37, num_obs=2, total_obs=4, B=20, sigma_acc=F32(0.0),
                       sigma_steer=F32(0.0), acc_const=F32(0.0), steer_const=F32(0.0), y_lb=F32(-100.0),
                       y_ub=F32(100.0))
    model = wm.native_model(native, w, pdot4)
    each = [_quiet(*c[1]) for c in cases]
    ins = {k: np.concatenate([q[k] for q in each]) for k in PLAN}
    s = np.array([c[2] for c in cases])
    v = np.array([c[3] for c in cases], F32)
    param = np.stack([np.array([c[4] for c in cases], F32), np.array([c[5] for c in cases], F32)], -1)
    sc = vm.scalars()
    rt = routed(s, v, param, sc)
    want = step(native, model, 3, ins, rt, None)
    got = step(native, model, 3, ins, rt, 0)
    compare(got, want)
    # the cases are what they claim, on the host's answers
    a = {c[0]: want["veh_log"][i, :, 1] for i, c in enumerate(cases)}
    acc = lambda vl, v=8, gap=15.5: vm.accel(sc, F32(v), F32(9), None if vl is None else (gap, F32(vl)))
    assert same(a["tie"][0], acc(1.0)) and same(a["tie_swapped"][0], acc(6.0)) and not same(acc(1.0), acc(6.0))
    assert same(a["ego_tie"][0], acc(5.0)) and same(a["ego_alone"][0], acc(0.0))
    assert same(a["lane_edge"][0], acc(None)) and a["gap_min"][0] == sc["acc_min"]
    i = [c[0] for c in cases].index("parked")
    assert not want["veh_v"][i, :3].any() and same(a["parked"][3], acc(3.0, v=6))
    i = [c[0] for c in cases].index("nan_s")
    assert (want["vehicles"][i, 1].view(np.uint32) == 0x7FC00000).all() and want["done_tick"][i] == 3
    assert want["veh_s"][i, 1:2].view(np.uint64)[0] == 0x7FF8000000000000
    i = [c[0] for c in cases].index("past_the_end")
    assert want["veh_s"][i, 2] > 798.0 and np.allclose(want["vehicles"][i, :3, 0], want["veh_s"][i, :3])


def test_device_argument_errors(native, pdot4):
    """The checks come before any HIP call; a device that does not exist."""
    hp, _ = wm.hairpin_route()
    w = wm.small_world(hp, 129, total_obs=2)
    model = wm.native_model(native, w, pdot4)
    ins = wm.random_inputs(np.random.default_rng(0), w, 1)
    good = routed(np.zeros((1, 2)), np.zeros((1, 2), F32), np.ones((1, 2, 2), F32), vm.scalars())
    with pytest.raises(native.NativeError):
        step(native, model, 0, ins, good, 4096)
    with pytest.raises(native.NativeError, match="acc_max > 0"):
        step(native, model, 0, ins, dict(good, brake=0.0), 0)
