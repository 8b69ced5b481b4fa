"""The surrogate world's routed vehicles without a GPU:
mpcmmd_world_step_host_routed against the NumPy restatement
(tests/world_vehicle_model.py) in every word it writes, the constructed edge
cases of the leader rule, the parked / NaN / past-the-end vehicles, frozen and
reset steps, known answers of the car-following model on the restatement and
on the host, the argument errors, and the sanitizer run of the host code
(tests/native/asan_world_vehicles.cpp).  Floats are compared by their bits."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import world_model as wm
import world_vehicle_model as vm
from world_vehicle_model import routed, straight_route, traffic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mpc-mmd_amd")
F32 = np.float32
KEYS = ("pos", "ego", "vehicles", "done_tick", "init_state", "x_wp", "y_wp", "obstacles", "pop", "log_d", "log_f",
        "log_i", "veh_s", "veh_v", "veh_log")
PLAN = ("cx", "cy", "steer", "u", "mean", "pos", "ego", "done_tick")


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def native_mod():
    from optimizer import _native
    return _native


def pdot4():
    n = native_mod()
    cfg = n.make_config(4, 2, 0.1, 8, "gaussian", 0.0, 0.0, num_batch=20, variant="carla_town05", maxiter_cem=3)
    return n.host_constant(cfg, "Pdot").reshape(-1, 11)[:4]


@pytest.fixture(scope="module")
def routes():
    syn, len_path = wm.synthetic_route()
    hp, _ = wm.hairpin_route()
    return dict(synthetic=(syn, len_path - 1), hairpin=(hp, 129))


def host(n, model, tick, ins, rt):
    return n.world_step(model, tick, vehicles=None, device=None, routed=rt, **{k: ins[k] for k in PLAN})


def check_all(got, w, sc, tick, ins, s, v, param, episodes=None):
    E = got["pos"].shape[0]
    for e in (range(E) if episodes is None else episodes):
        want = vm.step(w, sc, tick, *(ins[k][e] for k in PLAN), s[e], v[e], param[e])
        for k in KEYS:
            assert same(got[k][e], np.asarray(want[k])), (e, k, got[k][e], want[k])


def test_symbols():
    n = native_mod()
    for s in ("mpcmmd_world_step_host_routed", "mpcmmd_world_step_device_routed", "mpcmmd_world_route_vehicles",
              "mpcmmd_world_vehicle_log"):
        assert s in n.SYMBOLS and hasattr(n.lib(), s), s
    assert n.lib().mpcmmd_abi_version() == n.ABI_VERSION
    assert {k: float(F32(x)) for k, x in n.ROUTED_DEFAULTS.items()} == {k: float(x) for k, x in vm.scalars().items()}
    assert n.ROUTED_SCALARS == vm.SCALARS


@pytest.mark.parametrize("route,noise,E,V", [("synthetic", "gaussian", 120, 5), ("synthetic", "beta", 120, 5),
                                             ("hairpin", "gaussian", 60, 7)])
def test_host_step_equals_model(routes, route, noise, E, V):
    """Every word of E random states (300 in all), a fifth of the episodes frozen; then the same states
    through the reset-mode step."""
    n = native_mod()
    r, goal = routes[route]
    w = wm.small_world(r, goal, noise=noise, total_obs=V, num_obs=3, seed=3)
    model = wm.native_model(n, w, pdot4())
    rng = np.random.default_rng(21)
    ins = wm.random_inputs(rng, w, E)
    ins["done_tick"][::5] = 2
    s, v, param = traffic(rng, w, ins, E)
    sc = vm.scalars()
    got = host(n, model, 7, ins, routed(s, v, param, sc))
    check_all(got, w, sc, 7, ins, s, v, param)
    live = ins["done_tick"] < 0
    moving = live[:, None] & (param[..., 1] > 0)
    assert (got["veh_s"][moving] >= s[moving]).all() and (got["veh_s"][moving] > s[moving]).sum() > moving.sum() // 2
    assert same(got["veh_s"][~live], s[~live]) and same(got["veh_v"][~live], v[~live])
    assert (got["veh_log"][..., 1] < 0).sum() > 10 and (got["veh_log"][..., 1] > 0).sum() > 10, "both signs occur"
    rs = host(n, model, -1, ins, routed(s, v, param, sc))
    check_all(rs, w, sc, -1, ins, s, v, param, range(0, E, 7))
    assert same(rs["veh_s"], s) and same(rs["veh_v"], v) and same(rs["done_tick"], ins["done_tick"])
    assert same(rs["pos"], ins["pos"]) and not rs["veh_log"].any()


def _quiet(w, x, y, V, v_ego=0.0):
    """One live episode whose ego stands at (x, y) and stays (zero plan, zero variates)."""
    return dict(cx=np.zeros((1, 11), F32), cy=np.zeros((1, 11), F32), steer=np.zeros((1, 4), F32),
                u=np.zeros((1, 4), F32), mean=np.zeros((1, 8), F32), pos=np.array([[x, y]], float),
                ego=np.array([[v_ego, 0.0, 0.0]], F32), done_tick=np.full(1, -1, np.int32))


def _straight_world(V, **over):
    n = native_mod()
    w = wm.small_world(straight_route(), 399, num_path=5, num_obs=2, total_obs=V, B=4, sigma_acc=F32(0.0),
                       sigma_steer=F32(0.0), acc_const=F32(0.0), steer_const=F32(0.0), y_lb=F32(-100.0),
                       y_ub=F32(100.0), **over)
    return n, w, wm.native_model(n, w, pdot4())


def _one(n, model, w, sc, ins, s, v, d, v0, tick=3):
    s = np.asarray(s, np.float64)[None]
    v = np.asarray(v, F32)[None]
    param = np.stack([np.asarray(d, F32), np.asarray(v0, F32)], -1)[None]
    got = host(n, model, tick, ins, routed(s, v, param, sc))
    check_all(got, w, sc, tick, ins, s, v, param)
    return got


def test_leader_rule_cases():
    """The constructed cases of the leader rule on a straight route (x = s, d = y); each equals the
    restatement in every word and is shown to discriminate."""
    sc = vm.scalars()
    n, w, model = _straight_world(3)
    far = _quiet(w, 700.0, 30.0, 3)   # the ego out of everybody's lane
    # two candidates at bit-equal gaps with different speeds: the lower index leads
    got = _one(n, model, w, sc, far, [100.0, 120.0, 120.0], [8.0, 1.0, 6.0], [0.0, 0.5, -0.5], [9.0, 9.0, 9.0])
    a = got["veh_log"][0, 0, 1]
    assert same(a, vm.accel(sc, F32(8), F32(9), (120.0 - 100.0 - 4.5, F32(1.0))))
    assert not same(a, vm.accel(sc, F32(8), F32(9), (120.0 - 100.0 - 4.5, F32(6.0))))
    got = _one(n, model, w, sc, far, [100.0, 120.0, 120.0], [8.0, 6.0, 1.0], [0.0, 0.5, -0.5], [9.0, 9.0, 9.0])
    assert same(got["veh_log"][0, 0, 1], vm.accel(sc, F32(8), F32(9), (15.5, F32(6.0))))
    # a vehicle and the ego at bit-equal gaps: the vehicle leads (the ego comes last)
    near = _quiet(w, 120.0, 0.25, 3, v_ego=0.0)   # stands at route point 60: s = 120, d = 0.25
    got = _one(n, model, w, sc, near, [100.0, 120.0, 300.0], [8.0, 5.0, 0.0], [0.0, 30.0, 30.0], [9.0, 0.0, 0.0])
    assert got["log_d"][0, 2] == 120.0 and got["log_f"][0, 12] == 0.25
    assert same(got["veh_log"][0, 0, 1], vm.accel(sc, F32(8), F32(9), (15.5, F32(0.0)))), "alone, the ego leads"
    got = _one(n, model, w, sc, near, [100.0, 120.0, 300.0], [8.0, 5.0, 0.0], [0.0, -1.0, 30.0], [9.0, 0.0, 0.0])
    assert same(got["veh_log"][0, 0, 1], vm.accel(sc, F32(8), F32(9), (15.5, F32(5.0))))
    assert not same(got["veh_log"][0, 0, 1], vm.accel(sc, F32(8), F32(9), (15.5, F32(0.0))))
    # exactly lane_tol away: excluded by <; one fp32 step nearer: the leader
    free = vm.accel(sc, F32(8), F32(9), None)
    got = _one(n, model, w, sc, far, [100.0, 120.0, 300.0], [8.0, 1.0, 0.0], [0.0, 1.75, 30.0], [9.0, 0.0, 0.0])
    assert same(got["veh_log"][0, 0, 1], free)
    got = _one(n, model, w, sc, far, [100.0, 120.0, 300.0], [8.0, 1.0, 0.0],
               [0.0, np.nextafter(F32(1.75), F32(0)), 30.0], [9.0, 0.0, 0.0])
    assert not same(got["veh_log"][0, 0, 1], free)
    # the same s is nobody's leader (s_k > s_j is strict); lane_tol = 0 excludes even d_k == d_j
    got = _one(n, model, w, sc, far, [100.0, 100.0, 300.0], [8.0, 1.0, 0.0], [0.0, 0.0, 30.0], [9.0, 9.0, 0.0])
    assert same(got["veh_log"][0, 0, 1], free)
    sc0 = vm.scalars(lane_tol=0.0)
    got = _one(n, model, w, sc0, far, [100.0, 110.0, 300.0], [8.0, 1.0, 0.0], [0.0, 0.0, 30.0], [9.0, 9.0, 0.0])
    assert same(got["veh_log"][0, 0, 1], free)
    # gap <= gap_min (overlapping bumpers, gap -2.5): the interaction uses gap_min, the clip gives acc_min
    got = _one(n, model, w, sc, far, [100.0, 102.0, 300.0], [8.0, 1.0, 0.0], [0.0, 0.0, 30.0], [9.0, 0.0, 0.0])
    assert got["veh_log"][0, 0, 1] == sc["acc_min"]
    got = _one(n, model, w, sc, far, [100.0, 105.0, 300.0], [0.0, 0.0, 0.0], [0.0, 0.0, 30.0], [9.0, 0.0, 0.0])
    want = F32(max(1.5 * (1.0 - (5.0 / 0.5) * (5.0 / 0.5)), -8.0))
    assert same(got["veh_log"][0, 0, 1], want) and got["veh_v"][0, 0] == 0.0, "gap 0.5 == gap_min, v stays 0"


def test_parked_nan_and_past_the_end(routes):
    sc = vm.scalars()
    n, w, model = _straight_world(4)
    far = _quiet(w, 700.0, 30.0, 4)
    # v0 = 0, v0 < 0, NaN v0: parked, whatever v was; the fourth follows the first
    got = _one(n, model, w, sc, far, [100.0, 200.0, 300.0, 80.0], [3.0, 4.0, 5.0, 6.0], [0.0, 0.0, 0.0, 0.0],
               [0.0, -2.0, np.nan, 9.0])
    assert same(got["veh_v"][0, :3], np.zeros(3, F32)) and same(got["veh_s"][0, :3], np.array([100.0, 200.0, 300.0]))
    assert same(got["vehicles"][0, 0], np.array([100.0, 0.0, 0.0, 0.0, 0.0], F32)) and not got["veh_log"][0, :3, 1].any()
    assert same(got["veh_log"][0, 3, 1], vm.accel(sc, F32(6), F32(9), (15.5, F32(3.0)))), "the leader's speed before"
    # beyond the last breakpoint (798): the last piece extrapolates, x = s
    got = _one(n, model, w, sc, far, [900.0, -50.0, 797.9, 80.0], [5.0, 5.0, 5.0, 6.0], [1.0, 1.0, 1.0, 0.0],
               [9.0, 9.0, 9.0, 9.0])
    assert np.allclose(got["vehicles"][0, :3, 0], got["veh_s"][0, :3]) and (got["vehicles"][0, :3, 1] == 1.0).all()
    assert got["veh_s"][0, 2] > 798.0
    # a NaN s: its row is the quiet NaN, the episode collides, nobody else is affected
    base = _one(n, model, w, sc, far, [100.0, 120.0, 300.0, 80.0], [3.0, 4.0, 5.0, 6.0], [0.0, 0.0, 0.0, 0.0],
                [9.0, 9.0, 9.0, 9.0])
    got = _one(n, model, w, sc, far, [100.0, np.nan, 300.0, 80.0], [3.0, 4.0, 5.0, 6.0], [0.0, 0.0, 0.0, 0.0],
               [9.0, 9.0, 9.0, 9.0])
    assert (got["vehicles"][0, 1].view(np.uint32) == 0x7FC00000).all()
    assert got["veh_s"][0:1, 1].view(np.uint64)[0] == 0x7FF8000000000000
    assert got["log_i"][0, 2] == 1 and got["done_tick"][0] == 3 and np.isnan(got["log_f"][0, 11])
    for j in (2, 3):
        assert same(got["vehicles"][0, j], base["vehicles"][0, j]) and same(got["veh_log"][0, j], base["veh_log"][0, j])
    assert same(got["veh_log"][0, 0, 1], vm.accel(sc, F32(3), F32(9), (300.0 - 100.0 - 4.5, F32(5.0)))), \
        "vehicle 0 looks past the NaN vehicle"
    # NaN d and NaN v likewise equal the restatement
    _one(n, model, w, sc, far, [100.0, 120.0, 300.0, 80.0], [3.0, np.nan, 5.0, 6.0], [0.0, 0.0, np.nan, 0.0],
         [9.0, 9.0, 9.0, 9.0])
    # on the curved routes: s before the first and past the last breakpoint, beside vehicles inside
    for name in ("hairpin", "synthetic"):
        r, goal = routes[name]
        wc = wm.small_world(r, goal, total_obs=4, num_obs=2)
        mc = wm.native_model(n, wc, pdot4())
        ins = _quiet(wc, r[0][5], r[1][5] + 0.5, 4)
        end = r[2][-1]
        _one(n, mc, wc, sc, ins, [end + 25.0, -10.0, end, r[2][3] + 0.1], [5.0, 5.0, 5.0, 2.0], [0.5, -0.5, 0.0, 0.0],
             [9.0, 9.0, 9.0, 9.0])


@pytest.mark.parametrize("V", [0, 64])
def test_total_obs_edges(routes, V):
    n = native_mod()
    r, goal = routes["hairpin"]
    w = wm.small_world(r, goal, total_obs=V, num_obs=3, seed=4)
    model = wm.native_model(n, w, pdot4())
    rng = np.random.default_rng(5)
    ins = wm.random_inputs(rng, w, 6)
    s, v, param = traffic(rng, w, ins, 6)
    sc = vm.scalars()
    got = host(n, model, 2, ins, routed(s, v, param, sc))
    check_all(got, w, sc, 2, ins, s, v, param)
    assert got["vehicles"].shape == (6, V, 5)
    if V == 0:
        assert (got["log_f"][:, 11] == -np.inf).all() and (got["obstacles"][:, :, 0] != 0).all()


def test_frozen_and_reset_rewrite_the_same_rows(routes):
    """A frozen step and a reset-mode step keep S and write the rows a live step left, bit for bit."""
    n = native_mod()
    r, goal = routes["hairpin"]
    w = wm.small_world(r, goal, total_obs=5, num_obs=3, seed=6)
    model = wm.native_model(n, w, pdot4())
    rng = np.random.default_rng(8)
    ins = wm.random_inputs(rng, w, 4)
    s, v, param = traffic(rng, w, ins, 4)
    sc = vm.scalars()
    live = host(n, model, 0, ins, routed(s, v, param, sc))
    nxt = dict(ins, pos=live["pos"], ego=live["ego"], done_tick=np.zeros(4, np.int32))
    for tick in (1, -1):
        again = host(n, model, tick, nxt, routed(live["veh_s"], live["veh_v"], param, sc))
        assert same(again["vehicles"], live["vehicles"]) and same(again["veh_s"], live["veh_s"])
        assert same(again["veh_v"], live["veh_v"]) and same(again["obstacles"], live["obstacles"])
        assert same(again["x_wp"], live["x_wp"]) and not again["veh_log"][..., 1].any()
    assert not again["log_f"].any() and not again["log_i"].any(), "the reset-mode step writes no log row"


def test_pose_interpolates_the_knots(routes):
    """pose(arc[i], 0, v) is exactly (float(route_x[i]), float(route_y[i])): a spline interpolates its knots."""
    n = native_mod()
    sc = vm.scalars()
    for name in ("hairpin", "synthetic"):
        r, goal = routes[name]
        rx, ry, arc = r[0], r[1], r[2]
        idx = np.unique(np.linspace(0, arc.size - 2, 64).astype(int))
        w = wm.small_world(r, goal, total_obs=idx.size, num_obs=2)
        model = wm.native_model(n, w, pdot4())
        for j, i in enumerate(idx):
            row = vm.pose(w, arc[i], 0.0, 2.0)
            assert same(row[:2], np.array([rx[i], ry[i]]).astype(F32)), (name, i)
        ins = _quiet(w, rx[0], ry[0], idx.size)
        ins["done_tick"][:] = 0
        s, v = arc[idx][None], np.full((1, idx.size), 2.0, F32)
        param = np.stack([np.zeros(idx.size, F32), np.full(idx.size, 5.0, F32)], -1)[None]
        got = host(n, model, 0, ins, routed(s, v, param, sc))
        assert same(got["vehicles"][0, :, 0], rx[idx].astype(F32)) and same(got["vehicles"][0, :, 1], ry[idx].astype(F32))
        speed = np.hypot(got["vehicles"][0, :, 2].astype(float), got["vehicles"][0, :, 3])
        assert np.abs(speed - 2.0).max() < 1e-6


# ---- known answers: conditions on the restatement, then the same on the host step -----------------

def _model_run(sc, s, v, v0, ticks, dt=F32(0.05)):
    """The restatement's leader / advance over `ticks` ticks of vehicles on one lane; the state per tick."""
    s, v = np.array(s, np.float64), np.array(v, F32)
    d = np.zeros(s.size, F32)
    hist = []
    for _ in range(ticks):
        lead = [vm.leader(sc, j, s, d, v, (math.nan, math.nan, 0.0)) for j in range(s.size)]
        new = [vm.advance(sc, dt, s[j], v[j], v0[j], lead[j]) for j in range(s.size)]
        s, v = np.array([x[0] for x in new]), np.array([x[1] for x in new], F32)
        hist.append((s.copy(), v.copy()))
    return hist


def _host_run(s, v, v0, ticks):
    sc = vm.scalars()
    V = len(s)
    n, w, model = _straight_world(V)
    ins = _quiet(w, 780.0, 60.0, V)
    s, v = np.array(s, np.float64)[None], np.array(v, F32)[None]
    param = np.stack([np.zeros(V, F32), np.asarray(v0, F32)], -1)[None]
    hist = []
    for k in range(ticks):
        out = host(n, model, k, ins, routed(s, v, param, sc))
        assert out["done_tick"][0] == -1
        s, v = out["veh_s"], out["veh_v"]
        hist.append((s[0].copy(), v[0].copy()))
    return hist


def _runs(s, v, v0, ticks):
    m, h = _model_run(vm.scalars(), s, v, v0, ticks), _host_run(s, v, v0, ticks)
    for (ms, mv), (hs, hv) in zip(m, h):
        assert same(ms, hs) and same(mv, hv), "the host run is the restatement's, tick by tick"
    return h


def test_free_vehicle_reaches_its_target_speed():
    hist = _runs([10.0], [0.0], [5.0], 2000)
    v = float(hist[-1][1][0])
    print("free vehicle after 2000 ticks:", v)
    assert abs(v - 5.0) <= 1e-4 * 5.0
    assert all(b[1][0] >= a[1][0] for a, b in zip(hist, hist[1:])), "it never slows down"


@pytest.mark.parametrize("behind", [60.0, 20.0, 8.0])
def test_stops_behind_a_parked_vehicle(behind):
    """`behind` is the bumper gap at the start (4.33, 4.33 and 4.13 m are left at the end)."""
    hist = _runs([100.0 - 4.5 - behind, 100.0], [5.0, 0.0], [5.0, 0.0], 2000)
    gaps = np.array([s[1] - s[0] - 4.5 for s, _ in hist])
    print(f"{behind} m behind: final gap {gaps[-1]:.4f} m, smallest {gaps.min():.4f} m")
    assert same(hist[-1][1][0], F32(0.0)) and 4.0 < gaps[-1] <= 5.0 and gaps.min() > 0.0


def test_follower_settles_at_the_equilibrium_gap():
    sc = vm.scalars()
    # the leader holds 3 m/s exactly: v = v0 = 3 on a free road gives free = 0 and a = 0
    hist = _runs([50.0, 80.0], [3.0, 3.0], [5.0, 3.0], 3000)
    s, v = hist[-1]
    gap = s[1] - s[0] - 4.5
    want = (5.0 + 3.0 * 1.0) / math.sqrt(1.0 - (3.0 / 5.0) ** 4)
    print(f"follower: v {v[0]:.5f} m/s behind {v[1]:.5f}, gap {gap:.4f} m, equilibrium {want:.4f} m")
    assert same(v[1], F32(3.0)) and abs(float(v[0]) - 3.0) < 1e-3 and abs(gap - want) <= 0.01 * want
    assert abs(want - 8.575) < 1e-3 and float(sc["gap0"]) == 5.0


# ---- argument errors and the sanitizer run -----------------------------------------------------------

def test_argument_errors():
    n = native_mod()
    L = n.lib()
    hp, _ = wm.hairpin_route()
    w = wm.small_world(hp, 129, total_obs=2)
    model = wm.native_model(n, w, pdot4())
    ins = wm.random_inputs(np.random.default_rng(0), w, 1)
    good = routed(np.zeros((1, 2)), np.zeros((1, 2), F32), np.ones((1, 2, 2), F32), vm.scalars())
    assert host(n, model, 0, ins, good)["vehicles"].shape == (1, 2, 5)
    a = dict(s=np.zeros(2), v=np.zeros(2, F32), p=np.ones(4, F32), log=np.zeros(4, F32))
    ptr = lambda x, t: x.ctypes.data_as(C.POINTER(t))

    def rt(drop=None, **over):
        sc = [float(dict(vm.DEFAULTS, **over)[k]) for k in vm.SCALARS]
        arr = [None if drop == "s" else ptr(a["s"], C.c_double), None if drop == "v" else ptr(a["v"], C.c_float),
               None if drop == "p" else ptr(a["p"], C.c_float), ptr(a["log"], C.c_float)]
        return n.WorldRouted(*arr, *sc)

    io_keep = []

    def io():
        full = n.world_step(model, 0, device=None, **ins)   # arrays of the right sizes to point at
        arrs = dict(ins, **full)
        arrs["key"] = np.zeros(1, np.uint32)
        io_keep.append(arrs)
        f = dict(n.WorldStepIO._fields_)
        return n.WorldStepIO(*[C.cast(np.ascontiguousarray(arrs[k]).ctypes.data, f[k]) for k in f])

    for k in list(ins):
        ins[k] = np.ascontiguousarray(ins[k])
    the_io = io()
    call = lambda r: (L.mpcmmd_world_step_host_routed(C.byref(model.c), 0, C.byref(the_io), r),
                      L.mpcmmd_world_step_device_routed(C.byref(model.c), 0, 1, 0, C.byref(the_io), r))
    assert L.mpcmmd_world_step_host_routed(C.byref(model.c), 0, C.byref(the_io), C.byref(rt())) == 0
    assert call(None) == (-1, -1) and b"null" in L.mpcmmd_last_error()
    for drop in ("s", "v", "p"):
        assert call(C.byref(rt(drop=drop))) == (-1, -1), drop
        assert b"null array" in L.mpcmmd_last_error()
    for key, bad in (("acc_max", 0.0), ("acc_max", -1.0), ("acc_max", math.nan), ("brake", 0.0), ("brake", math.nan),
                     ("gap_min", 0.0), ("gap_min", math.nan), ("acc_min", 0.0), ("acc_min", 1.0),
                     ("acc_min", math.nan), ("lane_tol", -0.5), ("lane_tol", math.nan)):
        assert call(C.byref(rt(**{key: bad}))) == (-1, -1), (key, bad)
        assert b"acc_max > 0" in L.mpcmmd_last_error()
    assert L.mpcmmd_world_step_host_routed(C.byref(model.c), 0, C.byref(the_io), C.byref(rt(lane_tol=0.0))) == 0
    # the plain step's errors still come first; a world without vehicles takes NULL arrays
    assert L.mpcmmd_world_step_host_routed(None, 0, None, C.byref(rt())) == -1
    assert L.mpcmmd_world_step_device_routed(C.byref(model.c), 0, 0, 0, C.byref(the_io), C.byref(rt())) == -1
    model.c.total_obs = 0
    sc = [float(vm.DEFAULTS[k]) for k in vm.SCALARS]
    assert L.mpcmmd_world_step_host_routed(C.byref(model.c), 0, C.byref(the_io),
                                           C.byref(n.WorldRouted(None, None, None, None, *sc))) == 0
    # the context's entry points
    assert L.mpcmmd_world_route_vehicles(None, 1, None, None, None, None) == -1
    assert L.mpcmmd_world_vehicle_log(None, 1, None, None) == -1
    with pytest.raises(ValueError):
        n.routed_scalars(dict(headroom=1.0))


def test_vehicles_program_under_sanitizers():
    """`make asan_world_vehicles` builds tests/native/asan_world_vehicles.cpp with the host-only sources
    under ASan / UBSan (-fno-sanitize-recover); its run, a child process with nothing preloaded, must exit
    0 with no sanitizer report, and the checksums it prints must be those of the library's host step on the
    same inputs."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    subprocess.run(["make", "-C", PKG, "asan_world_vehicles"], check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(PKG, "build_asan", "asan_world_vehicles")], capture_output=True, text=True,
                       env=env, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "ok"
    # the program's world, restated here: a straight route of 40 points, 6 vehicles, the reset-mode step and 9 ticks
    n = native_mod()
    w = wm.small_world(straight_route(40), 39, num_path=5, num_obs=2, total_obs=6, B=4)
    w["cov"] = np.diag([4.0] * 8).astype(F32)
    w["pop0"] = (np.arange(32, dtype=F32).reshape(4, 8) - 16) / 8
    pd = np.zeros((4, 11))
    pd[:, 1] = 1.0
    model = wm.native_model(n, w, pd)
    st = dict(cx=np.zeros((1, 11), F32), cy=np.zeros((1, 11), F32), steer=np.full((1, 4), 0.05, F32),
              u=np.array([[0.5, -0.25, 1.0, -1.0]], F32), mean=np.arange(8, dtype=F32)[None] + 1,
              pos=np.array([[1.0, 0.5]]), ego=np.array([[2.0, 0.1, 0.0]], F32), done_tick=np.full(1, -1, np.int32))
    st["cx"][0, 1] = 6.0
    s = np.array([[20.0, 30.0, 30.0, 50.0, 95.0, -4.0]])
    v = np.array([[4.0, 1.0, 3.0, 2.0, 5.0, 6.0]], F32)
    param = np.array([[[0.0, 6.0], [0.5, 0.0], [-0.5, 5.0], [0.0, 5.0], [1.75, 7.0], [0.0, math.nan]]], F32)
    sc = vm.scalars()
    for k in range(-1, 9):
        if k == 8:
            s[0, 3] = math.nan
        out = host(n, model, k, st, routed(s, v, param, sc))
        st.update(pos=out["pos"], ego=out["ego"], done_tick=out["done_tick"])
        s, v = out["veh_s"], out["veh_v"]
        words = np.concatenate([out[key].reshape(-1).view(np.uint32) for key in
                                ("init_state", "x_wp", "y_wp", "obstacles", "pop", "log_f", "vehicles", "veh_v",
                                 "veh_log")] + [out["veh_s"].reshape(-1).view(np.uint32)])
        want = f"tick {k} {int(words.astype(np.uint64).sum() & 0xFFFFFFFF):08x} {int(out['done_tick'][0])}"
        assert lines[k + 1] == want, (lines[k + 1], want)
    assert out["done_tick"][0] == 8
