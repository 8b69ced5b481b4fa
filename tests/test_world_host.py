"""The surrogate world without a GPU: mpcmmd_world_step_host against the NumPy
restatement (tests/world_model.py) bit for bit, its waypoints against SciPy's
CubicSpline and the drop-in's waypoint_generator, its obstacles against
replay.nearest_obstacles, known answers, the argument errors and the sanitizer
run of the host code (tests/native/asan_world.cpp).  Floats are compared by
their bit patterns."""
import ctypes as C
import importlib
import importlib.util
import math
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import world_model as wm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mpc-mmd_amd")
F32 = np.float32
KEYS = ("pos", "ego", "vehicles", "done_tick", "init_state", "x_wp", "y_wp", "obstacles", "pop", "log_d", "log_f",
        "log_i")


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


def test_symbols():
    n = native_mod()
    for s in ("mpcmmd_world_step_host", "mpcmmd_world_step_device", "mpcmmd_world_create", "mpcmmd_world_destroy",
              "mpcmmd_world_reset", "mpcmmd_world_run", "mpcmmd_world_log"):
        assert s in n.SYMBOLS and hasattr(n.lib(), s), s
    assert n.lib().mpcmmd_abi_version() == n.ABI_VERSION


@pytest.mark.parametrize("route,noise,E", [("synthetic", "gaussian", 150), ("synthetic", "beta", 150),
                                           ("hairpin", "gaussian", 60)])
def test_host_step_equals_model(routes, route, noise, E):
    """Every output of E random states, bit for bit (300 states over the two noise kinds, 60
    more on the hairpin); a fifth of the episodes frozen."""
    n = native_mod()
    r, goal = routes[route]
    w = wm.small_world(r, goal, noise=noise, total_obs=5, num_obs=3, seed=3)
    model = wm.native_model(n, w, pdot4())
    rng = np.random.default_rng(11)
    ins = wm.random_inputs(rng, w, E)
    ins["done_tick"][::5] = 2
    got = n.world_step(model, 7, device=None, **ins)
    moved = 0
    for e in range(E):
        want = wm.step(w, 7, *(ins[k][e] for k in ("cx", "cy", "steer", "u", "mean", "pos", "ego", "vehicles",
                                                   "done_tick")))
        for k in KEYS:
            assert same(got[k][e], np.asarray(want[k])), (e, k, got[k][e], want[k])
        moved += int(not same(got["pos"][e], ins["pos"][e]))
    assert moved == E - len(range(0, E, 5)), "every running episode moves, no frozen one does"
    assert len({int(i) for i in got["log_i"][:, 0]}) > E // 4, "the states are spread over the route"


@pytest.mark.parametrize("noise", ["gaussian", "beta"])
def test_drawn_variates(routes, noise):
    """u = None: the library draws the variates from (key, seed, tick) once a_c and s_c are known.
    Against the oracle's Philox restatement: the normals bit for bit; the Beta draws within 2 fp32
    ulp (both sides evaluate Ga / (Ga + Gb) in fp64, by different formulas, to ~1e-13 relative, far
    below the fp32 ulp of 6e-8, so the rounded values are equal or adjacent; measured here: 0 ulp
    apart is the rule, 1 the exception).  The rest of the step, restated with the logged
    variates, is bit-equal.  Then the keys: another key, seed or tick gives other variates, the
    same triple the same; and a given u overrides the draw."""
    n = native_mod()
    r, goal = routes["hairpin"]
    w = wm.small_world(r, goal, noise=noise, total_obs=3, num_obs=2, seed=5)
    E, seed, tick = 40, 7, 11
    model = wm.native_model(n, w, pdot4(), seed=seed)
    ins = wm.random_inputs(np.random.default_rng(4), w, E)
    ins["cx"][0] = ins["cy"][0] = 0.0   # |a_c| = |s_c| = 0 exactly: the alpha -> 0+ limit of the Beta draw
    ins["steer"][0] = 0.0
    ins["ego"][0, 0] = 0.0
    given = ins.pop("u")
    keys = np.arange(E) * 100000 + 3
    got = n.world_step(model, tick, u=None, keys=keys, **ins)
    worst = 0
    for e in range(E):
        a_c, s_c = wm.controller(w, w["pdot4"], ins["cx"][e], ins["cy"][e], ins["steer"][e], F32(ins["ego"][e, 0]))
        assert same(got["log_f"][e, 3:5], np.array([a_c, s_c], F32)), e
        want_u = wm.draw(noise, keys[e], seed, tick, a_c, s_c)
        u = got["log_f"][e, 7:11]
        assert same(u[2:], want_u[2:]), e
        if noise == "gaussian":
            assert same(u, want_u), e
        else:
            assert ((u[:2] >= 0) & (u[:2] <= 1)).all()
            apart = np.abs(u[:2].view(np.int32).astype(np.int64) - want_u[:2].view(np.int32))
            worst = max(worst, int(apart.max()))
        want = wm.step(w, tick, ins["cx"][e], ins["cy"][e], ins["steer"][e], u, ins["mean"][e], ins["pos"][e],
                       ins["ego"][e], ins["vehicles"][e], ins["done_tick"][e])
        for k in KEYS:
            assert same(got[k][e], np.asarray(want[k])), (e, k)
    print(f"{noise}: Beta draws at most {worst} fp32 ulp from the oracle's")
    assert worst <= 2
    if noise == "beta":
        assert got["log_f"][0, 3] == 0 and got["log_f"][0, 4] == 0 and set(got["log_f"][0, 7:9]) <= {0.0, 1.0}
    u0 = got["log_f"][:, 7:11]
    again = n.world_step(model, tick, u=None, keys=keys, **ins)["log_f"][:, 7:11]
    assert same(again, u0)
    other_key = n.world_step(model, tick, u=None, keys=keys + 1, **ins)["log_f"][:, 7:11]
    other_tick = n.world_step(model, tick + 1, u=None, keys=keys, **ins)["log_f"][:, 7:11]
    other_seed = n.world_step(wm.native_model(n, w, pdot4(), seed=seed + 1), tick, u=None, keys=keys,
                              **ins)["log_f"][:, 7:11]
    for other in (other_key, other_tick, other_seed):
        assert (other[:, 2] != u0[:, 2]).all()
    assert len({float(x) for x in u0[:, 2]}) == E, "every episode its own normals"
    over = n.world_step(model, tick, u=given, keys=keys, **ins)
    assert same(over["log_f"][:, 7:11], given)
    with pytest.raises(ValueError):
        n.world_step(model, tick, u=None, **ins)


def _dropin_helper():
    name = "mpcmmd_carla_optimizer"
    if name not in sys.modules:
        d = os.path.join(PKG, "carla", "optimizer")
        spec = importlib.util.spec_from_file_location(name, os.path.join(d, "__init__.py"),
                                                      submodule_search_locations=[d])
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
    return importlib.import_module(name + ".cem_helper").Helper(num_prime=60)


def test_waypoints_against_scipy_and_dropin(routes):
    """600 waypoints at 40 ego positions along the synthetic route.  The restatement's fp64 spline
    values against SciPy's CubicSpline: the same term order, so the measured difference on this
    machine is 0 ulp; asserted within 4 ulp of the coordinate magnitude (|x| <= 5400 m: 3.6e-12).
    The host step's fp32 waypoints against the drop-in's waypoint_generator, shifted and cast as
    replay.tick_raw_inputs does: equal except where the fp64 values straddle a rounding boundary,
    at most 1 in 10^4 (measured: 0 of 48000)."""
    from scipy.interpolate import CubicSpline
    n = native_mod()
    (rx, ry, arc, sx, sy), goal = routes["synthetic"]
    h = _dropin_helper()
    h.num_path = 600
    csx, csy, csphi, length, arc_vec = h.path_spline(rx, ry)
    assert same(arc_vec, arc) and same(np.ascontiguousarray(csx.c), sx)
    w = wm.small_world(routes["synthetic"][0], goal, num_path=600, total_obs=0)
    model = wm.native_model(n, w, pdot4())
    rng = np.random.default_rng(5)
    E = 40
    ins = wm.random_inputs(rng, w, E)
    ins["done_tick"][:] = 0   # frozen: the waypoints are those of the given position
    got = n.world_step(model, 0, device=None, **ins)
    diff_ulp, mismatch, total = 0.0, 0, 0
    for e in range(E):
        x, y = ins["pos"][e]
        wx, wy, _ = h.waypoint_generator(x, y, rx, ry, arc_vec, csx, csy, csphi, length)
        i = int(got["log_i"][e, 0])
        assert arc[i] == arc_vec[int(np.argmin(np.sqrt((x - rx) ** 2 + (y - ry) ** 2)))]
        look = np.linspace(arc[i], arc[i] + 300.0, 600)
        for mine, ref, c0 in ((wm.spline_values(arc, sx, look), wx, x), (wm.spline_values(arc, sy, look), wy, y)):
            diff_ulp = max(diff_ulp, float(np.max(np.abs(mine - ref) / np.spacing(np.maximum(np.abs(ref), 1.0)))))
        for mine, ref, c0 in ((got["x_wp"][e], wx, x), (got["y_wp"][e], wy, y)):
            mismatch += int(np.sum(mine.view(np.uint32) != (ref - c0).astype(F32).view(np.uint32)))
            total += mine.size
    print(f"fp64 spline difference {diff_ulp} ulp; fp32 waypoints differing {mismatch} of {total}")
    assert diff_ulp <= 4.0
    assert mismatch * 10 ** 4 <= total
    assert CubicSpline(arc, rx)(arc[5] + 0.1) == wm.spline_values(arc, sx, np.array([arc[5] + 0.1]))[0]


def _threshold_dot():
    """A double d with acos(d) == 5 pi / 6 exactly, and its neighbour below (a larger angle)."""
    T = 5 * np.pi / 6
    d = math.cos(T)
    for _ in range(64):
        if math.acos(d) == T:
            break
        d = np.nextafter(d, 0.0 if math.acos(d) > T else -1.0)
    assert math.acos(d) == T
    lo = d
    while math.acos(lo) == T:
        lo = np.nextafter(lo, -1.0)
    return float(d), float(lo)


def _obstacle_cases(O):
    """(name, ego (x, y, v, psi), vehicles [T, 5]) -- the ego heads along +x."""
    z = lambda rows: np.array([[x, y, 0.5, -0.25, 0.1 * i] for i, (x, y) in enumerate(rows)], F32)
    d_at, d_below = _threshold_dot()
    return (
        ("none_kept", (10.0, 2.0, 5.0, 0.0), z([(0.0, 2.0), (-20.0, 1.0), (5.0, 3.0)])),
        ("fewer_than_num_obs", (10.0, 2.0, 5.0, 0.0), z([(0.0, 2.0), (40.0, 1.0), (5.0, 3.0), (25.0, -3.0)])),
        ("more_than_num_obs", (10.0, 2.0, 5.0, 0.0), z([(60.0, 2.0), (40.0, 1.0), (15.0, 3.0), (25.0, -3.0),
                                                        (90.0, 0.0), (12.0, 2.0)])),
        # four vehicles at the bit-equal squared distance 25, in an order that is not the sorted one
        ("distance_ties", (10.0, 2.0, 5.0, 0.0), z([(14.0, 5.0), (13.0, 6.0), (30.0, 2.0), (13.0, -2.0), (15.0, 2.0),
                                                    (14.0, -1.0)])),
        # v = 1, heading 0: the dot product is the x offset itself
        ("at_threshold", (-d_at, 0.0, 1.0, 0.0), z([(0.0, 0.5), (3.0, 0.0)])),
        ("past_threshold", (-d_below, 0.0, 1.0, 0.0), z([(0.0, 0.5), (3.0, 0.0)])),
    )


@pytest.mark.parametrize("O", [3, 5])
def test_obstacles_against_replay(routes, O):
    n = native_mod()
    R = wm.replay()
    kept_counts = {}
    for name, (x, y, v, psi), veh in _obstacle_cases(O):
        w = wm.small_world(routes["hairpin"][0], 129, num_obs=O, total_obs=veh.shape[0])
        model = wm.native_model(n, w, pdot4())
        ins = wm.random_inputs(np.random.default_rng(1), w, 1)
        ins.update(pos=np.array([[x, y]]), ego=np.array([[v, psi, 0.0]], F32), vehicles=veh[None],
                   done_tick=np.zeros(1, np.int32))   # frozen: nothing moves
        got = n.world_step(model, 0, device=None, **ins)
        ego = np.array([x, y, v, 0.0, psi, 0.0])
        want = R.nearest_obstacles(veh, ego, O).copy()
        want[:, 0] = (want[:, 0].astype(np.float64) - x).astype(F32)
        want[:, 1] = (want[:, 1].astype(np.float64) - y).astype(F32)
        assert same(got["obstacles"][0], want), (name, got["obstacles"][0], want)
        rel = veh[:, :2].astype(np.float64) - [x, y]
        kept_counts[name] = sum(math.acos(min(max(r * v, -1.0), 1.0)) <= 5 * np.pi / 6 for r in rel[:, 0])
    assert kept_counts["none_kept"] == 0 and 0 < kept_counts["fewer_than_num_obs"] < 3
    assert kept_counts["more_than_num_obs"] > 5
    assert kept_counts["at_threshold"] == 2 and kept_counts["past_threshold"] == 1


def _still(w, x, y, v=0.0, psi=0.0, **over):
    """Inputs of one episode whose plan asks for speed v and zero steering."""
    ins = dict(cx=np.zeros((1, 11), F32), cy=np.zeros((1, 11), F32), steer=np.zeros((1, 4), F32),
               u=np.zeros((1, 4), F32), mean=np.zeros((1, 8), F32), pos=np.array([[x, y]], float),
               ego=np.array([[v, psi, 0.0]], F32), vehicles=np.full((1, w["total_obs"], 5), 1e4, F32),
               done_tick=np.full(1, -1, np.int32))
    ins.update(over)
    return ins


def test_known_answers(routes):
    n = native_mod()
    (syn, goal) = routes["synthetic"]
    w = wm.small_world(syn, goal, total_obs=1, num_obs=2, steer_const=F32(0.0))
    model = wm.native_model(n, w, pdot4())
    rng = np.random.default_rng(2)
    # zero steer on the straight: y and psi bit-still over 50 ticks, x advances
    st = _still(w, 3.0, 0.25, v=4.0, u=rng.standard_normal((1, 4)).astype(F32))
    st["cx"][0, :] = np.linspace(0, 60, 11)   # some positive plan speed
    x0 = st["pos"][0, 0]
    for k in range(50):
        out = n.world_step(model, k, device=None, **st)
        st.update(pos=out["pos"], ego=out["ego"], vehicles=out["vehicles"], done_tick=out["done_tick"])
    assert same(out["pos"][0, 1], np.float64(0.25)) and same(out["ego"][0, 1], F32(0.0)) and out["pos"][0, 0] > x0 + 1
    assert abs(out["log_f"][0, 12] - 0.25) < 1e-6 and not out["log_i"][0, 1:].any() and out["done_tick"][0] == -1
    # v never goes negative: a plan speed of 0 from v = 0.5 asks for a = -1.1 m/s^2 ... times 20 by the noise
    w2 = wm.small_world(syn, goal, total_obs=1, num_obs=2, sigma_acc=F32(40.0))
    m2 = wm.native_model(n, w2, pdot4())
    st = _still(w2, 3.0, 0.0, v=0.5, u=np.array([[-1.0, 0, 0, 0]], F32))
    out = n.world_step(m2, 0, device=None, **st)
    assert out["log_f"][0, 5] < -10 and same(out["ego"][0, 0], F32(0.0)) and same(out["pos"], st["pos"])
    # a vehicle on the ego: collided, and the episode is done at this tick
    st = _still(w, 30.0, 0.0)
    st["vehicles"][0, 0] = [30.5, 0.5, 0, 0, 0.3]
    out = n.world_step(model, 4, device=None, **st)
    assert out["log_i"][0, 2] == 1 and out["log_f"][0, 11] > 0 and out["done_tick"][0] == 4
    # ... and a frozen episode's state does not change, whatever the plan asks
    st.update(pos=out["pos"], ego=out["ego"], vehicles=out["vehicles"], done_tick=out["done_tick"])
    st["cx"][0, :] = np.linspace(0, 90, 11)
    st["vehicles"][0, 0, 2:4] = [3.0, 1.0]
    nxt = n.world_step(model, 5, device=None, **st)
    for k in ("pos", "ego", "vehicles", "done_tick"):
        assert same(nxt[k], st[k]), k
    assert same(nxt["x_wp"], out["x_wp"]) and same(nxt["init_state"], out["init_state"])
    # the goal flag flips at 7 m from route point goal_index
    gx, gy = syn[0][goal], syn[1][goal]
    for dist, flag in ((6.999, 1), (7.001, 0)):
        out = n.world_step(model, 9, device=None, **_still(w, gx, gy - dist))
        assert out["log_i"][0, 3] == flag and out["done_tick"][0] == (9 if flag else -1), dist


def test_argument_errors():
    n = native_mod()
    L = n.lib()
    assert L.mpcmmd_world_step_host(None, 0, None) == -1 and L.mpcmmd_last_error()
    assert L.mpcmmd_world_step_device(None, 0, 1, 0, None) == -1
    hp, _ = wm.hairpin_route()
    for key, bad in (("num_path", 1), ("num_path", 2049), ("num_obs", 0), ("num_obs", 65), ("total_obs", 65),
                     ("goal_index", 130), ("noise", 2), ("num_batch", 0)):
        w = wm.small_world(hp, 129)
        model = wm.native_model(n, w, pdot4())
        setattr(model.c, key, bad)
        io = n.WorldStepIO()
        assert L.mpcmmd_world_step_host(C.byref(model.c), 0, C.byref(io)) == -1, key
        assert L.mpcmmd_world_step_device(C.byref(model.c), 0, 1, 0, C.byref(io)) == -1, key
    out = C.c_void_p()
    assert L.mpcmmd_world_create(None, C.byref(model.c), 4, C.byref(out)) == -1 and not out.value
    assert L.mpcmmd_world_reset(None, 1, None, None, None, None, None, None, None) == -1
    assert L.mpcmmd_world_run(None, 2, 0, 1, None, None, 0.1) == -1
    assert L.mpcmmd_world_log(None, 1, None, None, None, None, None) == -1
    L.mpcmmd_world_destroy(None)
    model = wm.native_model(n, wm.small_world(hp, 129), pdot4())
    assert L.mpcmmd_world_step_host(C.byref(model.c), 0, C.byref(n.WorldStepIO())) == -1
    assert b"null array" in L.mpcmmd_last_error()


def test_world_program_under_sanitizers():
    """`make asan_world` builds tests/native/asan_world.cpp with the host-only sources under ASan /
    UBSan (-fno-sanitize-recover); its run, a child process with nothing preloaded, must exit 0 with
    no sanitizer report, and the checksums it prints must be those of the library's host step on the
    same inputs."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    subprocess.run(["make", "-C", PKG, "asan_world"], check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(PKG, "build_asan", "asan_world")], capture_output=True, text=True, env=env,
                       timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "ok"
    # the program's world, restated here: a straight route of 40 points, 3 vehicles, 5 ticks
    n = native_mod()
    rx = np.arange(40) * 2.0
    sx = np.zeros((4, 39))   # the spline pieces of a straight line: x = arc, y = 0
    sx[2], sx[3] = 1.0, rx[:-1]
    route = (rx, np.zeros(40), rx.copy(), sx, np.zeros((4, 39)))
    w = wm.small_world(route, 39, num_path=5, num_obs=2, total_obs=3, B=4)
    w["cov"] = np.diag([4.0] * 8).astype(F32)
    w["pop0"] = (np.arange(32, dtype=F32).reshape(4, 8) - 16) / 8
    pd = np.zeros((4, 11))
    pd[:, 1] = 1.0
    model = wm.native_model(n, w, pd)
    st = dict(cx=np.zeros((1, 11), F32), cy=np.zeros((1, 11), F32), steer=np.full((1, 4), 0.05, F32),
              u=np.array([[0.5, -0.25, 1.0, -1.0]], F32), mean=np.arange(8, dtype=F32)[None] + 1,
              pos=np.array([[1.0, 0.5]]), ego=np.array([[2.0, 0.1, 0.0]], F32),
              vehicles=np.array([[[20, 1, -1, 0, 0.2], [-10, 0, 0, 0, 0], [30, -2, 0, 0.5, 3.0]]], F32),
              done_tick=np.full(1, -1, np.int32))
    st["cx"][0, 1] = 6.0
    for k in range(5):
        out = n.world_step(model, k, device=None, **st)
        st.update(pos=out["pos"], ego=out["ego"], vehicles=out["vehicles"], done_tick=out["done_tick"])
        words = np.concatenate([out[key].reshape(-1).view(np.uint32) for key in
                                ("init_state", "x_wp", "y_wp", "obstacles", "pop", "log_f")])
        want = f"tick {k} {int(words.astype(np.uint64).sum() & 0xFFFFFFFF):08x} {out['pos'][0, 0]!r} {int(out['log_i'][0, 0])}"
        got = lines[k].split()
        assert got[:3] == want.split()[:3] and float(got[3]) == out["pos"][0, 0] and int(got[4]) == out["log_i"][0, 0], \
            (lines[k], want)
