"""The planned vehicles of the synthetic closed loop without a GPU:
mpcmmd_mpc_step_host_planned against the NumPy restatement (tests/mpc_vehicle_model.py) on every
output word, its tracks against mpcmmd_obs_dynamic_traj and the sweep's generator, the QP against
an LU solve of its full KKT system, the known answers, the argument errors, the NaN rule and the
sanitizer run of the host code (tests/native/asan_mpc_vehicles.cpp).  Floats are compared by
their bit patterns unless a tolerance is named."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import mpc_vehicle_model as vm
import mpc_world_model as mm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mpc-mmd_amd")
F32 = np.float32
KEYS = ("pos", "vel", "vehicles", "done_tick", "init_state", "st0", "x_obs", "y_obs", "pop", "log_d", "log_f", "log_i",
        "veh_acc", "veh_log")
NEW = ("mpcmmd_mpc_vehicle_constant", "mpcmmd_mpc_step_host_planned", "mpcmmd_mpc_step_device_planned",
       "mpcmmd_mpc_plan_vehicles", "mpcmmd_mpc_vehicle_log")
INVALID = -1


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def nat():
    from optimizer import _native
    for s in NEW:   # a library without the entry points fails every test of this file
        assert s in _native.SYMBOLS and hasattr(_native.lib(), s), s
    return _native


def planned_inputs(rng, w, E):
    """Random states with accelerations |ax| <= 2, |ay| <= 1 and per-vehicle targets."""
    O = w["num_obs"]
    ins = mm.random_inputs(rng, w, E)
    acc = np.stack([rng.uniform(-2, 2, (E, O)), rng.uniform(-1, 1, (E, O))], 2).astype(F32)
    target = np.stack([rng.normal(6, 0.5, (E, O)), rng.choice([-1.75, 1.75, 0.3], (E, O))], 2).astype(F32)
    return ins, acc, target


def test_symbols():
    n = nat()
    assert n.lib().mpcmmd_abi_version() == n.ABI_VERSION == 5, "the ABI version is unchanged"


def test_constants():
    n = nat()
    K = vm.constants(n, 0.15)
    x0, y0, vx0, vy0, vd = [20.0], [1.75], [2.0], [0.0], [6.0]
    # the QP's arrays are those mpcmmd_obs_dynamic_traj solves with: its tracks from them, bit for bit
    xt, yt = n.obs_dynamic_traj(x0, y0, vx0, vy0, vd)
    cxf, cyf = vm.plan(K, [[20.0, 1.75, 2.0, 0.0, 0.0, 0.0]], [[6.0, -1.75]])
    assert same(vm.track(K, cxf), xt) and same(vm.track(K, cyf), yt)
    # adv: the basis rows at double(float32(dt)), rounded to fp32 and widened
    from oracle.problem import bernstein_order10
    for dt in (0.15, 0.1, 7.5):
        t = float(F32(dt))
        want = np.stack([m[0] for m in bernstein_order10(0.0, 15.0, np.array([t]))]).astype(F32).astype(np.float64)
        assert same(n.mpc_vehicle_constant(dt, "adv").reshape(3, 11), want), dt
    assert same(n.mpc_vehicle_constant(0.1, "P"), K["P"].ravel())


@pytest.mark.parametrize("num_obs,E", [(1, 12), (3, 12), (64, 4)])
@pytest.mark.parametrize("tick", [-1, 7])
def test_host_step_equals_model(num_obs, E, tick):
    """The frozen step (tick = -1, as the host-linked route makes tick 0's inputs) and a live step
    with every third episode frozen: every output word, nonzero accelerations, per-vehicle y_des."""
    n = nat()
    w, model = mm.small_model(n, noise="gaussian", num_obs=num_obs, variant="dynamic")
    K = vm.constants(n, w["dt"])
    ins, acc, target = planned_inputs(np.random.default_rng(5 + num_obs), w, E)
    if tick < 0:
        ins["done_tick"][:] = 0
    else:
        ins["done_tick"][::3] = 2
    got = n.mpc_step(model, tick, device=None, planned=dict(acc=acc, target=target), **ins)
    for e in range(E):
        want = vm.step(K, w, tick, ins["cx"][e], ins["cy"][e], ins["u"][e], ins["mean"][e], ins["pos"][e],
                       ins["vel"][e], ins["vehicles"][e], ins["done_tick"][e], acc[e], target[e])
        for k in KEYS:
            assert same(got[k][e], np.asarray(want[k])), (e, k, got[k][e].ravel()[:6], np.asarray(want[k]).ravel()[:6])
    frozen = ins["done_tick"] >= 0
    assert same(got["vehicles"][frozen], ins["vehicles"][frozen]) and same(got["veh_acc"][frozen], acc[frozen])
    if (~frozen).any():
        assert not same(got["vehicles"][~frozen], ins["vehicles"][~frozen])
    assert same(got["veh_log"][..., :4], got["vehicles"]) and same(got["veh_log"][..., 4:], got["veh_acc"])


def test_tracks_with_zero_acceleration():
    """veh_acc = 0 and one y_des: the frozen step's tracks are mpcmmd_obs_dynamic_traj's of the same
    states; for the CLI's scenario they are the sweep generator's."""
    n = nat()
    O, E = 5, 3
    w, model = mm.small_model(n, num_obs=O, variant="dynamic")
    ins, _, target = planned_inputs(np.random.default_rng(8), w, E)
    target[..., 1] = -1.75
    ins["done_tick"][:] = 0
    got = n.mpc_step(model, -1, device=None, planned=dict(acc=None, target=target), **ins)
    for e in range(E):
        v = ins["vehicles"][e]
        xt, yt = n.obs_dynamic_traj(v[:, 0], v[:, 1], v[:, 2], v[:, 3], target[e, :, 0], -1.75)
        assert same(got["x_obs"][e], xt) and same(got["y_obs"][e], yt), e
    from optimizer import closed_loop as cl
    from optimizer.sweep import obstacles
    veh, _ = cl.scenario("dynamic", E, O)
    tg = cl.vehicle_targets(E, O)
    ins["vehicles"] = veh
    got = n.mpc_step(model, -1, device=None, planned=dict(acc=None, target=tg), **ins)
    for e in range(E):
        ob = obstacles("dynamic", e, O)
        assert same(got["x_obs"][e], ob["x_traj"]) and same(got["y_obs"][e], ob["y_traj"]), e


def test_qp_against_lu():
    """The once-inverted KKT route against an LU solve of the full system with nonzero ax, ay:
    rtol = 1e-5, atol = 1e-4, the tolerance of tests/test_dynamic_obstacles.py."""
    n = nat()
    K = vm.constants(n, 0.15)
    rng = np.random.default_rng(21)
    O = 40
    S = np.stack([rng.uniform(0, 80, O), rng.uniform(-3, 3, O), rng.uniform(0.5, 8, O), rng.uniform(-0.5, 0.5, O),
                  rng.uniform(-2, 2, O), rng.uniform(-1, 1, O)], 1).astype(F32)
    tg = np.stack([rng.normal(6, 0.3, O), rng.choice([-1.75, 1.75], O)], 1).astype(F32)
    cxf, cyf = vm.plan(K, S, tg)
    rx, ry = vm.lu_tracks(S, tg)
    np.testing.assert_allclose(vm.track(K, cxf), rx, rtol=1e-5, atol=1e-4)
    np.testing.assert_allclose(vm.track(K, cyf), ry, rtol=1e-5, atol=1e-4)
    # and the library's own step forms the same tracks as the restatement (O = 40 in one episode)
    w, model = mm.small_model(n, num_obs=O, variant="dynamic")
    ins = mm.random_inputs(rng, w, 1)
    ins["done_tick"][:] = 0
    ins["vehicles"][0] = S[:, :4]
    got = n.mpc_step(model, -1, device=None, planned=dict(acc=S[None, :, 4:], target=tg[None]), **ins)
    assert same(got["x_obs"][0], vm.track(K, cxf)) and same(got["y_obs"][0], vm.track(K, cyf))


def run_vehicle(n, S0, target, steps, dt=0.15):
    """`steps` live host steps of one vehicle beside a far-away ego: S [steps, 6]."""
    w, model = mm.small_model(n, num_obs=1, variant="dynamic", dt=dt, goal_x=1e9)
    ins = mm.random_inputs(np.random.default_rng(1), w, 1)
    ins["pos"][:] = [-1e4, 0.0]
    ins["u"][:] = 0
    veh, acc = np.array([[S0[:4]]], F32), np.array([[S0[4:]]], F32)
    pos, vel, done = ins["pos"], ins["vel"], ins["done_tick"]
    log = []
    for k in range(steps):
        st = n.mpc_step(model, k, ins["cx"], ins["cy"], ins["u"], ins["mean"], pos, vel, veh, done, device=None,
                        planned=dict(acc=acc, target=[[target]]))
        assert st["done_tick"][0] == -1
        pos, vel, veh, acc = st["pos"], st["vel"], st["vehicles"], st["veh_acc"]
        log.append(st["veh_log"][0, 0].copy())
    return np.array(log)


def test_known_answers():
    n = nat()
    # on its target: constant speed in its lane (the tolerances of tests/test_dynamic_obstacles.py)
    S = run_vehicle(n, [10.0, -1.75, 6.0, 0.0, 0.0, 0.0], (6.0, -1.75), 20)
    want = 10.0 + 6.0 * np.float64(F32(0.15)) * np.arange(1, 21)
    assert (np.abs(S[:, 0] - want) <= 1e-3 + 1e-5 * np.abs(want)).all(), np.abs(S[:, 0] - want).max()
    assert (np.abs(S[:, 1] + 1.75) <= 1e-4).all(), np.abs(S[:, 1] + 1.75).max()
    # the cut-in: x strictly increasing, bounded accelerations, the target lane reached
    S = run_vehicle(n, [20.0, 1.75, 2.0, 0.0, 0.0, 0.0], (6.0, -1.75), 200)
    print(f"cut-in: max |ax| = {np.abs(S[:, 4]).max():.3f}, max |ay| = {np.abs(S[:, 5]).max():.3f}, "
          f"|y + 1.75| at the end = {abs(S[-1, 1] + 1.75):.2e}, y after 40 ticks = {S[39, 1]:.3f}")
    assert (np.diff(np.concatenate([[20.0], S[:, 0]])) > 0).all()
    assert np.abs(S[:, 4]).max() < 1 and np.abs(S[:, 5]).max() < 1
    assert abs(S[-1, 1] + 1.75) < 0.01


def test_errors():
    n = nat()
    L = n.lib()
    buf = (C.c_double * 1100)()
    for dt in (0.0, -0.15, 15.0, 20.0, float("nan")):
        assert L.mpcmmd_mpc_vehicle_constant(dt, b"adv", buf, 1100) == INVALID, dt
    assert L.mpcmmd_mpc_vehicle_constant(0.15, b"kinv_z", buf, 1100) == INVALID
    assert b"unknown" in L.mpcmmd_last_error()
    assert L.mpcmmd_mpc_vehicle_constant(0.15, b"P", buf, 1099) == INVALID
    assert L.mpcmmd_mpc_vehicle_constant(0.15, None, buf, 1100) == INVALID
    assert L.mpcmmd_mpc_vehicle_constant(0.15, b"P", None, 0) == 1100
    assert [L.mpcmmd_mpc_vehicle_constant(0.15, k.encode(), buf, 1100) for k in n.VEHICLE_CONSTANTS] == \
        [196, 225, 11, 11, 1100, 33]
    # the step: a NULL pl, a NULL array in pl, a tick length the basis does not cover
    w, model = mm.small_model(n, num_obs=2)
    ins = mm.random_inputs(np.random.default_rng(0), w, 1)
    a = dict(ins, init_state=np.empty((1, 6), F32), st0=np.empty((1, 8), F32), x_obs=np.empty((1, 2, 100), F32),
             y_obs=np.empty((1, 2, 100), F32), pop=np.empty((1, 20, 8), F32), log_d=np.empty((1, 2)),
             log_f=np.empty((1, 12), F32), log_i=np.empty((1, 4), np.int32), key=np.zeros(1, np.uint32))
    types = dict(n.MpcStepIO._fields_)
    io = n.MpcStepIO(*[C.cast(a[k].ctypes.data, types[k]) for k, _ in n.MpcStepIO._fields_])
    acc, tg, lg = np.zeros((2, 2), F32), np.ones((2, 2), F32), np.zeros((2, 6), F32)
    fp = n._fptr
    step = L.mpcmmd_mpc_step_host_planned
    assert step(C.byref(model.c), 0, C.byref(io), None) == INVALID
    assert step(C.byref(model.c), 0, C.byref(io), C.byref(n.MpcPlanned(None, fp(tg), fp(lg)))) == INVALID
    assert step(C.byref(model.c), 0, C.byref(io), C.byref(n.MpcPlanned(fp(acc), None, fp(lg)))) == INVALID
    assert step(C.byref(model.c), 0, None, C.byref(n.MpcPlanned(fp(acc), fp(tg), fp(lg)))) == INVALID
    # the device entry point refuses the same before any HIP call (no GPU here)
    dstep = L.mpcmmd_mpc_step_device_planned
    assert dstep(C.byref(model.c), 0, 1, 0, C.byref(io), None) == INVALID
    assert dstep(C.byref(model.c), 0, 1, 0, C.byref(io), C.byref(n.MpcPlanned(fp(acc), None, None))) == INVALID
    assert step(C.byref(model.c), 0, C.byref(io), C.byref(n.MpcPlanned(fp(acc), fp(tg), None))) == 0, "veh_log may be NULL"
    _, slow = mm.small_model(n, num_obs=2, dt=15.0)
    assert step(C.byref(slow.c), 0, C.byref(io), C.byref(n.MpcPlanned(fp(acc), fp(tg), fp(lg)))) == INVALID
    assert L.mpcmmd_mpc_plan_vehicles(None, 1, fp(tg), None) == INVALID
    assert L.mpcmmd_mpc_vehicle_log(None, 1, fp(lg)) == INVALID


@pytest.mark.parametrize("what", ["target", "state"])
def test_nan(what):
    """A NaN target (or state) makes that vehicle's tracks and state the quiet NaN 0x7FC00000 and
    sets collided; the other vehicle is untouched by it."""
    n = nat()
    w, model = mm.small_model(n, num_obs=2, variant="dynamic")
    K = vm.constants(n, w["dt"])
    ins, acc, target = planned_inputs(np.random.default_rng(3), w, 2)
    ins["vehicles"][:, :, 0] = ins["pos"][:, None, 0] + 500.0   # nobody near the ego
    ref = n.mpc_step(model, 4, device=None, planned=dict(acc=acc, target=target), **ins)
    assert not ref["log_i"][:, 1].any()
    if what == "target":
        target[0, 1, 0] = -np.float32(np.nan)   # any NaN: sign and payload do not survive
    else:
        ins["vehicles"][0, 1, 3] = np.nan
    got = n.mpc_step(model, 4, device=None, planned=dict(acc=acc, target=target), **ins)
    q = np.uint32(0x7FC00000)
    col = slice(0, None, 2) if what == "target" else slice(1, None, 2)   # a NaN v_des reaches x, a NaN vy reaches y
    assert (got["veh_log"][0, 1, col].view(np.uint32) == q).all(), got["veh_log"][0, 1]
    tr = got["x_obs" if what == "target" else "y_obs"][0, 1]
    assert (tr.view(np.uint32) == q).all()
    assert got["log_i"][0, 1] == 1 and got["done_tick"][0] == 4 and got["log_f"][0, 10].view(np.uint32) == q
    assert same(got["veh_log"][0, 0], ref["veh_log"][0, 0]) and same(got["x_obs"][0, 0], ref["x_obs"][0, 0])
    for k in ("veh_log", "x_obs", "y_obs", "log_i", "done_tick"):
        assert same(got[k][1], ref[k][1]), k
    want = vm.step(K, w, 4, ins["cx"][0], ins["cy"][0], ins["u"][0], ins["mean"][0], ins["pos"][0], ins["vel"][0],
                   ins["vehicles"][0], ins["done_tick"][0], acc[0], target[0])
    for k in KEYS:
        assert same(got[k][0], np.asarray(want[k])), k


def test_vehicle_program_under_sanitizers():
    """`make asan_mpc_vehicles` builds tests/native/asan_mpc_vehicles.cpp with the host-only sources
    under ASan / UBSan (-fno-sanitize-recover); its run, a child process with nothing preloaded, must
    exit 0 with no sanitizer report, and the checksums it prints must be those of the library's host
    step on the same inputs."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    n = nat()
    subprocess.run(["make", "-C", PKG, "asan_mpc_vehicles"], check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(PKG, "build_asan", "asan_mpc_vehicles")], capture_output=True, text=True, env=env,
                       timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "ok"
    # the program's scene, restated here: 3 vehicles cutting in, a population of 4, 5 chained ticks
    cfg = n.make_config(4, 3, 0.2, 8, "gaussian", 0.05, 0.01, num_batch=4, maxiter_cem=3)
    pop0 = ((np.arange(32, dtype=F32) - F32(16.0)) / F32(8.0)).reshape(4, 8)
    model = n.MpcModel(cfg, 4.0 * np.eye(8, dtype=F32), pop0, goal_x=1000.0, sigma_steer=0.1, K_steer=0.03,
                       y_lb=-5.25, y_ub=5.25)
    pd, pdd = np.zeros((2, 11)), np.zeros(11)
    pd[0, 1] = 1.0
    pd[1, 1], pd[1, 2] = 1.0, 0.01
    pdd[2] = 0.5
    model.arrays["pdot2"][:], model.arrays["pddot1"][:] = pd, pdd
    cx, cy = np.zeros((1, 11), F32), np.zeros((1, 11), F32)
    cx[0, 1], cx[0, 2], cy[0, 2] = 6.0, 40.0, 0.2
    pos, vel = np.array([[1.0, 0.5]]), np.array([[6.0, 0.1, 0.0]], F32)
    veh = np.array([[[40, 1.75, 2, 0], [-10, 1.75, 3, 0.1], [60, -1.75, 5, 0]]], F32)
    acc = np.array([[[0.5, -0.25], [0, 0], [-1, 0.125]]], F32)
    tg = np.array([[[6.0, -1.75], [5.5, -1.75], [6.25, 1.75]]], F32)
    done = np.array([-1], np.int32)
    ticks = [ln.split() for ln in lines if ln.startswith("tick ")]
    assert len(ticks) == 5
    for k, row in enumerate(ticks):
        st = n.mpc_step(model, k, cx, cy, np.array([[0.5, -0.25, 1.0]], F32), np.arange(1, 9, dtype=F32)[None], pos, vel,
                        veh, done, device=None, planned=dict(acc=acc, target=tg))
        pos, vel, veh, done, acc = st["pos"], st["vel"], st["vehicles"], st["done_tick"], st["veh_acc"]
        words = np.concatenate([st[name].ravel().view(np.uint32) for name in
                                ("init_state", "st0", "x_obs", "y_obs", "pop", "log_f", "vehicles", "veh_acc", "veh_log")])
        assert int(row[1]) == k and int(row[2], 16) == int(words.sum(dtype=np.uint64) & 0xFFFFFFFF), (k, row)
