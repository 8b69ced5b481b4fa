"""The synthetic closed loop's world without a GPU: mpcmmd_mpc_step_host against the NumPy
restatement (tests/mpc_world_model.py) on every output word, the drawn variates against the
oracle's Philox restatement, the edge cases of DESIGN.md section 21, the argument errors and the
sanitizer run of the host code (tests/native/asan_mpc.cpp).  Floats are compared by their bit
patterns."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import mpc_world_model as mm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mpc-mmd_amd")
F32 = np.float32
KEYS = ("pos", "vel", "vehicles", "done_tick", "init_state", "st0", "x_obs", "y_obs", "pop", "log_d", "log_f", "log_i")
ARGS = ("cx", "cy", "u", "mean", "pos", "vel", "vehicles", "done_tick")


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def native_mod():
    from optimizer import _native
    return _native


def check_all(got, w, tick, ins, E, u=None):
    for e in range(E):
        a = {k: ins[k][e] for k in ARGS if k != "u"}
        want = mm.step(w, tick, a["cx"], a["cy"], ins["u"][e] if u is None else u[e], a["mean"], a["pos"], a["vel"],
                       a["vehicles"], a["done_tick"])
        for k in KEYS:
            assert same(got[k][e], np.asarray(want[k])), (e, k, got[k][e], want[k])


def test_symbols():
    n = native_mod()
    for s in ("mpcmmd_mpc_step_host", "mpcmmd_mpc_step_device", "mpcmmd_mpc_create", "mpcmmd_mpc_destroy",
              "mpcmmd_mpc_reset", "mpcmmd_mpc_run", "mpcmmd_mpc_log", "mpcmmd_mpc_first_normals"):
        assert s in n.SYMBOLS and hasattr(n.lib(), s), s
    assert n.lib().mpcmmd_abi_version() == n.ABI_VERSION == 5


@pytest.mark.parametrize("noise,variant,E", [("gaussian", "static", 150), ("beta", "dynamic", 150)])
def test_host_step_equals_model(noise, variant, E):
    """Every output word of E random states (300 over the two noise kinds); a fifth of the
    episodes frozen."""
    n = native_mod()
    w, model = mm.small_model(n, noise=noise, num_obs=3, variant=variant)
    ins = mm.random_inputs(np.random.default_rng(11), w, E)
    ins["done_tick"][::5] = 2
    got = n.mpc_step(model, 7, device=None, **ins)
    check_all(got, w, 7, ins, E)
    moved = sum(int(not same(got["pos"][e], ins["pos"][e])) for e in range(E))
    assert moved == E - len(range(0, E, 5)), "every running episode moves, no frozen one does"
    assert (got["log_i"][::5, 3] == 1).all() and (got["log_i"][1::5, 3] == 0).all()
    # the heading of st0 is the host libm's atan2f of the new velocity, not a rounded fp64 value
    for e in range(E):
        assert same(got["st0"][e, 4], mm.atan2f(got["init_state"][e, 3], got["init_state"][e, 2]))
    assert w["y_lb"] < w["y_ub"] and w["K_steer"] > 0


def test_st0_heading_is_the_libm_atan2f():
    """initial_state (the host routes' st0) calls the libm's atan2f; the step restates that routine
    in fp32 so the kernel can form the same bits.  20000 velocities, among them vy = 0, vx = 1,
    negative vx and tiny ratios."""
    n = native_mod()
    w, model = mm.small_model(n, num_obs=0)
    rng = np.random.default_rng(3)
    E = 20000
    ins = mm.random_inputs(rng, w, E)
    ins["done_tick"][:] = 0   # frozen: st0 is that of the given velocity
    v = rng.uniform(-30, 30, (E, 2)).astype(F32)
    v[::7, 1] *= F32(1e-4)
    v[::11, 0] = 1.0
    v[::13, 1] = 0.0
    v[5::17, 0] = 0.0
    ins["vel"][:, :2] = v
    got = n.mpc_step(model, 0, device=None, **ins)
    for e in range(E):
        assert same(got["st0"][e, 4], mm.atan2f(v[e, 1], v[e, 0])), (e, v[e])


@pytest.mark.parametrize("noise", ["gaussian", "beta"])
def test_drawn_variates(noise):
    """u = None: the library draws the variates from (key, seed, tick) once a_c and s_c are known.
    The normals equal oracle/rng.py's Philox restatement bit for bit; the Beta draws lie within 2
    fp32 ulp of it (both sides evaluate Ga / (Ga + Gb) in fp64, by different formulas, to ~1e-13
    relative, far below the fp32 ulp of 6e-8, so the rounded values are equal or adjacent).  The
    rest of the step, restated with the logged variates, is bit-equal."""
    n = native_mod()
    E, seed, tick = 40, 7, 11
    w, model = mm.small_model(n, noise=noise, num_obs=2, seed=seed)
    ins = mm.random_inputs(np.random.default_rng(4), w, E)
    ins["cx"][0] = np.linspace(0, 60, 11)   # a straight plan at constant speed: a_c = s_c = 0 up to rounding
    ins["cy"][0] = 0.0
    given = ins.pop("u")
    keys = np.arange(E) * 100000 + 3
    got = n.mpc_step(model, tick, u=None, keys=keys, **ins)
    worst = 0
    for e in range(E):
        a_c, s_c, _ = mm.controller(w, ins["cx"][e], ins["cy"][e])
        assert same(got["log_f"][e, 3:5], np.array([a_c, s_c], F32)), e
        want_u = mm.draw(noise, keys[e], seed, tick, a_c, s_c)
        u = got["log_f"][e, 7:10]
        assert same(u[2:], want_u[2:]), e
        if noise == "gaussian":
            assert same(u, want_u), e
        else:
            assert ((u[:2] >= 0) & (u[:2] <= 1)).all()
            apart = np.abs(u[:2].view(np.int32).astype(np.int64) - want_u[:2].view(np.int32))
            worst = max(worst, int(apart.max()))
    print(f"{noise}: Beta draws at most {worst} fp32 ulp from the oracle's")
    assert worst <= 2
    ins["u"] = got["log_f"][:, 7:10].copy()
    check_all(got, w, tick, ins, E)
    del ins["u"]
    u0 = got["log_f"][:, 7:10]
    assert same(n.mpc_step(model, tick, u=None, keys=keys, **ins)["log_f"][:, 7:10], u0)
    other_key = n.mpc_step(model, tick, u=None, keys=keys + 1, **ins)["log_f"][:, 7:10]
    other_tick = n.mpc_step(model, tick + 1, u=None, keys=keys, **ins)["log_f"][:, 7:10]
    w2, model2 = mm.small_model(n, noise=noise, num_obs=2, seed=seed + 1)
    other_seed = n.mpc_step(model2, tick, u=None, keys=keys, **ins)["log_f"][:, 7:10]
    for other in (other_key, other_tick, other_seed):
        assert (other[:, 2] != u0[:, 2]).all()
    assert len({float(x) for x in u0[:, 2]}) == E, "every episode its own normals"
    over = n.mpc_step(model, tick, u=given, keys=keys, **ins)
    assert same(over["log_f"][:, 7:10], given)
    with pytest.raises(ValueError):
        n.mpc_step(model, tick, u=None, **ins)


def _one(w, **over):
    """Inputs of one episode driving straight along y = 0 at 6 m/s."""
    O = w["num_obs"]
    ins = dict(cx=np.linspace(0, 90, 11, dtype=F32)[None], cy=np.zeros((1, 11), F32), u=np.zeros((1, 3), F32),
               mean=np.zeros((1, 8), F32), pos=np.array([[0.0, 0.0]]), vel=np.array([[6.0, 0.0, 0.0]], F32),
               vehicles=np.full((1, O, 4), 1e4, F32), done_tick=np.full(1, -1, np.int32))
    ins["vehicles"][..., 2:] = 0
    ins.update(over)
    return ins


def test_edge_cases():
    n = native_mod()
    QNAN = np.array([0x7FC00000], np.uint32).view(F32)[0]
    # no vehicle: clear = -inf, nothing collides
    w0, m0 = mm.small_model(n, num_obs=0)
    ins = _one(w0)
    out = n.mpc_step(m0, 0, device=None, **ins)
    check_all(out, w0, 0, ins, 1)
    assert out["log_f"][0, 10] == -np.inf and out["log_i"][0, 1] == 0 and out["done_tick"][0] == -1
    assert out["pos"][0, 0] > 0 and out["x_obs"].shape == (1, 0, 100)
    # a frozen episode's state does not change, whatever the plan asks, and its inputs carry no acceleration
    w, m = mm.small_model(n, num_obs=2)
    ins = _one(w, done_tick=np.array([3], np.int32))
    ins["vehicles"][0, 0] = [30, 0, 2, 0.5]
    out = n.mpc_step(m, 5, device=None, **ins)
    check_all(out, w, 5, ins, 1)
    for k in ("pos", "vel", "vehicles", "done_tick"):
        assert same(out[k], ins[k]), k
    assert same(out["init_state"][0], np.array([0, 0, 6, 0, 0, 0], F32)) and out["log_i"][0, 3] == 1
    assert same(out["x_obs"][0, 0], (F32(30) + F32(2) * mm.TT).astype(F32))
    # a NaN plan: collided, and every NaN the step stores is the quiet NaN 0x7FC00000
    ins = _one(w)
    ins["cx"][0, 3] = np.nan
    out = n.mpc_step(m, 2, device=None, **ins)
    check_all(out, w, 2, ins, 1)
    assert out["log_i"][0, 1] == 1 and out["done_tick"][0] == 2
    for k in ("vel", "init_state", "st0", "log_f"):
        a = out[k][0]
        assert np.isnan(a).any() and same(a[np.isnan(a)], np.full(int(np.isnan(a).sum()), QNAN, F32)), k
    assert np.isnan(out["pos"]).all() and same(out["pos"][0], np.array([np.nan, np.nan]))
    # s2 = 0 (a plan that stands still): curv = 0 / 0, stored as the quiet NaN; the model's verdict is a collision
    ins = _one(w, cx=np.zeros((1, 11), F32))
    out = n.mpc_step(m, 2, device=None, **ins)
    check_all(out, w, 2, ins, 1)
    assert same(out["log_f"][0, 11], QNAN) and same(out["log_f"][0, 4], QNAN) and out["log_i"][0, 1] == 1
    # a vehicle exactly on the ellipse: clear == 0 is not a collision; one ulp inside is
    a_obs = float(w["a_obs"])
    ins = _one(w, done_tick=np.array([0], np.int32), pos=np.array([[10.0, 0.0]]))
    ins["vehicles"][0, 0] = [10.0 + a_obs, 0, 0, 0]
    out = n.mpc_step(m, 1, device=None, **ins)
    check_all(out, w, 1, ins, 1)
    assert out["log_f"][0, 10] == 0.0 and out["log_i"][0, 1] == 0
    ins["vehicles"][0, 0, 0] = np.nextafter(F32(10.0 + a_obs), F32(0))
    out = n.mpc_step(m, 1, device=None, **ins)
    assert out["log_f"][0, 10] > 0.0 and out["log_i"][0, 1] == 1
    # lane and goal flags
    ins = _one(w, pos=np.array([[199.9, float(w["y_ub"]) + 0.5]]))
    out = n.mpc_step(m, 4, device=None, **ins)
    assert out["log_i"][0, 0] == 1 and out["log_i"][0, 2] == 1 and out["done_tick"][0] == 4


def test_argument_errors():
    n = native_mod()
    L = n.lib()
    assert L.mpcmmd_mpc_step_host(None, 0, None) == -1 and L.mpcmmd_last_error()
    assert L.mpcmmd_mpc_step_device(None, 0, 1, 0, None) == -1
    for key, bad in (("num_obs", -1), ("num_obs", 65), ("num_batch", 0), ("noise", 2), ("dt", 0.0), ("a_obs", 0.0),
                     ("b_obs", -1.0)):
        w, model = mm.small_model(n)
        setattr(model.c, key, bad)
        io = n.MpcStepIO()
        assert L.mpcmmd_mpc_step_host(C.byref(model.c), 0, C.byref(io)) == -1, key
        assert L.mpcmmd_mpc_step_device(C.byref(model.c), 0, 1, 0, C.byref(io)) == -1, key
    w, model = mm.small_model(n)
    assert L.mpcmmd_mpc_step_host(C.byref(model.c), 0, C.byref(n.MpcStepIO())) == -1
    assert b"null array" in L.mpcmmd_last_error()
    model.c.pdot2 = None
    assert L.mpcmmd_mpc_step_host(C.byref(model.c), 0, C.byref(n.MpcStepIO())) == -1
    w, model = mm.small_model(n)
    ins = mm.random_inputs(np.random.default_rng(0), w, 2)
    for bad in (0, 65536):   # n_episodes out of range, before any HIP call
        io = n.MpcStepIO(*[C.cast(C.c_void_p(8), t) for _, t in n.MpcStepIO._fields_])
        assert L.mpcmmd_mpc_step_device(C.byref(model.c), 0, bad, 0, C.byref(io)) == -1, bad
    out = C.c_void_p()
    assert L.mpcmmd_mpc_create(None, C.byref(model.c), 4, C.byref(out)) == -1 and not out.value
    assert L.mpcmmd_mpc_reset(None, 1, None, None, None, None, None, None, None) == -1
    assert L.mpcmmd_mpc_run(None, 2, 0, 1, None, None) == -1
    assert L.mpcmmd_mpc_log(None, 1, None, None, None, None, None) == -1
    assert L.mpcmmd_mpc_first_normals(None, None) == -1
    L.mpcmmd_mpc_destroy(None)


def test_pop0_is_the_fixed_key_stream():
    """mpcmmd_mpc_first_normals: stream 16 under the fixed key and the configuration's seed."""
    from oracle import rng as R
    n = native_mod()
    cfg = n.make_config(4, 2, 0.1, 8, "gaussian", 0.0, 0.0, num_batch=20, seed=5)
    assert same(n.pop0_normals(cfg), R.philox_normals(R.fixed_key(5), 16, 0, 160).reshape(20, 8))


def test_mpc_program_under_sanitizers():
    """`make asan_mpc` builds tests/native/asan_mpc.cpp with the host-only sources under ASan /
    UBSan (-fno-sanitize-recover); its run, a child process with nothing preloaded, must exit 0 with
    no sanitizer report, and the checksums it prints must be those of the library's host step on the
    same inputs."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    subprocess.run(["make", "-C", PKG, "asan_mpc"], check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(PKG, "build_asan", "asan_mpc")], capture_output=True, text=True, env=env,
                       timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "ok"
    # the program's model, restated here: 3 vehicles, a population of 4, 5 chained ticks
    n = native_mod()
    w, model = mm.small_model(n, num_obs=3, B=4)
    pd = np.zeros((2, 11))
    pd[0, 1], pd[1, 1], pd[1, 2] = 1.0, 1.0, 0.01
    pdd = np.zeros(11)
    pdd[2] = 0.5
    chol = np.diag([2.0] * 8)
    pop0 = ((np.arange(32, dtype=F32) - 16) / 8).reshape(4, 8)
    model.arrays.update(pdot2=pd, pddot1=pdd, chol=chol)
    model.pop0 = pop0
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    model.c.pdot2, model.c.pddot1, model.c.chol, model.c.pop0 = dp(pd), dp(pdd), dp(chol), n._fptr(pop0)
    for k, v in dict(dt=0.15, sigma_acc=0.2, sigma_steer=0.1, acc_const=0.05, steer_const=0.01, K_steer=0.03,
                     a_obs=4.25, b_obs=2.75, y_lb=-5.25, y_ub=5.25, goal_x=1000.0).items():
        setattr(model.c, k, v)
    st = dict(cx=np.zeros((1, 11), F32), cy=np.zeros((1, 11), F32), u=np.array([[0.5, -0.25, 1.0]], F32),
              mean=np.arange(8, dtype=F32)[None] + 1, pos=np.array([[1.0, 0.5]]),
              vel=np.array([[6.0, 0.1, 0.0]], F32),
              vehicles=np.array([[[40, 1, -1, 0], [-10, 0, 2, 0], [60, -2, 0, 0.5]]], F32),
              done_tick=np.full(1, -1, np.int32))
    st["cx"][0, 1], st["cx"][0, 2], st["cy"][0, 2] = 6.0, 40.0, 0.2
    for k in range(5):
        out = n.mpc_step(model, k, device=None, **st)
        st.update(pos=out["pos"], vel=out["vel"], vehicles=out["vehicles"], done_tick=out["done_tick"])
        words = np.concatenate([out[key].reshape(-1).view(np.uint32) for key in
                                ("init_state", "st0", "x_obs", "y_obs", "pop", "log_f")])
        want = f"tick {k} {int(words.astype(np.uint64).sum() & 0xFFFFFFFF):08x}"
        got = lines[k].split()
        assert " ".join(got[:3]) == want and float(got[3]) == out["pos"][0, 0], (lines[k], want)
