"""The validation stage of the synthetic closed loop (mpcmmd_mpc_validate):
the Monte-Carlo risk of every tick's plan, computed inside the chained loop on the GPU.  Every
val_* array of the chained run -- whole, split (2, 2), each episode alone, the stage in-line and
on the side stream -- against the host-linked loop that calls mpcmmd_validate and
mpcmmd_validate_risk after each tick's solve, bit for bit; the loop's own log with and without
the stage; the packed inputs against a NumPy restatement; two scenes whose answer is known without
a GPU; the errors.  test_gpu_mpc_loop.py's shapes: n = 4, 2 obstacles, num_prime 8, num_batch
20, maxiter_cem 3, 3 episodes x 4 ticks; R = 1025 is two row blocks of k_vrisk_roll (the second
holds one rollout) and two passes of k_validate's rollout loop."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F32 = np.float32
OUT = ("log_d", "log_f", "log_i", "done_tick", "cx", "cy", "mean")
VAL = ("val_counts", "val_count_pos", "val_stats", "val_mmd", "val_est")
E, T = 3, 4
R_MAIN, SIGMA_MAIN = 1025, (0.01, 0.3)
INVALID, UNSUPPORTED, STATE = -1, -3, -4


@pytest.fixture(autouse=True)
def pin_generators(monkeypatch):
    """MPCMMD_GENWAVE is read when a handle is created: every handle of these tests gets the same
    beta-CEM generators whatever its capacity, so runs of 1 and of 3 episodes compare bit for bit."""
    monkeypatch.setenv("MPCMMD_GENWAVE", "1")


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def make_prob(variant, noise="gaussian", max_configs=E, num_obs=2, num_prime=8):
    from optimizer.cem import CEM
    return CEM(4, num_obs, 0.1, num_prime, noise, 0.05, 0.01, num_batch=20, variant=variant, maxiter_cem=3,
               max_configs=max_configs)


def scene(variant):
    """test_gpu_mpc_loop.py's: 3 episodes, two obstacles ahead (moving in the dynamic variant)."""
    y = -1.75 if variant == "dynamic" else 1.75
    v = 3.0 if variant == "dynamic" else 0.0
    vehicles = np.array([[[35, y, v, 0], [50, -y, v, 0]], [[40, -y, v, 0], [60, y, v, 0]],
                         [[30, y, v, 0.1 * v], [45, y, v, 0]]], F32)
    starts = np.array([[0, y, 5.0, 0], [2, y - 0.25, 6.0, 0.1], [4, y + 0.25, 4.0, -0.1]], float)
    return vehicles, starts


def variates(given):
    return np.random.default_rng(3).standard_normal((T, E, 3)).astype(F32) if given else None


@functools.lru_cache(maxsize=None)
def host_linked(variant, cost, noise, given, R, sigma):
    """The reference of a case, computed once: the host-linked loop with the validators after each
    tick's solve.  The arrays are shared between the cases and never written."""
    vehicles, starts = scene(variant)
    prob = make_prob(variant, noise)
    try:
        out = prob.run_episodes(cost, vehicles, starts, T, chained=False, device_step=None, u=variates(given),
                                validate=dict(rollouts=R, sigma=sigma))
    finally:
        prob.handle.close()
    for a in out.values():
        a.setflags(write=False)
    return out


def check_routes(variant, cost, noise, given, R, sigma, overlap):
    vehicles, starts = scene(variant)
    u = variates(given)
    host = host_linked(variant, cost, noise, given, R, sigma)
    val = dict(rollouts=R, sigma=sigma, overlap=overlap)
    prob = make_prob(variant, noise)
    try:
        chain = prob.run_episodes(cost, vehicles, starts, T, chained=True, u=u, validate=val)
        halves = prob.run_episodes(cost, vehicles, starts, T, chained=(2, 2), u=u, validate=val)
        alone = [prob.run_episodes(cost, vehicles[e:e + 1], starts[e:e + 1], T, chained=True,
                                   u=None if u is None else u[:, e:e + 1], key_base=100003 * e, validate=val)
                 for e in range(E)]
    finally:
        prob.handle.close()
    assert host["val_mmd"].shape == (T, E, 3, len(sigma)) and host["val_stats"].shape == (T, E, 4, 3)
    for k in OUT + VAL:
        assert same(chain[k], host[k]), ("chained", k, np.argwhere(chain[k] != host[k])[:4])
        assert same(halves[k], host[k]), ("run(0, 2) + run(2, 2)", k, np.argwhere(halves[k] != host[k])[:4])
        for e in range(E):
            a = alone[e][k]
            assert same(a[:, 0] if a.ndim > 1 else a[0], host[k][:, e] if host[k].ndim > 1 else host[k][e]), (e, k)
    # the rows are live: R rollouts each, every tick and episode its own noise rows, the solver's own estimate kept
    assert np.isfinite(host["val_stats"]).all() and np.isfinite(host["val_est"]).all()
    assert (host["val_count_pos"] >= 0).all() and (host["val_count_pos"] <= R).all()
    assert (host["val_counts"] >= 0).all() and (host["val_counts"][..., 0] <= R).all()


@pytest.mark.parametrize("overlap", [0, 1])
@pytest.mark.parametrize("variant", ["static", "dynamic"])
@pytest.mark.parametrize("cost,noise,given", [("cvar", "gaussian", True), ("saa", "beta", False),
                                              ("mmd_opt", "gaussian", False)])
def test_chained_validation_equals_host_linked(native, variant, cost, noise, given, overlap):
    check_routes(variant, cost, noise, given, R_MAIN, SIGMA_MAIN, overlap)


@pytest.mark.parametrize("overlap", [0, 1])
@pytest.mark.parametrize("S", [0, 1])
@pytest.mark.parametrize("R", [1, 1024, 1025])
def test_row_count_edges(native, R, S, overlap):
    """R = 1 (one rollout: var = cvar = mean = max), 1024 (exactly one row block and one pass) and
    1025, without bandwidths (no MMD launches, mmd NULL) and with one."""
    check_routes("static", "cvar", "gaussian", True, R, (0.3,)[:S], overlap)
    if R == 1:
        st = host_linked("static", "cvar", "gaussian", True, R, (0.3,)[:S])["val_stats"]
        assert same(st[:, :, 0], st[:, :, 3]) and same(st[:, :, 2], st[:, :, 3])


def test_stage_does_not_disturb_the_loop(native):
    """With the stage on (both placements) the loop's log and every tick's cx, cy, mean are those of
    the run without it, and mpcmmd_solve_batch on the same handle returns the same bits before
    and after."""
    vehicles, starts = scene("static")
    u = variates(True)
    prob = make_prob("static")
    try:
        h = prob.handle
        init = np.array([0.0, 1.75, 5.0, 0.0, 0.0, 0.0], F32)
        mean = np.array([15.0] * 4 + [0.0] * 4, F32)
        cov = np.diag([20.0] * 4 + [100.0] * 4).astype(F32)
        tt = np.linspace(0, 15, 100).astype(F32)
        xo = (vehicles[:, :, 0:1] + 0 * tt).astype(F32)
        yo = (vehicles[:, :, 1:2] + 0 * tt).astype(F32)
        solve = lambda: h.solve_batch("cvar", [11, 12, 13], init, mean, cov, xo, yo, 15.0)
        before = solve()
        plain = prob.run_episodes("cvar", vehicles, starts, T, chained=True, u=u)
        runs = [prob.run_episodes("cvar", vehicles, starts, T, chained=True, u=u,
                                  validate=dict(rollouts=R_MAIN, sigma=SIGMA_MAIN, overlap=ov)) for ov in (0, 1)]
        after = solve()
        again = prob.run_episodes("cvar", vehicles, starts, T, chained=True, u=u)
    finally:
        prob.handle.close()
    assert set(plain) == set(OUT) and set(again) == set(OUT), "without validate= the dict is what it was"
    for got in runs + [again]:
        for k in OUT:
            assert same(got[k], plain[k]), k
    for k in VAL:
        assert same(runs[0][k], runs[1][k]), k
    for a, b in zip(before, after):
        for k in ("cx", "cy", "cost_lane", "cost_obs"):
            assert same(np.asarray(a[k]), np.asarray(b[k])), k


@pytest.mark.parametrize("H", [8, 100])
def test_packed_inputs(native, H):
    """validation_inputs() after the last tick against a NumPy restatement: the log's plan widened,
    the init state from the previous tick's log row, the tracks of the vehicles where T - 1 steps
    left them (columns >= H zero; H = 100 has none to zero), keys = tick + key."""
    vehicles, starts = scene("dynamic")
    prob = make_prob("dynamic", num_prime=H)
    cov = np.diag([20.0] * 4 + [100.0] * 4).astype(F32)
    keys = 7 + 100003 * np.arange(E)
    try:
        model = native.MpcModel(prob._cfg, cov, native.pop0_normals(prob._cfg), goal_x=200.0)
        ctx = native.Mpc(prob.handle, model, T)
        ctx.validate(64, sigma=(0.3,), overlap=True)
        vel = np.concatenate([starts[:, 2:4], np.arctan2(starts[:, 3:4], starts[:, 2:3])], 1).astype(F32)
        mean = np.tile(np.array([15.0] * 4 + [0.0] * 4, F32), (E, 1))
        ctx.reset(starts[:, :2], vel, vehicles, mean, cov, None, keys)
        ctx.run("cvar", 0, T, cov, 15.0)
        got, log = ctx.validation_inputs(), ctx.log(T)
        ctx.close()
    finally:
        prob.handle.close()
    assert (log["done_tick"] == -1).all(), "the restatement below steps every vehicle on every tick"
    assert same(got["cx"], log["cx"][T - 1].astype(np.float64)) and same(got["cy"], log["cy"][T - 1].astype(np.float64))
    init = np.zeros((E, 6))
    init[:, :2] = log["log_d"][T - 2].astype(F32)   # the position rounded as the step's init_state rounds it
    init[:, 2:4] = log["log_f"][T - 2, :, :2]       # vx, vy after the step
    assert same(got["init_state"], init)
    veh = vehicles.copy()
    for _ in range(T - 1):
        veh[:, :, 0] = veh[:, :, 0] + veh[:, :, 2] * F32(0.15)
        veh[:, :, 1] = veh[:, :, 1] + veh[:, :, 3] * F32(0.15)
    tt = np.linspace(0, 15, 100).astype(F32)
    xo, yo = np.zeros((E, 2, 100), F32), np.zeros((E, 2, 100), F32)
    xo[:, :, :H] = (veh[:, :, 0:1] + veh[:, :, 2:3] * tt)[:, :, :H]
    yo[:, :, :H] = (veh[:, :, 1:2] + veh[:, :, 3:4] * tt)[:, :, :H]
    assert xo.dtype == F32 and same(got["x_obs"], xo) and same(got["y_obs"], yo)
    assert same(got["keys"], (T - 1 + keys).astype(np.uint32))


@pytest.mark.parametrize("overlap", [0, 1])
def test_known_answers(native, overlap):
    """Episode 0 starts 2 m behind a stationary vehicle in its lane: at step 0 of tick 0 every rollout
    has f_bar = 1 - 4 / 18.0625 > 0, so all R rollouts count.  Episode 1's vehicles are 1000 m away:
    no rollout ever has a positive obstacle cost, every statistic of the channel is 0 and its MMD is
    the all-zero channel's closed form, 1000 (1 - 2) exactly."""
    R = R_MAIN
    y = 1.75
    vehicles = np.array([[[2, y, 0, 0], [60, -y, 0, 0]], [[1000, y, 0, 0], [1100, -y, 0, 0]],
                         [[30, y, 0, 0], [45, y, 0, 0]]], F32)
    starts = np.array([[0, y, 5.0, 0], [2, y - 0.25, 6.0, 0.1], [4, y + 0.25, 4.0, -0.1]], float)
    prob = make_prob("static")
    try:
        out = prob.run_episodes("cvar", vehicles, starts, T, chained=True,
                                validate=dict(rollouts=R, sigma=SIGMA_MAIN, overlap=overlap))
    finally:
        prob.handle.close()
    OBS = 0
    assert out["val_count_pos"][0, 0, OBS] == R and out["val_counts"][0, 0, 0] == R
    assert out["val_stats"][0, 0, 3, OBS] > 0
    assert (out["val_count_pos"][:, 1, OBS] == 0).all() and (out["val_counts"][:, 1, 0] == 0).all()
    assert (out["val_stats"][:, 1, :, OBS] == 0).all()
    assert (out["val_mmd"][:, 1, OBS, :] == F32(-1000.0)).all()


def test_errors(native):
    """Every MPCMMD_E_INVALID and MPCMMD_E_STATE case of include/mpcmmd.h, and that a refused
    configuration leaves the context as it was."""
    L = native.lib()
    prob = make_prob("static")
    cov = np.diag([20.0] * 4 + [100.0] * 4).astype(F32)
    vehicles, starts = scene("static")
    fp, ip, dp = native._fptr, C.POINTER(C.c_int32), C.POINTER(C.c_double)
    vd = np.full(E, 15.0, F32)

    def cfg_of(R=16, alpha=0.98, sigma=(0.3,), overlap=1, num_sigma=None):
        c = native.MpcValidation(R, alpha, len(sigma) if num_sigma is None else num_sigma)
        for i, v in enumerate(sigma):
            c.sigma[i] = v
        c.overlap = overlap
        return c

    run = lambda ctx, k=0, n=1: L.mpcmmd_mpc_run(ctx._c, 2, k, n, fp(cov.reshape(64)), fp(vd))
    try:
        model = native.MpcModel(prob._cfg, cov, native.pop0_normals(prob._cfg), goal_x=200.0)
        ctx = native.Mpc(prob.handle, model, T)
        vel = np.concatenate([starts[:, 2:4], np.zeros((E, 1))], 1).astype(F32)
        mean = np.tile(np.array([15.0] * 4 + [0.0] * 4, F32), (E, 1))
        reset = lambda: ctx.reset(starts[:, :2], vel, vehicles, mean, cov, None, np.arange(E))
        cn, cp = np.zeros((T, E, 2), np.int32), np.zeros((T, E, 3), np.int32)
        st, mm, es = np.zeros((T, E, 4, 3), F32), np.zeros((T, E, 3, 1), F32), np.zeros((T, E, 2), F32)
        log_args = [cn.ctypes.data_as(ip), cp.ctypes.data_as(ip), fp(st), fp(mm), fp(es)]
        # a NULL context
        assert L.mpcmmd_mpc_validate(None, C.byref(cfg_of())) == INVALID
        assert L.mpcmmd_mpc_validate(None, None) == INVALID
        assert L.mpcmmd_mpc_validation_log(None, 1, *log_args) == INVALID
        assert L.mpcmmd_mpc_validation_inputs(None, None, None, None, None, None, None) == INVALID
        # the stage off: read-backs are state errors
        assert L.mpcmmd_mpc_validation_log(ctx._c, 1, *log_args) == STATE
        assert L.mpcmmd_mpc_validation_inputs(ctx._c, None, None, None, None, None, None) == STATE
        # refused configurations, each leaving the context able to run
        reset()
        bad = [cfg_of(R=0), cfg_of(R=-1), cfg_of(R=(1 << 20) + 1), cfg_of(alpha=-0.01), cfg_of(alpha=1.01),
               cfg_of(alpha=float("nan")), cfg_of(sigma=(), num_sigma=-1), cfg_of(sigma=(0.3,) * 8, num_sigma=9),
               cfg_of(sigma=(0.3, 0.0)), cfg_of(sigma=(-0.3,)), cfg_of(sigma=(float("inf"),)),
               cfg_of(sigma=(float("nan"),)), cfg_of(overlap=2), cfg_of(overlap=-1)]
        for i, c in enumerate(bad):
            assert L.mpcmmd_mpc_validate(ctx._c, C.byref(c)) == INVALID, i
        assert run(ctx) == 0 and L.mpcmmd_mpc_validation_log(ctx._c, 1, *log_args) == STATE
        # the edges of the ranges are accepted; a run between the configuration and the next reset is a state error
        for c in (cfg_of(R=1, alpha=0.0, sigma=()), cfg_of(R=1 << 20, alpha=1.0, sigma=(0.3,) * 8, overlap=0), cfg_of()):
            assert L.mpcmmd_mpc_validate(ctx._c, C.byref(c)) == 0
        assert run(ctx) == STATE
        reset()
        assert run(ctx, 0, 2) == 0
        # the log's required arrays and its tick range
        for i in (0, 1, 2, 3, 4):
            args = list(log_args)
            args[i] = None
            assert L.mpcmmd_mpc_validation_log(ctx._c, 2, *args) == INVALID and b"null" in L.mpcmmd_last_error(), i
        assert L.mpcmmd_mpc_validation_log(ctx._c, -1, *log_args) == INVALID
        assert L.mpcmmd_mpc_validation_log(ctx._c, T + 1, *log_args) == INVALID
        assert L.mpcmmd_mpc_validation_log(ctx._c, 0, *log_args) == 0
        assert L.mpcmmd_mpc_validation_log(ctx._c, 2, *log_args) == 0 and (cp[:2] <= 16).all() and (cp[:2] >= 0).all()
        assert L.mpcmmd_mpc_validation_inputs(ctx._c, None, None, None, None, None, None) == 0, "every array optional"
        # without bandwidths mmd may be NULL
        assert L.mpcmmd_mpc_validate(ctx._c, C.byref(cfg_of(sigma=()))) == 0
        reset()
        assert run(ctx) == 0
        args = list(log_args)
        args[3] = None
        assert L.mpcmmd_mpc_validation_log(ctx._c, 1, *args) == 0
        # turning the stage off also waits for the next reset; then the loop runs as before and has no validation log
        assert L.mpcmmd_mpc_validate(ctx._c, None) == 0
        assert run(ctx) == STATE
        reset()
        assert run(ctx) == 0
        assert L.mpcmmd_mpc_validation_log(ctx._c, 1, *log_args) == STATE
        assert L.mpcmmd_mpc_validation_inputs(ctx._c, None, None, None, None, None, None) == STATE
        ctx.close()
    finally:
        prob.handle.close()


def test_too_many_obstacles_for_the_validators(native):
    """The loop takes up to 64 vehicles, the validators 1..32: a 33-obstacle handle is refused, and
    its loop goes on without the stage."""
    L = native.lib()
    cfg = native.make_config(4, 33, 0.1, 8, "gaussian", 0.05, 0.01, num_batch=20, maxiter_cem=3)
    cov = np.diag([20.0] * 4 + [100.0] * 4).astype(F32)
    handle = native.Handle(cfg)
    try:
        ctx = native.Mpc(handle, native.MpcModel(cfg, cov, native.pop0_normals(cfg), goal_x=200.0), 2)
        with pytest.raises(native.NativeError, match="num_obs"):
            ctx.validate(16)
        assert L.mpcmmd_mpc_validate(ctx._c, C.byref(native.MpcValidation(16, 0.98, 0))) == INVALID
        ctx.close()
    finally:
        handle.close()
