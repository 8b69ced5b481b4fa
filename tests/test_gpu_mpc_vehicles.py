"""The planned vehicles of the synthetic closed loop on the GPU: the planned
instantiation of k_mpc_step against its host twin on every word it writes, the chained loop with
the policy on against the host-stepped loop bit for bit (the run split in two and the kernel
through the host included), the same with the validation stage on, the policy turned off again on
the same context, and the context's state and argument errors.  The shapes are those of
tests/test_gpu_mpc_step.py and tests/test_gpu_mpc_loop.py."""
import ctypes as C

import numpy as np
import pytest

import mpc_world_model as mm

pytestmark = pytest.mark.gpu

F32 = np.float32
STEP_KEYS = ("pos", "vel", "vehicles", "done_tick", "init_state", "st0", "x_obs", "y_obs", "pop", "log_d", "log_f",
             "log_i", "veh_acc", "veh_log")
OUT = ("log_d", "log_f", "log_i", "done_tick", "cx", "cy", "mean", "veh")
VAL = ("val_counts", "val_count_pos", "val_stats", "val_mmd", "val_est")
NEW = ("mpcmmd_mpc_vehicle_constant", "mpcmmd_mpc_step_host_planned", "mpcmmd_mpc_step_device_planned",
       "mpcmmd_mpc_plan_vehicles", "mpcmmd_mpc_vehicle_log")
E, T = 3, 4
QNAN = np.uint32(0x7FC00000)


@pytest.fixture(autouse=True)
def pin_generators(monkeypatch):
    """MPCMMD_GENWAVE is read when a handle is created: every handle of these tests gets the same
    beta-CEM generators whatever its capacity."""
    monkeypatch.setenv("MPCMMD_GENWAVE", "1")


@pytest.fixture(autouse=True)
def symbols(native):
    for s in NEW:   # a library without the entry points fails every test of this file
        assert s in native.SYMBOLS and hasattr(native.lib(), s), s


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def both(native, model, tick, ins, planned):
    host = native.mpc_step(model, tick, device=None, planned=planned, **ins)
    dev = native.mpc_step(model, tick, device=0, planned=planned, **ins)
    for k in STEP_KEYS:
        assert same(dev[k], host[k]), (k, np.argwhere(dev[k] != host[k])[:4], dev[k].ravel()[:4], host[k].ravel()[:4])
    return host


@pytest.mark.parametrize("num_obs", [1, 2, 64])
@pytest.mark.parametrize("noise", ["gaussian", "beta"])
def test_device_step_equals_host_step(native, noise, num_obs):
    """Episode 0 has a NaN target, episode 1 is frozen, episode 2 has a vehicle on the ego; then the
    frozen step of tick -1 that makes tick 0's inputs."""
    w, model = mm.small_model(native, noise=noise, num_obs=num_obs, seed=3, variant="dynamic")
    rng = np.random.default_rng(23 + num_obs)
    ins = mm.random_inputs(rng, w, E)
    acc = np.stack([rng.uniform(-2, 2, (E, num_obs)), rng.uniform(-1, 1, (E, num_obs))], 2).astype(F32)
    target = np.stack([rng.normal(6, 0.5, (E, num_obs)), rng.choice([-1.75, 1.75], (E, num_obs))], 2).astype(F32)
    ins["vehicles"][:, :, 0] = ins["pos"][:, None, 0] + rng.uniform(30, 90, (E, num_obs))   # ahead, out of reach
    ins["done_tick"][1] = 2
    ins["vehicles"][2, 0] = [ins["pos"][2, 0] + 1.0, ins["pos"][2, 1] + 0.2, ins["vel"][2, 0], 0.0]
    acc[2, 0] = 0.0
    target[2, 0] = [ins["vel"][2, 0], ins["pos"][2, 1]]
    target[0, num_obs - 1, 1] = np.nan
    out = both(native, model, 5, ins, dict(acc=acc, target=target))
    assert out["done_tick"].tolist() == [5, 2, 5] and out["log_i"][:, 1].tolist() == [1, 0, 1] and out["log_i"][1, 3] == 1
    nan = out["veh_log"][0, num_obs - 1, 1::2].view(np.uint32)
    assert (nan == QNAN).all() and (out["y_obs"][0, num_obs - 1].view(np.uint32) == QNAN).all()
    assert np.isfinite(out["x_obs"]).all() and np.isfinite(out["y_obs"][1:]).all()
    assert same(out["vehicles"][1], ins["vehicles"][1]) and same(out["veh_acc"][1], acc[1])
    assert not same(out["vehicles"][2], ins["vehicles"][2]) and not same(out["veh_acc"][2], acc[2])
    # the policy is on: the tracks are no straight lines
    plain = native.mpc_step(model, 5, device=0, **ins)
    assert not same(plain["x_obs"][2], out["x_obs"][2]) and "veh_log" not in plain
    ins["done_tick"][:] = 0
    frozen = both(native, model, -1, ins, dict(acc=acc, target=target))
    assert same(frozen["vehicles"], ins["vehicles"]) and same(frozen["veh_acc"], acc)


def test_no_vehicle(native):
    w, model = mm.small_model(native, num_obs=0, variant="dynamic")
    ins = mm.random_inputs(np.random.default_rng(2), w, E)
    out = both(native, model, 0, ins, dict(acc=None, target=np.zeros((E, 0, 2), F32)))
    assert (out["log_f"][:, 10] == -np.inf).all() and not out["log_i"][:, 1].any()
    assert out["veh_log"].shape == (E, 0, 6)


def make_prob(noise="gaussian", max_configs=E):
    from optimizer.cem import CEM
    return CEM(4, 2, 0.1, 8, noise, 0.05, 0.01, num_batch=20, variant="dynamic", maxiter_cem=3, max_configs=max_configs)


def scene():
    """3 episodes of the dynamic variant: two slower vehicles ahead in the other lane that cut in to
    the ego's (one stays), starts a few metres apart; nonzero start accelerations."""
    vehicles = np.array([[[35, 1.75, 3, 0], [50, 1.75, 2, 0]], [[40, 1.75, 4, 0], [60, -1.75, 3, 0]],
                         [[30, 1.75, 3, -0.3], [45, 1.75, 2.5, 0]]], F32)
    starts = np.array([[0, -1.75, 5.0, 0], [2, -2.0, 6.0, 0.1], [4, -1.5, 4.0, -0.1]], float)
    target = np.array([[[6.0, -1.75], [5.9, -1.75]], [[6.1, -1.75], [6.0, -1.75]], [[5.95, -1.75], [6.05, 1.75]]], F32)
    acc = np.array([[[0, 0], [0.5, 0]], [[0, -0.2], [0, 0]], [[0, 0], [-0.25, 0.1]]], F32)
    return vehicles, starts, dict(target=target, acc=acc)


@pytest.mark.parametrize("cost,noise,given", [("cvar", "gaussian", True), ("mmd_opt", "beta", False)])
def test_chained_loop_equals_host_stepped_loop(native, cost, noise, given):
    vehicles, starts, planned = scene()
    u = np.random.default_rng(3).standard_normal((T, E, 3)).astype(F32) if given else None
    prob = make_prob(noise)
    try:
        host = prob.run_episodes(cost, vehicles, starts, T, chained=False, device_step=None, u=u, planned=planned)
        chain = prob.run_episodes(cost, vehicles, starts, T, chained=True, u=u, planned=planned)
        halves = prob.run_episodes(cost, vehicles, starts, T, chained=(2, 2), u=u, planned=planned)
        dev = prob.run_episodes(cost, vehicles, starts, T, chained=False, device_step=0, u=u, planned=planned)
        plain = prob.run_episodes(cost, vehicles, starts, T, chained=True, u=u)
    finally:
        prob.handle.close()
    for k in OUT:
        assert same(dev[k], host[k]), ("kernel through the host", k, np.argwhere(dev[k] != host[k])[:4])
        assert same(chain[k], host[k]), ("chained", k, np.argwhere(chain[k] != host[k])[:4])
        assert same(halves[k], host[k]), ("run(0, 2) + run(2, 2)", k)
    veh = host["veh"]
    assert veh.shape == (T, E, 2, 6) and np.isfinite(veh).all() and np.isfinite(host["cx"]).all()
    assert (np.diff(veh[:, :, :, 0], axis=0) > 0).all(), "every vehicle advances"
    assert (veh[-1, [0, 0, 1, 2], [0, 1, 0, 0], 1] < 1.75).all(), "the cut-in has begun"
    assert "veh" not in plain and not same(plain["log_f"][:, :, 10], host["log_f"][:, :, 10]), "other positions"
    assert (np.diff(host["log_d"][:, :, 0], axis=0) > 0).all()


def test_with_the_validation_stage(native):
    vehicles, starts, planned = scene()
    val = dict(rollouts=64, sigma=(0.5,))
    prob = make_prob()
    try:
        host = prob.run_episodes("cvar", vehicles, starts, T, chained=False, validate=val, planned=planned)
        chain = prob.run_episodes("cvar", vehicles, starts, T, chained=True, validate=val, planned=planned)
    finally:
        prob.handle.close()
    for k in OUT + VAL:
        assert same(chain[k], host[k]), (k, np.argwhere(chain[k] != host[k])[:4])
    assert host["val_mmd"].shape == (T, E, 3, 1) and np.isfinite(host["val_stats"]).all()


def context(native, prob, max_ticks=T):
    cov = np.diag([20.0] * 4 + [100.0] * 4).astype(F32)
    model = native.MpcModel(prob._cfg, cov, native.pop0_normals(prob._cfg), goal_x=200.0)
    return native.Mpc(prob.handle, model, max_ticks), cov


def reset(ctx, cov, vehicles, starts, n=E):
    vel = np.concatenate([starts[:n, 2:4], np.arctan2(starts[:n, 3:4], starts[:n, 2:3])], 1).astype(F32)
    mean = np.tile(np.array([15.0] * 4 + [0.0] * 4, F32), (n, 1))
    ctx.reset(starts[:n, :2], vel, vehicles[:n], mean, cov, None, 100003 * np.arange(n))


def test_solver_reads_the_planned_tracks(native):
    """What the chained solve of tick 1 read from the handle's obs buffer -- packed by the validation
    stage -- is track(plan(S_1, target)) of the vehicle log's row 0, restated in NumPy: the first
    num_prime points, bit for bit."""
    import mpc_vehicle_model as vm
    vehicles, starts, planned = scene()
    K = vm.constants(native, 0.15)
    prob = make_prob()
    try:
        ctx, cov = context(native, prob)
        ctx.validate(8, sigma=())
        ctx.plan_vehicles(planned["target"], planned["acc"])
        reset(ctx, cov, vehicles, starts)
        ctx.run("cvar", 0, 2, cov, 15.0)
        veh, ins = ctx.vehicle_log(2), ctx.validation_inputs()
        ctx.close()
    finally:
        prob.handle.close()
    H = prob.num_prime
    for e in range(E):
        cxf, cyf = vm.plan(K, veh[0, e], planned["target"][e])
        assert same(ins["x_obs"][e, :, :H], vm.track(K, cxf)[:, :H]), e
        assert same(ins["y_obs"][e, :, :H], vm.track(K, cyf)[:, :H]), e
    assert not ins["x_obs"][:, :, H:].any() and not same(veh[0, :, :, :4], vehicles)


def test_policy_off_again(native):
    """After a planned run, plan_vehicles(None) and a reset: the context's next run is a fresh
    context's without the policy.  A second reset with the policy on starts from the staged
    accelerations again."""
    vehicles, starts, planned = scene()
    prob = make_prob()
    try:
        ctx, cov = context(native, prob)
        ctx.plan_vehicles(planned["target"], planned["acc"])
        reset(ctx, cov, vehicles, starts)
        ctx.run("cvar", 0, T, cov, 15.0)
        first, veh1 = ctx.log(T), ctx.vehicle_log(T)
        reset(ctx, cov, vehicles, starts)
        ctx.run("cvar", 0, T, cov, 15.0)
        again, veh2 = ctx.log(T), ctx.vehicle_log(T)
        ctx.plan_vehicles(None)
        reset(ctx, cov, vehicles, starts)
        ctx.run("cvar", 0, T, cov, 15.0)
        off = ctx.log(T)
        ctx.close()
        fresh, _ = context(native, prob)
        reset(fresh, cov, vehicles, starts)
        fresh.run("cvar", 0, T, cov, 15.0)
        want = fresh.log(T)
        fresh.close()
    finally:
        prob.handle.close()
    assert same(veh1, veh2) and not same(veh1[0, :, :, 4:], planned["acc"])
    for k in want:
        assert same(again[k], first[k]), ("a second planned run", k)
        assert same(off[k], want[k]), ("the policy off again", k)
    assert not same(first["log_f"][:, :, 10], want["log_f"][:, :, 10]), "the planned vehicles were elsewhere"


def test_state_and_argument_errors(native):
    vehicles, starts, planned = scene()
    L, fp = native.lib(), native._fptr
    prob = make_prob()
    try:
        ctx, cov = context(native, prob)
        vd = np.full(E, 15.0, F32)
        run = lambda: L.mpcmmd_mpc_run(ctx._c, 2, 0, 1, fp(cov.reshape(64)), fp(vd))
        buf = np.zeros((T, E, 2, 6), F32)
        assert L.mpcmmd_mpc_vehicle_log(ctx._c, 1, fp(buf)) == -4, "MPCMMD_E_STATE: the policy is off"
        reset(ctx, cov, vehicles, starts)
        assert run() == 0
        tg = np.ascontiguousarray(planned["target"])
        assert L.mpcmmd_mpc_plan_vehicles(ctx._c, 0, fp(tg), None) == -1
        assert L.mpcmmd_mpc_plan_vehicles(ctx._c, E + 1, fp(tg), None) == -1
        assert run() == 0, "a refused call changes nothing"
        ctx.plan_vehicles(tg[:2])
        assert run() == -4, "MPCMMD_E_STATE between plan_vehicles and the reset"
        with pytest.raises(native.NativeError):
            reset(ctx, cov, vehicles, starts)          # 3 episodes, 2 staged
        assert b"n_episodes" in L.mpcmmd_last_error()
        assert run() == -4, "a refused reset does not count"
        reset(ctx, cov, vehicles, starts, n=2)
        assert L.mpcmmd_mpc_run(ctx._c, 2, 0, 2, fp(cov.reshape(64)), fp(vd)) == 0
        assert L.mpcmmd_mpc_vehicle_log(ctx._c, T + 1, fp(buf)) == -1 and L.mpcmmd_mpc_vehicle_log(ctx._c, 1, None) == -1
        veh = ctx.vehicle_log(2)
        assert veh.shape == (2, 2, 2, 6) and np.isfinite(veh).all() and (veh[1, :, :, 0] > veh[0, :, :, 0]).all()
        ctx.plan_vehicles(None)
        assert run() == -4 and L.mpcmmd_mpc_vehicle_log(ctx._c, 1, fp(buf)) == -4
        ctx.close()
    finally:
        prob.handle.close()
