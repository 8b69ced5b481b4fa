"""Closed-loop episodes of the synthetic variants on the GPU (CEM.run_episodes, DESIGN.md section
21): the chained run (mpcmmd_mpc_run: begin, CEM and k_mpc_step enqueued per tick, nothing
crossing the host), the run split in two and the loop stepped by k_mpc_step through the host
against the same loop stepped by the host twin (mpcmmd_solve_batch + mpcmmd_mpc_step_host) --
every log row and every tick's cx, cy and mean bit-equal -- an episode alone against the same key
inside a batch of 3, the context's errors, and mpcmmd_solve_batch on the same handle before and
after a chained run.  Small shapes: n = 4, 2 obstacles, num_prime 8, num_batch 20, maxiter_cem
3, 3 episodes x 6 ticks."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F32 = np.float32
OUT = ("log_d", "log_f", "log_i", "done_tick", "cx", "cy", "mean")
E, T = 3, 6


@pytest.fixture(autouse=True)
def pin_generators(monkeypatch):
    """MPCMMD_GENWAVE is read when a handle is created: every handle of these tests gets the same
    beta-CEM generators whatever its capacity, so runs of 1 and of 3 episodes compare bit for bit."""
    monkeypatch.setenv("MPCMMD_GENWAVE", "1")


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def make_prob(variant, noise="gaussian", max_configs=E):
    from optimizer.cem import CEM
    return CEM(4, 2, 0.1, 8, noise, 0.05, 0.01, num_batch=20, variant=variant, maxiter_cem=3, max_configs=max_configs)


def scene(variant):
    """3 episodes: two obstacles ahead (moving in the dynamic variant), starts a few metres apart."""
    y = -1.75 if variant == "dynamic" else 1.75
    v = 3.0 if variant == "dynamic" else 0.0
    vehicles = np.array([[[35, y, v, 0], [50, -y, v, 0]], [[40, -y, v, 0], [60, y, v, 0]],
                         [[30, y, v, 0.1 * v], [45, y, v, 0]]], F32)
    starts = np.array([[0, y, 5.0, 0], [2, y - 0.25, 6.0, 0.1], [4, y + 0.25, 4.0, -0.1]], float)
    return vehicles, starts


@pytest.mark.parametrize("variant", ["static", "dynamic"])
@pytest.mark.parametrize("cost,noise,given", [("cvar", "gaussian", True), ("saa", "beta", False),
                                              ("mmd_random", "beta", False), ("mmd_opt", "gaussian", False)])
def test_chained_loop_equals_host_stepped_loop(native, variant, cost, noise, given):
    vehicles, starts = scene(variant)
    u = np.random.default_rng(3).standard_normal((T, E, 3)).astype(F32) if given else None
    prob = make_prob(variant, noise)
    try:
        host = prob.run_episodes(cost, vehicles, starts, T, chained=False, device_step=None, u=u)
        chain = prob.run_episodes(cost, vehicles, starts, T, chained=True, u=u)
        halves = prob.run_episodes(cost, vehicles, starts, T, chained=(3, 3), u=u)
        dev = prob.run_episodes(cost, vehicles, starts, T, chained=False, device_step=0, u=u)
        alone = [prob.run_episodes(cost, vehicles[e:e + 1], starts[e:e + 1], T, chained=True,
                                   u=None if u is None else u[:, e:e + 1], key_base=100003 * e) for e in range(E)]
    finally:
        prob.handle.close()
    for k in OUT:
        assert same(dev[k], host[k]), ("kernel through the host", k, np.argwhere(dev[k] != host[k])[:4])
        assert same(chain[k], host[k]), ("chained", k, np.argwhere(chain[k] != host[k])[:4])
        assert same(halves[k], host[k]), ("run(0, 3) + run(3, 3)", k)
    # the loop is closed: x advances, the plans differ from tick to tick and between the episodes
    x = host["log_d"][:, :, 0]
    assert (x[0] > starts[:, 0]).all() and (np.diff(x, axis=0) > 0).all() and np.isfinite(host["cx"]).all()
    assert not same(host["cx"][0], host["cx"][T - 1]) and not same(host["cx"][:, 0], host["cx"][:, 1])
    assert not same(host["mean"][0], host["mean"][T - 1])
    uu = host["log_f"][:, :, 7:10]
    if given:
        assert same(uu, u)
    else:
        assert np.unique(uu[:, :, 2]).size == T * E, "every (tick, episode) its own variates"
        if noise == "beta":
            assert ((uu[:, :, :2] >= 0) & (uu[:, :, :2] <= 1)).all() and np.unique(uu[:, :, 0]).size > T
    # every episode alone, under its own key, equals its slot in the batch of 3
    for e in range(E):
        for k in OUT:
            a = alone[e][k]
            assert same(a[:, 0] if a.ndim > 1 else a[0], host[k][:, e] if host[k].ndim > 1 else host[k][e]), (e, k)


def test_existing_route_unchanged_around_a_chained_run(native):
    """mpcmmd_solve_batch on the same handle before and after a chained run returns the same bits."""
    vehicles, starts = scene("static")
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
        prob.run_episodes("cvar", vehicles, starts, T, chained=True)
        after = solve()
    finally:
        prob.handle.close()
    for a, b in zip(before, after):
        for k in ("cx", "cy", "cost_lane", "cost_obs"):
            assert same(np.asarray(a[k]), np.asarray(b[k])), k


def test_context_errors(native):
    """A run before a reset is a state error; a CARLA handle, a model whose num_obs is not the
    handle's, too many episodes, a covariance that is not positive definite and a tick range past
    max_ticks are invalid; mmd_opt on a handle without it is unsupported."""
    import mpc_world_model as mm
    L = native.lib()
    cfg = native.make_config(4, 2, 0.1, 8, "gaussian", 0.05, 0.01, num_batch=20, maxiter_cem=3)
    handle = native.Handle(cfg, max_configs=E)
    cov = np.diag([20.0] * 4 + [100.0] * 4).astype(F32)
    vehicles, starts = scene("static")
    try:
        model = native.MpcModel(cfg, cov, native.pop0_normals(cfg), goal_x=200.0)
        out = C.c_void_p()
        assert L.mpcmmd_mpc_create(handle._h, C.byref(model.c), 0, C.byref(out)) == -1
        _, other = mm.small_model(native, num_obs=3)
        assert L.mpcmmd_mpc_create(handle._h, C.byref(other.c), 4, C.byref(out)) == -1
        assert b"num_obs" in L.mpcmmd_last_error()
        ccfg = native.make_config(4, 2, 0.1, 8, "gaussian", 0.05, 0.01, num_batch=20, variant="carla_town05",
                                  maxiter_cem=3)
        ch = native.Handle(ccfg)
        try:
            assert L.mpcmmd_mpc_create(ch._h, C.byref(model.c), 4, C.byref(out)) == -1 and not out.value
        finally:
            ch.close()
        ctx = native.Mpc(handle, model, 4)
        fp = native._fptr
        vd = np.full(E, 15.0, F32)
        assert L.mpcmmd_mpc_run(ctx._c, 2, 0, 1, fp(cov.reshape(64)), fp(vd)) == -4, "MPCMMD_E_STATE before a reset"
        vel = np.concatenate([starts[:, 2:4], np.zeros((E, 1))], 1).astype(F32)
        mean = np.tile(np.array([15.0] * 4 + [0.0] * 4, F32), (E, 1))
        with pytest.raises(native.NativeError):
            ctx.reset(np.zeros((E + 1, 2)), np.zeros((E + 1, 3)), np.zeros((E + 1, 2, 4)), np.zeros((E + 1, 8)), cov,
                      None, np.arange(E + 1))
        with pytest.raises(native.NativeError):
            ctx.reset(starts[:, :2], vel, vehicles, mean, -cov, None, np.arange(E))
        assert L.mpcmmd_mpc_run(ctx._c, 2, 0, 1, fp(cov.reshape(64)), fp(vd)) == -4, "failed resets do not count"
        ctx.reset(starts[:, :2], vel, vehicles, mean, cov, None, np.arange(E))
        for begin, count in ((0, 5), (-1, 1), (4, 1), (0, -1)):
            assert L.mpcmmd_mpc_run(ctx._c, 2, begin, count, fp(cov.reshape(64)), fp(vd)) == -1, (begin, count)
        assert L.mpcmmd_mpc_run(ctx._c, 2, 0, 1, None, fp(vd)) == -1
        assert L.mpcmmd_mpc_run(ctx._c, 4, 0, 1, fp(cov.reshape(64)), fp(vd)) == -1, "det is the CARLA optimizer's"
        ctx.run("cvar", 0, 2, cov, 15.0)
        log = ctx.log(2)
        assert np.isfinite(log["cx"]).all() and (log["log_d"][1, :, 0] > log["log_d"][0, :, 0]).all()
        ld = np.empty((5, E, 2))
        assert L.mpcmmd_mpc_log(ctx._c, 5, ld.ctypes.data_as(C.POINTER(C.c_double)), None, None, None, None) == -1
        ctx.close()
    finally:
        handle.close()
    # mmd_opt on a handle without it (num_reduced 70 > 64): unsupported, before anything is enqueued
    cfg = native.make_config(70, 2, 0.1, 8, "gaussian", 0.05, 0.01, num_batch=20, maxiter_cem=3)
    handle = native.Handle(cfg)
    try:
        ctx = native.Mpc(handle, native.MpcModel(cfg, cov, native.pop0_normals(cfg), goal_x=200.0), 2)
        ctx.reset(starts[:1, :2], vel[:1], vehicles[:1], mean[:1], cov, None, [0])
        vd = np.full(1, 15.0, F32)
        assert L.mpcmmd_mpc_run(ctx._c, 0, 0, 1, fp(cov.reshape(64)), fp(vd)) == -3, "MPCMMD_E_UNSUPPORTED"
        ctx.close()
    finally:
        handle.close()
