"""The validation stage of the chained closed loop (mpcmmd_world_validate,
DESIGN.md section 20) against its reference, the host-linked loop that calls
mpcmmd_validate_carla_risk after every tick's solve: every val_* array bit-equal
for the chained run, a run split in two and each episode alone; the loop
undisturbed by the stage; the row-block edges of R; the packed inputs against
host-formed ones (H = 8, and H = 100 where v[100] = v[99] is live); rows that
hit and rows that do not; and the entry points' errors.  No tolerance anywhere.
The setup is test_gpu_closed_loop.py's: num_batch 20, maxiter_cem 3, num_prime 8,
2 obstacles, 37 waypoints, 5 vehicles, 3 episodes x 6 ticks."""
import ctypes as C
import importlib
import math

import numpy as np
import pytest

from test_carla_tick_cpu import carla_package
from test_gpu_closed_loop import E, OUT, P, T, make_prob, pin_generators, same, world  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

F32 = np.float32
VAL = ("val_counts", "val_count_pos", "val_var", "val_cvar", "val_mean", "val_max", "val_mmd", "val_est")
CASES = [("cvar", 4, "gaussian"), ("det", 4, "beta"), ("mmd", 4, "gaussian")]


def carla_native():
    """The binding module the CARLA package loaded (its own copy, by file path): the one whose
    structs ``prob.world_model`` returns."""
    return importlib.import_module(carla_package() + "._lib").native()


def given_u(cost):
    """cvar: given variates; det, mmd: drawn by the library (test_gpu_closed_loop.py's choice)."""
    return np.random.default_rng(3).standard_normal((T, E, 4)) if cost == "cvar" else None


def assert_val_equal(got, want, what):
    for k in VAL:
        assert same(got[k], want[k]), (what, k, np.argwhere(np.asarray(got[k]) != np.asarray(want[k]))[:4])


@pytest.mark.parametrize("cost,n,noise", CASES)
def test_chained_validation_equals_host_linked(native, world, cost, n, noise):
    """R = 100: two row blocks of 64, the second ragged.  The host-linked route stores what
    finish_batch returned as cost_lane, cost_obs in val_est, so val_est is held to that too."""
    route, goal, vehicles, starts = world
    u = given_u(cost)
    val = dict(rollouts=100, alpha=0.9, sigma=[0.1, 1.0])
    prob = make_prob(n, noise)
    try:
        kw = dict(goal_index=goal, num_path=P, u=u, validate=val)
        chain = prob.run_episodes(cost, route, vehicles, starts, T, chained=True, **kw)
        halves = prob.run_episodes(cost, route, vehicles, starts, T, chained=(3, 3), **kw)
        host = prob.run_episodes(cost, route, vehicles, starts, T, device_step=False, **kw)
        alone = [prob.run_episodes(cost, route, vehicles, starts[e:e + 1], T, chained=True, goal_index=goal,
                                   num_path=P, u=None if u is None else u[:, e:e + 1], key_base=100000 * e,
                                   validate=val)
                 for e in range(E)]
    finally:
        prob.close()
    assert host["val_mmd"].shape == (T, E, 3, 2) and host["val_counts"].shape == (T, E, 3)
    assert_val_equal(chain, host, "chained")
    assert_val_equal(halves, host, "run(0, 3) + run(3, 3)")
    for k in OUT:   # and the loop itself is the host-linked one's, as without the stage
        assert same(chain[k], host[k]), ("chained", k)
    for e in range(E):
        for k in VAL:
            assert same(alone[e][k][:, 0], host[k][:, e]), ("alone", e, k)
    # the validators' own invariants
    assert same(host["val_count_pos"][..., 0], host["val_counts"][..., 2])
    assert (host["val_counts"] >= 0).all() and (host["val_counts"][..., 2] <= 100).all()
    assert np.isfinite(host["val_est"]).all()
    # every (tick, episode) has its own key: the lane statistics differ between rows
    assert np.unique(host["val_mean"][..., 1:].reshape(T * E, 2), axis=0).shape[0] > 1


@pytest.mark.parametrize("cost,n,noise", CASES)
def test_stage_does_not_disturb_the_loop(native, world, cost, n, noise):
    route, goal, vehicles, starts = world
    prob = make_prob(n, noise)
    try:
        kw = dict(goal_index=goal, num_path=P, u=given_u(cost), chained=True)
        off = prob.run_episodes(cost, route, vehicles, starts, T, **kw)
        path_off = prob.handle.read("path").copy()
        on = prob.run_episodes(cost, route, vehicles, starts, T, validate=dict(rollouts=100, sigma=[0.1, 1.0]), **kw)
        path_on = prob.handle.read("path").copy()
        again = prob.run_episodes(cost, route, vehicles, starts, T, **kw)
    finally:
        prob.close()
    assert not any(k.startswith("val_") for k in off) and sorted(off) == sorted(again)
    for k in OUT:
        assert same(on[k], off[k]), k
        assert same(again[k], off[k]), k
    assert same(path_on, path_off) and np.abs(path_off).sum() > 0


@pytest.mark.parametrize("R", [1, 64, 65])
def test_row_count_edges(native, world, R):
    """One row, exactly one full block of 64 rows, one row into the second block; S = 0 and S = 1."""
    route, goal, vehicles, starts = world
    prob = make_prob(4)
    try:
        for sigma in ((), (0.5,)):
            kw = dict(goal_index=goal, num_path=P, validate=dict(rollouts=R, alpha=0.98, sigma=sigma))
            chain = prob.run_episodes("cvar", route, vehicles, starts, 2, chained=True, **kw)
            host = prob.run_episodes("cvar", route, vehicles, starts, 2, device_step=False, **kw)
            assert chain["val_mmd"].shape == (2, E, 3, len(sigma))
            assert_val_equal(chain, host, (R, sigma))
            assert (host["val_counts"][..., 2] <= R).all()
    finally:
        prob.close()


def host_inputs(prob, log, fin, keys, tick, H, num_path):
    """The validators' inputs of tick ``tick`` formed on the host from what the chained run left:
    plan_controls of the returned v_best and steering, carla_velocity_heading of the tick's
    init_state (0, 0, v, 0, psi, psidot of the ego after tick - 1's step), the path's first
    num_path columns, obs padded to 100 columns, keys = idx_mpc."""
    n, O = len(fin), prob.num_obs
    v = np.array([r["v_best"] for r in fin], F32)
    vn = np.concatenate([v[:, 1:], v[:, 99:]], 1)   # v[100] = v[99]
    acc = ((vn - v) / F32(0.15)).astype(F32)[:, :H]
    steer = np.array([r["steering"] for r in fin], F32)[:, :H]
    st0 = np.zeros((n, 8), F32)
    for e in range(n):
        v0, psi0 = log["log_f"][tick - 1, e, 0], log["log_f"][tick - 1, e, 1]
        vx, vy = v0 * F32(math.cos(float(psi0))), v0 * F32(math.sin(float(psi0)))
        st0[e, 2:5] = vx, vy, F32(math.atan2(float(vy), float(vx)))
    path = prob.handle.read("path").reshape(-1, 6, 2048)[:n, :, :num_path]
    obs = prob.handle.read("obs", shape=(n, 2, O, H))
    tracks = np.zeros((2, n, O, 100), F32)
    tracks[:, :, :, :H] = obs.transpose(1, 0, 2, 3)
    return dict(acc=acc, steer=steer, st0=st0, path=path, x_obs=tracks[0], y_obs=tracks[1],
                keys=(tick + np.asarray(keys)).astype(np.uint32))


@pytest.mark.parametrize("H,num_path", [(8, 37), (8, 64), (100, 37), (100, 64)])
def test_packed_inputs(native, world, H, num_path):
    route, goal, vehicles, starts = world
    cem = importlib.import_module(carla_package() + ".cem")
    prob = cem.CEM(4, 1, 2, 0.1, H, "gaussian", "Town05", 0.05, 0.01, num_batch=20, maxiter_cem=3, max_configs=E)
    cov = np.diag([20.0] * 4 + [100.0] * 4).astype(F32)
    keys = 100000 * np.arange(E)
    native = carla_native()
    try:
        model, tk = prob.world_model(route, vehicles.shape[0], goal, num_path, cov)
        w = native.World(tk, model, 2)
        w.validate(10, sigma=[0.1])
        w.reset(starts[:, :2], np.stack([starts[:, 2], starts[:, 3], np.zeros(E)], 1), np.tile(vehicles[None], (E, 1, 1)),
                np.tile(np.array([10.0] * 4 + [0.0] * 4, F32), (E, 1)), cov, None, keys)
        w.run("cvar", 0, 2, cov, 10.0)
        got = w.validation_inputs()
        log = w.log(2)
        fin = prob.handle.finish_batch()   # the handle holds the last tick's solve
        want = host_inputs(prob, log, fin, keys, 1, H, num_path)
        vlog = w.validation_log(2)
        w.close()
    finally:
        prob.close()
    for k, a in want.items():
        assert same(got[k], a), (k, np.argwhere(got[k] != a)[:4])
    assert np.abs(got["acc"]).sum() > 0 and np.abs(got["path"]).sum() > 0 and (got["st0"][:, 2] > 0).all()
    if H == 100:   # the edge: the last acc is (v[99] - v[99]) / dt
        assert (got["acc"][:, 99] == 0).all() and (got["acc"][:, 98] != 0).any()
    else:
        assert (got["x_obs"][:, :, H:] == 0).all() and (got["x_obs"][:, :, :H] != 0).any()
    assert same(vlog["val_est"][1], np.array([[r["cost_lane"], r["cost_obs"]] for r in fin], F32))


def test_not_vacuous(native, world):
    """A world of this test's own: a stationary vehicle 4.5 m ahead of the third start (inside the
    horizon's reach of the second, out of the first's), so some plans hit in some rows and
    others in none."""
    route, goal, _, starts = world
    vehicles = np.array([[12.5, 0.0, 0, 0, 0], [40, -3.5, 1.0, 0, 0], [-20, 0, 0, 0, 0]], F32)
    R = 100
    prob = make_prob(4)
    try:
        kw = dict(goal_index=goal, num_path=P, validate=dict(rollouts=R, sigma=[0.1]))
        chain = prob.run_episodes("cvar", route, vehicles, starts, 3, chained=True, **kw)
        host = prob.run_episodes("cvar", route, vehicles, starts, 3, device_step=False, **kw)
    finally:
        prob.close()
    assert_val_equal(chain, host, "own world")
    rows = chain["val_counts"][..., 2]
    print("count_rows\n", rows, "\nval_cvar obs\n", chain["val_cvar"][..., 0], "\nval_est\n", chain["val_est"])
    assert same(chain["val_count_pos"][..., 0], rows)
    assert (rows >= 0).all() and (rows <= R).all()
    assert (rows > 0).any() and (rows == 0).any()
    # a row that hits has a positive obstacle cost: its mean, maximum and MMD say so
    hit = rows > 0
    assert (chain["val_max"][..., 0][hit] > 0).all() and (chain["val_max"][..., 0][~hit] == 0).all()
    assert (chain["val_mmd"][..., 0, 0][hit] > 0).all()


def test_errors(native, world):
    route, goal, vehicles, starts = world
    prob = make_prob(4)
    cov = np.diag([20.0] * 4 + [100.0] * 4).astype(F32)
    native = carla_native()
    L = native.lib()
    ip, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    try:
        model, tk = prob.world_model(route, vehicles.shape[0], goal, P, cov)
        w = native.World(tk, model, 4)
        st = (starts[:, :2], np.stack([starts[:, 2], starts[:, 3], np.zeros(E)], 1), np.tile(vehicles[None], (E, 1, 1)),
              np.tile(np.array([10.0] * 4 + [0.0] * 4, F32), (E, 1)), cov, None, 100000 * np.arange(E))
        w.reset(*st)
        for call in (lambda: w.validation_log(1), w.validation_inputs):   # the stage is off
            with pytest.raises(native.NativeError, match="without a validation stage"):
                call()
        for bad in (dict(rollouts=0), dict(rollouts=(1 << 20) + 1), dict(rollouts=10, alpha=1.5),
                    dict(rollouts=10, alpha=-0.1), dict(rollouts=10, alpha=float("nan")),
                    dict(rollouts=10, sigma=[0.1] * 9), dict(rollouts=10, sigma=[0.1, 0.0]),
                    dict(rollouts=10, sigma=[-1.0]), dict(rollouts=10, sigma=[float("inf")]),
                    dict(rollouts=10, sigma=[float("nan")])):
            with pytest.raises(native.NativeError, match="world validation"):
                w.validate(**bad)
        w.run("cvar", 0, 1, cov, 10.0)   # a refused configuration changed nothing: the reset still holds
        w.validate(10, sigma=[0.1])
        with pytest.raises(native.NativeError, match="before mpcmmd_world_reset"):   # it takes effect at a reset
            w.run("cvar", 0, 1, cov, 10.0)
        w.reset(*st)
        w.run("cvar", 0, 2, cov, 10.0)
        for ticks in (-1, 5):
            with pytest.raises(native.NativeError, match="tick range"):
                w.validation_log(ticks)
        n = 2 * E
        cn, cp, s4 = np.zeros((n, 3), np.int32), np.zeros((n, 3), np.int32), np.zeros((n, 12), F32)
        mm, es = np.zeros((n, 3), F32), np.zeros((n, 2), F32)
        full = [cn.ctypes.data_as(ip), cp.ctypes.data_as(ip), s4.ctypes.data_as(fp), mm.ctypes.data_as(fp),
                es.ctypes.data_as(fp)]
        for missing in range(5):   # every log array is required (mmd too: S = 1)
            args = [None if i == missing else a for i, a in enumerate(full)]
            assert L.mpcmmd_world_validation_log(w._w, 2, *args) == -1 and b"null" in L.mpcmmd_last_error()
        assert L.mpcmmd_world_validation_log(w._w, 2, *full) == 0
        first = w.validation_log(2)
        assert same(first["val_counts"].reshape(n, 3), cn) and same(first["val_est"].reshape(n, 2), es)
        assert w.validation_log(0)["val_counts"].shape == (0, E, 3)
        # off again: the readbacks are state errors, the loop runs as before
        w.validate(None)
        w.reset(*st)
        w.run("cvar", 0, 2, cov, 10.0)
        with pytest.raises(native.NativeError, match="without a validation stage"):
            w.validation_log(2)
        with pytest.raises(native.NativeError, match="without a validation stage"):
            w.validation_inputs()
        assert w.log(2)["log_d"].shape == (2, E, 3)
        w.close()
    finally:
        prob.close()


def test_too_many_obstacles_for_the_validator(native, world):
    """The validators take at most 32 obstacle tracks: a handle with 33 is refused before any HIP call."""
    route, goal, _, _ = world
    cem = importlib.import_module(carla_package() + ".cem")
    prob = cem.CEM(4, 1, 33, 0.1, 8, "gaussian", "Town05", 0.05, 0.01, num_batch=20, maxiter_cem=3, max_configs=1)
    native = carla_native()
    try:
        model, tk = prob.world_model(route, 33, goal, P)
        w = native.World(tk, model, 2)
        with pytest.raises(native.NativeError, match="num_obs <= 32"):
            w.validate(10)
        w.close()
    finally:
        prob.close()
