"""The validation stage and the vehicle policy of one episode context, configured, reconfigured and
dropped in both orders (mpcmmd_world_validate / mpcmmd_world_route_vehicles, mpcmmd_mpc_validate /
mpcmmd_mpc_plan_vehicles): after every change a reset and 2 ticks, whose log, validation log and
vehicle log are those of a context created for that configuration alone, byte for byte.  Every call
is a documented sequence; the two stages own separate device buffers, and neither order of making
or dropping them may disturb the other's.  Shapes: the neighbours' smallest (2 episodes, 2 ticks,
num_batch 20, maxiter_cem 3, num_prime 8, 2 obstacles), R = 64 with one bandwidth, then R = 96
with none."""
import importlib

import numpy as np
import pytest

import world_model as wm
from test_carla_tick_cpu import carla_package

pytestmark = pytest.mark.gpu

F32 = np.float32
E, T, P = 2, 2, 37
VAL64, VAL96 = dict(rollouts=64, sigma=(0.5,)), dict(rollouts=96, sigma=())
# (vehicles policy, validation stage) after each step; the last is reached validation first, vehicles second
STEPS = [(True, None), (True, VAL64), (True, VAL96), (False, VAL96), (False, None), (True, VAL64)]


@pytest.fixture(autouse=True)
def pin_generators(monkeypatch):
    """MPCMMD_GENWAVE is read when a handle is created: every handle of these tests gets the same
    beta-CEM generators."""
    monkeypatch.setenv("MPCMMD_GENWAVE", "1")


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def check_sequence(create, set_vehicles, segment):
    """``create()`` makes a context, ``set_vehicles(ctx, on)`` and ``ctx.validate`` configure it,
    ``segment(ctx, veh, val)`` resets, runs T ticks and returns every log that is on."""
    ctx = create()
    seen = []
    try:
        veh, val = False, None
        for step, (veh_to, val_to) in enumerate(STEPS):
            if val_to != val:   # the context: validation first where both change; the fresh one: vehicles first
                ctx.validate(**(val_to or dict(rollouts=None)))
            if veh_to != veh:
                set_vehicles(ctx, veh_to)
            veh, val = veh_to, val_to
            got = segment(ctx, veh, val)
            fresh = create()
            try:
                if veh:
                    set_vehicles(fresh, True)
                if val:
                    fresh.validate(**val)
                want = segment(fresh, veh, val)
            finally:
                fresh.close()
            assert sorted(got) == sorted(want) and ("veh" in got) == veh and ("val_est" in got) == bool(val), step
            for k in want:
                assert same(got[k], want[k]), (step, k, np.argwhere(np.asarray(got[k]) != np.asarray(want[k]))[:4])
            if val:
                assert got["val_mmd"].shape == (T, E, 3, len(val["sigma"])) and (got["val_count_pos"] <= val["rollouts"]).all()
            seen.append(got)
    finally:
        ctx.close()
    # the policy is live (the vehicles are elsewhere), and both orders reach the same configuration
    assert not same(seen[0]["log_f"], seen[4]["log_f"])
    for k in seen[1]:
        assert same(seen[5][k], seen[1][k]), k


def logs_of(ctx, veh, val):
    out = dict(ctx.log(T))
    if val:
        out.update(ctx.validation_log(T))
    if veh:
        out["veh"] = ctx.vehicle_log(T)
    return out


def test_world_stages_in_both_orders(native):
    """The surrogate world: 5 vehicles, routed or at constant velocity (test_gpu_closed_loop_vehicles.py's)."""
    (rx, ry, *_), len_path = wm.synthetic_route()
    starts = np.array([[0, 0, 3.0, 0], [4, -0.5, 5.0, 0.05]], float)
    vehicles = np.array([[25, 0.2, 0, 0, 0], [40, -3.5, 1.0, 0, 0], [55, 0, 0, 0, 0.1], [-20, 0, 0, 0, 0],
                         [70, 4, 0, 0.5, 1.0]], F32)
    per = lambda a: np.tile(np.asarray(a)[None], (E, 1))
    routed = (per([25.0, 40.0, 55.0, -20.0, 70.0]), per(np.array([2.0, 3.0, 0.0, 4.0, 1.0], F32)),
              np.stack([per(np.array([0.0, -3.5, 0.0, 0.25, -3.5], F32)), per(np.array([4.0, 5.0, 0.0, 9.0, 3.3], F32))], -1))
    cov = np.diag([20.0] * 4 + [100.0] * 4).astype(F32)
    cem = importlib.import_module(carla_package() + ".cem")
    prob = cem.CEM(4, 1, 2, 0.1, 8, "gaussian", "Town05", 0.05, 0.01, num_batch=20, maxiter_cem=3, max_configs=E)
    binding = importlib.import_module(carla_package() + "._lib").native()
    try:
        model, tk = prob.world_model((rx, ry), 5, len_path - 1, P, cov)

        def segment(w, veh, val):
            w.reset(starts[:, :2], np.stack([starts[:, 2], starts[:, 3], np.zeros(E)], 1),
                    None if veh else np.tile(vehicles[None], (E, 1, 1)),
                    np.tile(np.array([10.0] * 4 + [0.0] * 4, F32), (E, 1)), cov, None, 100000 * np.arange(E))
            w.run("cvar", 0, T, cov, 10.0)
            return logs_of(w, veh, val)

        check_sequence(lambda: binding.World(tk, model, T),
                       lambda w, on: w.route_vehicles(*routed) if on else w.route_vehicles(None), segment)
    finally:
        prob.close()


def test_mpc_stages_in_both_orders(native):
    """The synthetic loop, dynamic variant: 2 vehicles, planned or at constant velocity
    (test_gpu_mpc_vehicles.py's); the validators on the side stream."""
    from optimizer.cem import CEM
    vehicles = np.array([[[35, 1.75, 3, 0], [50, 1.75, 2, 0]], [[40, 1.75, 4, 0], [60, -1.75, 3, 0]]], F32)
    starts = np.array([[0, -1.75, 5.0, 0], [2, -2.0, 6.0, 0.1]], float)
    target = np.array([[[6.0, -1.75], [5.9, -1.75]], [[6.1, -1.75], [6.0, -1.75]]], F32)
    acc = np.array([[[0, 0], [0.5, 0]], [[0, -0.2], [0, 0]]], F32)
    cov = np.diag([20.0] * 4 + [100.0] * 4).astype(F32)
    prob = CEM(4, 2, 0.1, 8, "gaussian", 0.05, 0.01, num_batch=20, variant="dynamic", maxiter_cem=3, max_configs=E)
    try:
        model = native.MpcModel(prob._cfg, cov, native.pop0_normals(prob._cfg), goal_x=200.0)

        def segment(ctx, veh, val):
            vel = np.concatenate([starts[:, 2:4], np.arctan2(starts[:, 3:4], starts[:, 2:3])], 1).astype(F32)
            ctx.reset(starts[:, :2], vel, vehicles, np.tile(np.array([15.0] * 4 + [0.0] * 4, F32), (E, 1)), cov, None,
                      100003 * np.arange(E))
            ctx.run("cvar", 0, T, cov, 15.0)
            return logs_of(ctx, veh, val)

        check_sequence(lambda: native.Mpc(prob.handle, model, T),
                       lambda c, on: c.plan_vehicles(target, acc) if on else c.plan_vehicles(None), segment)
    finally:
        prob.handle.close()
