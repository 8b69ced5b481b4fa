"""k_mpc_step against its host twin: mpcmmd_mpc_step_device equals mpcmmd_mpc_step_host on every
word it writes.  E = 3 episodes, 1 / 2 / 32 vehicles (one lane each: a partial wave), a
population of 20; both noise kinds, given and drawn variates, a frozen episode, a NaN plan, a plan
that stands still (s2 = 0) and no vehicle at all."""
import numpy as np
import pytest

import mpc_world_model as mm

pytestmark = pytest.mark.gpu

F32 = np.float32
KEYS = ("pos", "vel", "vehicles", "done_tick", "init_state", "st0", "x_obs", "y_obs", "pop", "log_d", "log_f", "log_i")
E = 3


@pytest.fixture(autouse=True)
def pin_generators(monkeypatch):
    monkeypatch.setenv("MPCMMD_GENWAVE", "1")


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def both(native, model, tick, ins, **kw):
    host = native.mpc_step(model, tick, device=None, **ins, **kw)
    dev = native.mpc_step(model, tick, device=0, **ins, **kw)
    for k in KEYS:
        assert same(dev[k], host[k]), (k, np.argwhere(dev[k] != host[k])[:4], dev[k].ravel()[:4], host[k].ravel()[:4])
    return host


@pytest.mark.parametrize("num_obs", [1, 2, 32])
@pytest.mark.parametrize("noise", ["gaussian", "beta"])
def test_device_step_equals_host_step(native, noise, num_obs):
    w, model = mm.small_model(native, noise=noise, num_obs=num_obs, seed=3)
    ins = mm.random_inputs(np.random.default_rng(17 + num_obs), w, E)
    ins["done_tick"][1] = 2                                   # a frozen episode
    ins["vehicles"][2, 0, :2] = ins["pos"][2] + [1.0, 0.2]    # a vehicle on the ego of episode 2
    out = both(native, model, 5, ins)
    assert out["done_tick"][1:].tolist() == [2, 5] and out["log_i"][1, 3] == 1 and out["log_i"][2, 1] == 1
    assert not same(out["pos"][0], ins["pos"][0]) and same(out["pos"][1], ins["pos"][1])
    # drawn variates: the kernel draws them from (key, seed, tick) once the controls are known
    given = ins.pop("u")
    keys = np.array([3, 100003, 200003])
    drawn = both(native, model, 5, ins, u=None, keys=keys)
    u = drawn["log_f"][:, 7:10]
    assert np.unique(u[:, 2]).size == E and not same(u, given)
    if noise == "beta":
        assert ((u[:, :2] >= 0) & (u[:, :2] <= 1)).all()
    # a NaN plan and a plan that stands still: collided, every stored NaN the quiet NaN
    ins["cx"][0, 3] = np.nan
    ins["cx"][2] = ins["cy"][2] = 0.0
    ins["done_tick"][:] = -1
    bad = both(native, model, 6, ins, u=given)
    assert bad["log_i"][0, 1] == 1 and bad["log_i"][2, 1] == 1 and bad["done_tick"][[0, 2]].tolist() == [6, 6]
    nan = bad["log_f"][0][np.isnan(bad["log_f"][0])]
    assert nan.size and (nan.view(np.uint32) == 0x7FC00000).all()


def test_no_vehicle(native):
    w, model = mm.small_model(native, num_obs=0)
    ins = mm.random_inputs(np.random.default_rng(2), w, E)
    out = both(native, model, 0, ins)
    assert (out["log_f"][:, 10] == -np.inf).all() and not out["log_i"][:, 1].any()
