"""The accounting of carla/closed_loop.py without a GPU: a fake episode runner
with known logs, the files it writes and the figures it prints; and the
synthetic world's route, spawns and starts."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CARLA = os.path.join(ROOT, "mpc-mmd_amd", "carla")
F32 = np.float32


@pytest.fixture(scope="module")
def CL():
    spec = importlib.util.spec_from_file_location("mpcmmd_carla_closed_loop", os.path.join(CARLA, "closed_loop.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def fake_run(prob, cost, route, goal_index, vehicles, starts, ticks, **kw):
    """4 episodes x 5 ticks.  Episode 0 runs through; 1 collides at tick 2 (its rows 3, 4 repeat
    the frozen state, with a lane flag that must not count); 2 reaches the goal at tick 3; 3
    leaves the lane at tick 1 and runs through."""
    T, E = int(ticks), 4
    assert (T, np.asarray(starts).shape, goal_index, kw) == (5, (4, 4), 7, dict(seed=3))
    log_d = np.zeros((T, E, 3))
    log_f = np.zeros((T, E, 13), F32)
    log_i = np.zeros((T, E, 4), np.int32)
    log_d[:, :, 2] = 2.0 + np.arange(T)[:, None] * np.array([1.0, 2.0, 3.0, 0.5])   # arc: progress per tick
    log_f[:, :, 11] = -5.0 + np.arange(T)[:, None] * np.array([1.0, 3.0, 0.5, -1.0])   # clear
    done = np.array([-1, 2, 3, -1], np.int32)
    log_i[2:, 1, 2] = 1
    log_i[3:, 1, 1] = 1          # after the episode froze: not counted
    log_d[3:, 1, 2] = log_d[2, 1, 2]
    log_f[3:, 1, 11] = 99.0      # not counted either
    log_i[3:, 2, 3] = 1
    log_i[1, 3, 1] = 1
    return dict(log_d=log_d, log_f=log_f, log_i=log_i, done_tick=done, collided=np.array([0, 1, 0, 0], bool),
                goal=np.array([0, 0, 1, 0], bool), cost=cost)


def test_accounting(CL, tmp_path):
    lines = []
    res = CL.closed_loop(None, ["cvar", "det"], None, 7, None, np.zeros((4, 4)), 5, out_dir=str(tmp_path),
                         run=fake_run, log=lines.append, seed=3)
    assert sorted(res) == ["cvar", "det"] and res["det"][0]["cost"] == "det"
    s = res["cvar"][1]
    sd = lambda v: float(np.std(v, ddof=1))
    assert s["collision"] == (0.25, sd([0, 1, 0, 0]))
    # min over the live ticks of -clear: 5 - 4, 5 - 6 (tick 2), 5 - 1.5 (tick 3), 5 (tick 0)
    want = [1.0, -1.0, 3.5, 5.0]
    assert s["min_neg_clear"] == (float(np.mean(want)), sd(want))
    assert s["lane_departure"] == (0.25, sd([0, 0, 0, 1]))
    want = [4.0, 4.0, 9.0, 2.0]   # arc at the last live tick minus arc at tick 0
    assert s["progress"] == (float(np.mean(want)), sd(want))
    assert len(lines) == 2 and lines[0].startswith("cvar: 4 episodes x 5 ticks, collision share = 0.2500 +- 0.5000")
    assert "lane departure share = 0.2500" in lines[0] and "mean progress = 4.75 +- " in lines[0]
    with np.load(tmp_path / "closed_loop_cvar.npz") as z:
        assert sorted(z.files) == sorted(CL.LOG_KEYS)
        assert z["log_f"].shape == (5, 4, 13) and z["done_tick"].tolist() == [-1, 2, 3, -1]
    with pytest.raises(ValueError):
        CL.closed_loop(None, ["saa"], None, 7, None, np.zeros((4, 4)), 5, run=fake_run)


def test_synthetic_world(CL):
    route, goal, vehicles = CL.synthetic_world("Town05")
    R = CL._replay()
    rec = R.record_synthetic(ticks=1)
    assert np.array_equal(np.stack(route), rec["route"]) and goal == R.synthetic_route()[0].size - 1
    assert vehicles.dtype == F32 and np.array_equal(vehicles, rec["obstacles"][0])
    st = CL.synthetic_starts(route, 4, spread=8.0)
    assert st.shape == (4, 4) and np.allclose(st[:, 0], [0, 2, 4, 6]) and np.allclose(st[:, [1, 3]], 0) \
        and np.allclose(st[:, 2], 0.1)
