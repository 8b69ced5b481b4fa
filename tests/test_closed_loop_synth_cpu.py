"""The accounting of optimizer/closed_loop.py without a GPU: a fake episode runner with known
logs, the files it writes, the figures it prints and the options it hands on; the scenario of an
episode (the sweep's generator) and the command line with the runner replaced."""
import numpy as np
import pytest

F32 = np.float32


@pytest.fixture(scope="module")
def CL():
    from optimizer import closed_loop
    return closed_loop


def fake_run(prob, cost, vehicles, starts, ticks, **kw):
    """4 episodes x 5 ticks.  Episode 0 runs through; 1 collides at tick 2 (its rows 3, 4 repeat
    the frozen state, with a lane flag that must not count); 2 reaches the goal at tick 3; 3
    leaves the lane at tick 1 and runs through."""
    T, E = int(ticks), 4
    assert (T, np.asarray(starts).shape, kw) == (5, (4, 4), dict(goal_x=120.0))
    log_d = np.zeros((T, E, 2))
    log_f = np.zeros((T, E, 12), F32)
    log_i = np.zeros((T, E, 4), np.int32)
    log_d[:, :, 0] = 2.0 + np.arange(T)[:, None] * np.array([1.0, 2.0, 3.0, 0.5])   # x: progress per tick
    log_f[:, :, 10] = -5.0 + np.arange(T)[:, None] * np.array([1.0, 3.0, 0.5, -1.0])   # clear
    done = np.array([-1, 2, 3, -1], np.int32)
    log_i[2:, 1, 1] = 1          # collided from tick 2 on
    log_i[3:, 1, 0] = 1          # a lane flag after the episode froze: not counted
    log_i[3:, 1, 3] = 1
    log_d[3:, 1, 0] = log_d[2, 1, 0]
    log_f[3:, 1, 10] = 99.0      # not counted either
    log_i[3:, 2, 2] = 1
    log_i[1, 3, 0] = 1
    return dict(log_d=log_d, log_f=log_f, log_i=log_i, done_tick=done, cx=np.zeros((T, E, 11), F32),
                cy=np.ones((T, E, 11), F32), mean=np.zeros((T, E, 8), F32), cost=cost)


def test_accounting(CL, tmp_path):
    lines = []
    res = CL.closed_loop(None, ["cvar", "mmd_opt"], None, np.zeros((4, 4)), 5, out_dir=str(tmp_path), run=fake_run,
                         log=lines.append, goal_x=120.0)
    assert sorted(res) == ["cvar", "mmd_opt"] and res["mmd_opt"][0]["cost"] == "mmd_opt"
    s = res["cvar"][1]
    sd = lambda v: float(np.std(v, ddof=1))
    assert s["collision"] == (0.25, sd([0, 1, 0, 0]))
    # min over the live ticks of -clear: 5 - 4, 5 - 6 (tick 2), 5 - 1.5 (tick 3), 5 (tick 0)
    want = [1.0, -1.0, 3.5, 5.0]
    assert s["min_neg_clear"] == (float(np.mean(want)), sd(want))
    assert s["lane_departure"] == (0.25, sd([0, 0, 0, 1]))
    want = [4.0, 4.0, 9.0, 2.0]   # x at the last live tick minus x at tick 0
    assert s["progress"] == (float(np.mean(want)), sd(want))
    assert len(lines) == 2 and lines[0].startswith("cvar: 4 episodes x 5 ticks, collision share = 0.2500 +- 0.5000")
    assert "lane departure share = 0.2500" in lines[0] and "mean progress = 4.75 +- " in lines[0]
    assert "mean min -clear = 2.1250 +- " in lines[0] and lines[1].startswith("mmd_opt: ")
    with np.load(tmp_path / "closed_loop_cvar.npz") as z:
        assert sorted(z.files) == sorted(CL.KEYS) == sorted(("log_d", "log_f", "log_i", "cx", "cy", "mean", "done_tick"))
        assert z["log_f"].shape == (5, 4, 12) and z["done_tick"].tolist() == [-1, 2, 3, -1] and z["cy"].all()
    with pytest.raises(ValueError):
        CL.closed_loop(None, ["det"], None, np.zeros((4, 4)), 5, run=fake_run, goal_x=120.0)
    # no out_dir: nothing is written
    CL.closed_loop(None, ["saa"], None, np.zeros((4, 4)), 5, run=fake_run, log=lines.append, goal_x=120.0)
    assert len(lines) == 3 and not (tmp_path / "closed_loop_saa.npz").exists()


def test_log_columns_are_the_bindings(CL):
    from optimizer import _native
    assert _native.MPC_LOG_F[CL.CLEAR] == "clear" and _native.MPC_LOG_I[CL.LANE_OUT] == "lane_out"
    assert _native.MPC_LOG_I[CL.COLLIDED] == "collided" and _native.MPC_LOG_D[0] == "x"


@pytest.mark.parametrize("variant", ["static", "dynamic"])
def test_scenario_is_the_sweeps(CL, variant):
    from optimizer import sweep
    veh, keys = CL.scenario(variant, 3, 4)
    assert veh.shape == (3, 4, 4) and veh.dtype == F32 and keys.shape == (3,)
    for e in range(3):
        ob = sweep.obstacles(variant, e, 4)
        for j, k in enumerate(("x", "y", "vx", "vy")):
            assert np.array_equal(veh[e, :, j], np.asarray(ob[k], F32)), (e, k)
        assert keys[e] == ob["idx_mpc"]
    assert (veh[:, :, 2:] == 0).all() == (variant == "static")
    st = CL.starts_of(variant, 3)
    assert st.shape == (3, 4) and (st[:, 1] == (1.75 if variant == "static" else -1.75)).all() and (st[:, 2] == 5).all()


def test_command_line(CL, monkeypatch, tmp_path):
    """--host-step, --variant, --costs, --noise and the shapes reach the runner; the handle is closed."""
    from optimizer import cem
    seen = {}

    class Handle:
        def close(self):
            seen["closed"] = True

    class Prob:
        def __init__(self, *a, **kw):
            seen["ctor"] = (a, kw)
            self.handle = Handle()

        def run_episodes(self, cost, vehicles, starts, ticks, **kw):
            seen.setdefault("runs", []).append((cost, vehicles.shape, starts.shape, ticks, kw))
            E = starts.shape[0]
            return dict(log_d=np.zeros((ticks, E, 2)), log_f=np.zeros((ticks, E, 12), F32),
                        log_i=np.zeros((ticks, E, 4), np.int32), done_tick=np.full(E, -1, np.int32),
                        cx=np.zeros((ticks, E, 11), F32), cy=np.zeros((ticks, E, 11), F32),
                        mean=np.zeros((ticks, E, 8), F32))

    monkeypatch.setattr(cem, "CEM", Prob)
    out = tmp_path / "o"
    CL.main(["--variant", "dynamic", "--episodes", "2", "--ticks", "3", "--costs", "saa", "cvar", "--host-step",
             "--noise", "beta", "--num-obs", "2", "--out", str(out), "--goal-x", "90"])
    a, kw = seen["ctor"]
    assert a[1] == 2 and a[4] == "beta" and kw["variant"] == "dynamic" and kw["max_configs"] == 2
    assert [r[0] for r in seen["runs"]] == ["saa", "cvar"] and seen["closed"]
    cost, vs, ss, ticks, rkw = seen["runs"][0]
    assert (vs, ss, ticks) == ((2, 2, 4), (2, 4), 3)
    assert rkw["chained"] is False and rkw["device_step"] is None and rkw["goal_x"] == 90.0 and len(rkw["keys"]) == 2
    assert sorted(p.name for p in out.iterdir()) == ["closed_loop_cvar.npz", "closed_loop_saa.npz"]
    seen.clear()
    CL.main(["--episodes", "1", "--ticks", "1", "--costs", "mmd_random", "--out", str(out)])
    assert seen["runs"][0][4]["chained"] is True and seen["ctor"][1]["variant"] == "static"
