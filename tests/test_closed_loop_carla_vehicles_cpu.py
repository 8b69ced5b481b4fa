"""The routed vehicles of carla/closed_loop.py (--vehicles routed) without a
GPU: the traffic seeded from the episodes' keys, a fake episode runner with a hand-made ``veh``
array, the three figures of the extra line, the npz keys, the command line, and that without the
option the keys, the lines and the runner's arguments are what they were."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CARLA = os.path.join(ROOT, "mpc-mmd_amd", "carla")
F32 = np.float32


@pytest.fixture(scope="module")
def CL():
    spec = importlib.util.spec_from_file_location("mpcmmd_carla_closed_loop_vehicles",
                                                  os.path.join(CARLA, "closed_loop.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert hasattr(mod, "routed_traffic"), "closed_loop.py lacks the routed vehicles"
    return mod


def base(T, E):
    out = dict(log_d=np.zeros((T, E, 3)), log_f=np.zeros((T, E, 13), F32), log_i=np.zeros((T, E, 4), np.int32),
               done_tick=np.array([-1, 1, 0], np.int32)[:E], collided=np.zeros(E, bool), goal=np.zeros(E, bool))
    out["log_f"][:, :, 11] = -1.0
    return out


ROUTED = dict(s=np.zeros((3, 3)), v=np.zeros((3, 3), F32), d=np.tile(np.array([0.0, -3.5, 0.5], F32), (3, 1)),
              v0=np.ones((3, 3), F32))


def fake_run(prob, cost, route, goal_index, vehicles, starts, ticks, **kw):
    """3 episodes x 4 ticks x 3 vehicles (lanes 0, -3.5, 0.5: vehicles 0 and 2 share a lane).  Episode 0
    runs through; 1 is done at tick 1 (its rows 2, 3 carry values that must not count); 2 at tick 0."""
    out = base(int(ticks), 3)
    # the ego: episode 0 on lane 0.25 at arc 20 on ticks 1 and 2 (between vehicles 0 and 2: it leads 0), at
    # arc 40 on tick 3 (ahead of everything, vehicle 2 leads 0, the ego leads 2), behind everybody on tick 0
    out["log_d"][:, 0, 2] = [5.0, 20.0, 20.0, 40.0]
    out["log_f"][:, 0, 12] = 0.25
    out["log_d"][:, 1, 2] = 20.0                  # episode 1: on the other lane's far side, never a leader
    out["log_f"][:, 1, 12] = 3.0
    out["log_d"][:, 2, 2] = 11.0                  # episode 2, tick 0 only: leads vehicle 1 (lane -3.5)? no: d = -6
    out["log_f"][:, 2, 12] = -6.0
    if kw.get("routed") is None:
        assert "routed" not in kw
        return out
    veh = np.zeros((4, 3, 3, 3))
    veh[:, :, :, 0] = [10.0, 12.0, 30.0]          # vehicle 2 leads vehicle 0: gap 30 - 10 - 4.5 = 15.5
    veh[:, 0, :, 1] = [[1, 1, 1], [2, 2, 2], [3, 3, 3], [4, 4, 4]]   # episode 0: mean speed 2.5
    veh[3, 0, :, 0] = [10.0, 12.0, 16.0]          # ... and at tick 3 the gap is 1.5
    veh[:2, 1, :, 1] = 6.0                        # episode 1, live ticks 0 and 1: 6
    veh[2:, 1, :, 1] = 100.0
    veh[2:, 1, :, 0] = [10.0, 12.0, 14.6]         # not counted: a gap of 0.1 after the episode froze
    veh[0, 2, :, 1] = 0.5
    out["veh"] = veh
    return out


def test_traffic_is_seeded_from_the_keys(CL):
    route, goal, vehicles = CL.synthetic_world("Town05")
    starts = CL.synthetic_starts(route, 3, spread=9.0)
    rt = CL.routed_traffic(route, starts)
    offs, lanes = CL._replay().SPAWN["Town05"]
    assert rt["s"].shape == (3, 10) and rt["s"].dtype == np.float64 and rt["v0"].dtype == F32
    assert np.allclose(rt["s"] - offs[None], np.array([0.0, 3.0, 6.0])[:, None], atol=1e-9)
    assert np.array_equal(rt["d"][1], np.array([lanes[i % 2] for i in range(10)], F32)) and not rt["v"].any()
    for e in range(3):
        p = np.random.default_rng(100000 * e).choice((0.4, 0.6, 0.4), 10)
        assert np.array_equal(rt["v0"][e], ((1.0 - p) * 8.33).astype(F32))
    assert set(np.unique(rt["v0"])) == {F32(0.6 * 8.33), F32(0.4 * 8.33)}
    assert not np.array_equal(rt["v0"][0], rt["v0"][1]), "every episode its own draw"
    other = CL.routed_traffic(route, starts, speed_limit=10.0, key_base=7)
    assert set(np.unique(other["v0"])) == {F32(6.0), F32(4.0)} and not np.array_equal(other["v0"] > 5, rt["v0"] > 4)
    # the spawns of the parked scene are those vehicles at rest
    assert np.allclose(CL._replay().Route(*route).at(rt["s"][0], rt["d"][0].astype(float))[0], vehicles[:, 0], atol=1e-3)


def test_vehicle_accounting(CL, tmp_path):
    lines = []
    res = CL.closed_loop(None, ["cvar"], None, 7, None, np.zeros((3, 4)), 4, out_dir=str(tmp_path), run=fake_run,
                         log=lines.append, routed=ROUTED)
    s = res["cvar"][1]
    speed = [2.5, 6.0, 0.5]
    assert s["vehicle_speed"] == pytest.approx((float(np.mean(speed)), float(np.std(speed, ddof=1))), rel=1e-12)
    assert s["min_gap"] == pytest.approx(1.5, abs=1e-12), "the frozen rows' 0.1 m does not count"
    assert s["ego_led"] == 3, "episode 0 on ticks 1, 2 (vehicle 0) and 3 (vehicle 2)"
    assert len(lines) == 2 and lines[0].startswith("cvar: 3 episodes x 4 ticks, collision share = ")
    assert lines[1] == (f"cvar: routed vehicles, mean speed = 3.0000 +- {np.std(speed, ddof=1):.4f} m/s, "
                        "smallest bumper gap = 1.5000 m, ticks with the ego as a leader = 3")
    with np.load(tmp_path / "closed_loop_cvar.npz") as z:
        assert sorted(z.files) == sorted(CL.LOG_KEYS + ("veh",)) and z["veh"].shape == (4, 3, 3, 3)
        assert z["veh"].dtype == np.float64


def test_nothing_changes_without_the_option(CL, tmp_path):
    plain, routed = [], []
    a, b = tmp_path / "a", tmp_path / "b"
    r0 = CL.closed_loop(None, ["det"], None, 7, None, np.zeros((3, 4)), 4, out_dir=str(a), run=fake_run,
                        log=plain.append)
    CL.closed_loop(None, ["det"], None, 7, None, np.zeros((3, 4)), 4, out_dir=str(b), run=fake_run, log=routed.append,
                   routed=ROUTED)
    assert len(plain) == 1 and len(routed) == 2 and plain[0] == routed[0]
    assert sorted(r0["det"][1]) == ["collision", "lane_departure", "min_neg_clear", "progress"]
    with np.load(a / "closed_loop_det.npz") as za, np.load(b / "closed_loop_det.npz") as zb:
        assert sorted(za.files) == sorted(CL.LOG_KEYS)
        for k in CL.LOG_KEYS:
            assert za[k].dtype == zb[k].dtype and za[k].tobytes() == zb[k].tobytes(), k


def test_options(CL):
    a = CL.parse_args(["--synthetic"])
    assert a.vehicles == "parked" and a.speed_limit == 8.33
    a = CL.parse_args(["--synthetic", "--vehicles", "routed", "--speed-limit", "12.5"])
    assert a.vehicles == "routed" and a.speed_limit == 12.5
    with pytest.raises(SystemExit):
        CL.parse_args(["--synthetic", "--vehicles", "planned"])
    with pytest.raises(SystemExit):
        CL.parse_args([])


def test_command_line_hands_routed_on(CL, monkeypatch, tmp_path, capsys):
    import sys
    seen = []

    class Prob:
        def __init__(self, *a, **kw):
            pass

        def close(self):
            pass

        def run_episodes(self, cost, route, vehicles, starts, ticks, **kw):
            seen.append(kw)
            E = starts.shape[0]
            out = base(ticks, E)
            out["done_tick"] = np.full(E, -1, np.int32)
            if "routed" in kw:
                V = kw["routed"]["s"].shape[1]
                out["veh"] = np.zeros((ticks, E, V, 3))
                out["veh"][..., 0] = kw["routed"]["s"][None]
                out["veh"][..., 1] = 2.0
            return out

    fake = type(sys)("optimizer")
    fake.cem = type(sys)("optimizer.cem")
    fake.cem.CEM = Prob
    monkeypatch.setitem(sys.modules, "optimizer", fake)
    monkeypatch.setitem(sys.modules, "optimizer.cem", fake.cem)
    monkeypatch.setattr(sys, "path", list(sys.path))
    out = tmp_path / "o"
    CL.main(["--synthetic", "--episodes", "2", "--ticks", "3", "--costs", "cvar", "--out", str(out),
             "--vehicles", "routed", "--speed-limit", "10"])
    rt = seen[0]["routed"]
    assert set(rt) == {"s", "v", "d", "v0"} and rt["s"].shape == (2, 10) and seen[0]["chained"] is True
    assert set(np.unique(rt["v0"])) <= {F32(6.0), F32(4.0)}
    text = capsys.readouterr().out.strip().splitlines()
    # offsets 50, 70 (other lane), 95: the smallest gap on one lane is 105 - 95 - 4.5 on lane -3.5? lanes alternate:
    # lane 0 holds 50, 95, 130, 160, 180; lane -3.5 holds 70, 105, 150, 170, 190: 180 - 160 - 4.5 = 15.5
    assert len(text) == 2 and text[1] == ("cvar: routed vehicles, mean speed = 2.0000 +- 0.0000 m/s, smallest bumper "
                                          "gap = 15.5000 m, ticks with the ego as a leader = 0")
    with np.load(out / "closed_loop_cvar.npz") as z:
        assert sorted(z.files) == sorted(CL.LOG_KEYS + ("veh",)) and z["veh"].shape == (3, 2, 10, 3)
    CL.main(["--synthetic", "--episodes", "2", "--ticks", "3", "--costs", "cvar", "--out", str(out)])
    assert "routed" not in seen[1]
    assert len(capsys.readouterr().out.strip().splitlines()) == 1
    with np.load(out / "closed_loop_cvar.npz") as z:
        assert sorted(z.files) == sorted(CL.LOG_KEYS)
