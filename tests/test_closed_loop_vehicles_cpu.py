"""The planned vehicles of optimizer/closed_loop.py (--vehicles planned) without
a GPU: the driver-seeded targets, a fake episode runner with a hand-made ``veh`` array, the figure
of the extra line (the last live tick only), the npz keys, and that without the option the keys
and the lines are what they were."""
import numpy as np
import pytest

F32 = np.float32


@pytest.fixture(scope="module")
def CL():
    from optimizer import _native, closed_loop
    assert hasattr(_native.lib(), "mpcmmd_mpc_plan_vehicles"), "the library lacks the planned vehicles"
    return closed_loop


def base(T, E):
    out = dict(log_d=np.zeros((T, E, 2)), log_f=np.zeros((T, E, 12), F32), log_i=np.zeros((T, E, 4), np.int32),
               done_tick=np.array([-1, 1, 0], np.int32)[:E], cx=np.zeros((T, E, 11), F32), cy=np.zeros((T, E, 11), F32),
               mean=np.zeros((T, E, 8), F32))
    out["log_d"][:, :, 0] = np.arange(T)[:, None]
    return out


def fake_run(prob, cost, vehicles, starts, ticks, **kw):
    """3 episodes x 4 ticks x 2 vehicles.  Episode 0 runs through; 1 is done at tick 1 (its rows 2, 3
    carry values that must not count); 2 is done at tick 0."""
    out = base(int(ticks), 3)
    if kw.get("planned") is None:
        assert "planned" not in kw
        return out
    veh = np.zeros((4, 3, 2, 6), F32)
    veh[..., 1] = 1.75
    veh[3, 0, :, 1] = [-1.3, -2.3]     # episode 0 at its last tick: one inside, one outside
    veh[1, 1, :, 1] = [-1.75, -2.2]    # episode 1 at done_tick 1: both inside
    veh[2:, 1, :, 1] = 9.0
    veh[0, 2, :, 1] = [1.75, -1.0]     # episode 2 at done_tick 0: none inside
    veh[1:, 2, :, 1] = -1.75
    out["veh"] = veh
    return out


def test_targets_are_the_drivers(CL):
    from optimizer.obs_data_generate_dynamic import obs_data
    tg = CL.vehicle_targets(3, 4)
    assert tg.shape == (3, 4, 2) and tg.dtype == F32 and (tg[..., 1] == F32(-1.75)).all()
    gen = obs_data(1)
    for e in range(3):
        for o in range(4):
            assert tg[e, o, 0] == gen.sampling_param(43 * e + 11 * o + 5)[0]
    assert np.unique(tg[..., 0]).size == 12 and (np.abs(tg[..., 0] - 6.0) < 0.6).all()


def test_vehicle_accounting(CL, tmp_path):
    lines = []
    pl = dict(target=CL.vehicle_targets(3, 2), acc=None)
    res = CL.closed_loop(None, ["cvar"], None, np.zeros((3, 4)), 4, out_dir=str(tmp_path), run=fake_run,
                         log=lines.append, planned=pl)
    s = res["cvar"][1]
    share = [0.5, 1.0, 0.0]
    assert s["in_lane"] == pytest.approx((float(np.mean(share)), float(np.std(share, ddof=1))), rel=1e-12)
    assert len(lines) == 2 and lines[0].startswith("cvar: 3 episodes x 4 ticks, collision share = ")
    assert lines[1] == ("cvar: planned vehicles, share inside |y + 1.75| < 0.5 at the last live tick = "
                        f"0.5000 +- {np.std(share, ddof=1):.4f}")
    with np.load(tmp_path / "closed_loop_cvar.npz") as z:
        assert sorted(z.files) == sorted(CL.KEYS + ("veh",)) and z["veh"].shape == (4, 3, 2, 6)


def test_nothing_changes_without_the_option(CL, tmp_path):
    plain, planned = [], []
    a, b = tmp_path / "a", tmp_path / "b"
    r0 = CL.closed_loop(None, ["saa"], None, np.zeros((3, 4)), 4, out_dir=str(a), run=fake_run, log=plain.append)
    CL.closed_loop(None, ["saa"], None, np.zeros((3, 4)), 4, out_dir=str(b), run=fake_run, log=planned.append,
                   planned=dict(target=CL.vehicle_targets(3, 2), acc=None))
    assert len(plain) == 1 and len(planned) == 2 and plain[0] == planned[0]
    assert sorted(r0["saa"][1]) == ["collision", "lane_departure", "min_neg_clear", "progress"]
    with np.load(a / "closed_loop_saa.npz") as za, np.load(b / "closed_loop_saa.npz") as zb:
        assert sorted(za.files) == sorted(CL.KEYS)
        for k in CL.KEYS:
            assert za[k].dtype == zb[k].dtype and za[k].tobytes() == zb[k].tobytes(), k


def test_options(CL):
    a = CL.parse_args([])
    assert a.vehicles == "constant" and CL.planned_of(a) == {}
    a = CL.parse_args(["--vehicles", "planned", "--episodes", "2", "--num-obs", "3"])
    p = CL.planned_of(a)
    assert set(p) == {"planned"} and p["planned"]["acc"] is None
    assert np.array_equal(p["planned"]["target"], CL.vehicle_targets(2, 3))
    with pytest.raises(SystemExit):
        CL.parse_args(["--vehicles", "parked"])


def test_command_line_hands_planned_on(CL, monkeypatch, tmp_path, capsys):
    from optimizer import cem
    seen = []

    class Handle:
        def close(self):
            pass

    class Prob:
        def __init__(self, *a, **kw):
            self.handle = Handle()

        def run_episodes(self, cost, vehicles, starts, ticks, **kw):
            seen.append(kw)
            E, O = starts.shape[0], vehicles.shape[1]
            out = base(ticks, E)
            out["done_tick"] = np.full(E, -1, np.int32)
            if "planned" in kw:
                out["veh"] = np.zeros((ticks, E, O, 6), F32)
                out["veh"][..., 1] = -1.75
            return out

    monkeypatch.setattr(cem, "CEM", Prob)
    out = tmp_path / "o"
    CL.main(["--variant", "dynamic", "--episodes", "2", "--ticks", "3", "--costs", "cvar", "--out", str(out),
             "--vehicles", "planned"])
    assert set(seen[0]["planned"]) == {"target", "acc"} and seen[0]["planned"]["acc"] is None
    assert np.array_equal(seen[0]["planned"]["target"], CL.vehicle_targets(2, 3)) and seen[0]["chained"] is True
    text = capsys.readouterr().out.strip().splitlines()
    assert len(text) == 2 and text[1].endswith("at the last live tick = 1.0000 +- 0.0000")
    with np.load(out / "closed_loop_cvar.npz") as z:
        assert sorted(z.files) == sorted(CL.KEYS + ("veh",)) and z["veh"].shape == (3, 2, 3, 6)
    CL.main(["--variant", "dynamic", "--episodes", "2", "--ticks", "3", "--costs", "cvar", "--out", str(out)])
    assert "planned" not in seen[1]
    text = capsys.readouterr().out.strip().splitlines()
    assert len(text) == 1
    with np.load(out / "closed_loop_cvar.npz") as z:
        assert sorted(z.files) == sorted(CL.KEYS)
