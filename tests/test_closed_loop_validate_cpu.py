"""The validation accounting of carla/closed_loop.py without a GPU: a fake
episode runner that returns val_* arrays with known values -- the figures of
the second line, the live-row mask after done_tick, the keys of the npz -- and
that without ``validate`` the files and lines are what test_closed_loop_cpu.py
pins.  Also the library's argument checks of the validation stage that need no
device (a NULL world) and the binding's symbols."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

from test_closed_loop_cpu import fake_run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CARLA = os.path.join(ROOT, "mpc-mmd_amd", "carla")
F32 = np.float32
R = 50
VAL = dict(rollouts=R, alpha=0.9, sigma=[0.1, 0.5])


@pytest.fixture(scope="module")
def CL():
    spec = importlib.util.spec_from_file_location("mpcmmd_carla_closed_loop_val", os.path.join(CARLA, "closed_loop.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def fake_val_run(prob, cost, route, goal_index, vehicles, starts, ticks, validate=None, **kw):
    """test_closed_loop_cpu's 4 episodes x 5 ticks (episode 1 done at tick 2, episode 2 at tick 3)
    with validation arrays whose rows after done_tick hold values that must not count."""
    res = fake_run(prob, cost, route, goal_index, vehicles, starts, ticks, **kw)
    assert validate == VAL
    T, E, S = int(ticks), 4, 2
    t = np.arange(T)[:, None]
    counts = np.zeros((T, E, 3), np.int32)
    counts[:, :, 2] = t * np.array([0, 5, 10, 1])          # count_rows
    cvar = np.zeros((T, E, 3), F32)
    cvar[:, :, 0] = 0.5 * t + np.array([0.0, 1.0, 2.0, 3.0])
    est = np.zeros((T, E, 2), F32)
    est[:, :, 1] = 0.25 * t * np.array([1.0, 2.0, 4.0, 0.0])
    counts[3:, 1, 2], cvar[3:, 1, 0], est[3:, 1, 1] = R, 1000.0, 1000.0   # frozen rows of episode 1
    counts[4:, 2, 2], cvar[4:, 2, 0], est[4:, 2, 1] = R, 1000.0, 1000.0   # and of episode 2
    z3 = np.zeros((T, E, 3), F32)
    res.update(val_counts=counts, val_count_pos=np.zeros((T, E, 3), np.int32), val_var=z3, val_cvar=cvar,
               val_mean=z3, val_max=z3, val_mmd=np.zeros((T, E, 3, S), F32), val_est=est)
    return res


def test_validation_accounting(CL, tmp_path):
    lines = []
    res = CL.closed_loop(None, ["cvar", "det"], None, 7, None, np.zeros((4, 4)), 5, out_dir=str(tmp_path),
                         run=fake_val_run, log=lines.append, seed=3, validate=VAL)
    s = res["cvar"][1]
    sd = lambda v: float(np.std(v, ddof=1))
    # per episode the mean over its live ticks (5, 3, 4, 5 of them), then mean and sd over the episodes
    p = [0.0, (0 + 5 + 10) / 3 / R, (0 + 10 + 20 + 30) / 4 / R, (0 + 1 + 2 + 3 + 4) / 5 / R]
    assert s["p_collision"] == pytest.approx((float(np.mean(p)), sd(p)), rel=1e-12)
    c = [1.0, 1.0 + 0.5, 2.0 + 0.75, 3.0 + 1.0]
    assert s["cvar_obs"] == pytest.approx((float(np.mean(c)), sd(c)), rel=1e-12)
    e = [0.25 * 2, 0.5 * 1, 1.0 * 1.5, 0.0]
    assert s["est_obs"] == pytest.approx((float(np.mean(e)), sd(e)), rel=1e-12)
    # the first line of each cost is the one without validation; the second is new
    assert len(lines) == 4 and lines[0].startswith("cvar: 4 episodes x 5 ticks, collision share = 0.2500 +- 0.5000")
    assert lines[1].startswith(f"cvar: plans under {R} fresh noise rows, mean collision probability = "
                               f"{np.mean(p):.4f} +- {sd(p):.4f}")
    assert f"mean validated CVaR(obs) = {np.mean(c):.4f} +- {sd(c):.4f}" in lines[1]
    assert f"mean solver cost_obs = {np.mean(e):.4f} +- {sd(e):.4f}" in lines[1]
    assert lines[2].startswith("det: 4 episodes") and lines[3].startswith("det: plans under")
    with np.load(tmp_path / "closed_loop_cvar.npz") as z:
        assert sorted(z.files) == sorted(CL.LOG_KEYS + CL.VAL_KEYS)
        assert z["val_mmd"].shape == (5, 4, 3, 2) and z["val_counts"].dtype == np.int32
        assert z["val_counts"][2, 1].tolist() == [0, 0, 10]


def test_without_validate_nothing_changes(CL, tmp_path):
    """The runner gets no ``validate`` keyword (fake_run asserts its keywords), the npz holds LOG_KEYS
    only and there is one line per cost, whatever else the result holds."""
    assert CL.LOG_KEYS == ("log_d", "log_f", "log_i", "done_tick", "collided", "goal")
    lines = []
    res = CL.closed_loop(None, ["cvar"], None, 7, None, np.zeros((4, 4)), 5, out_dir=str(tmp_path), run=fake_run,
                         log=lines.append, seed=3)
    assert len(lines) == 1 and "fresh noise rows" not in lines[0]
    assert sorted(res["cvar"][1]) == ["collision", "lane_departure", "min_neg_clear", "progress"]
    with np.load(tmp_path / "closed_loop_cvar.npz") as z:
        assert sorted(z.files) == sorted(CL.LOG_KEYS)


def test_all_episodes_done_at_tick_0(CL):
    """Only tick 0 is live: the figures are tick 0's, and a zero-tick mask divides by nothing."""
    T, E = 3, 2
    counts = np.full((T, E, 3), R, np.int32)
    counts[0, :, 2] = [10, 20]
    res = dict(done_tick=np.array([0, 0]), val_counts=counts, val_cvar=np.ones((T, E, 3), F32),
               val_est=np.full((T, E, 2), 2.0, F32))
    s = CL.summarise_validation(res, R)
    assert s["p_collision"][0] == pytest.approx(0.3) and s["cvar_obs"] == (1.0, 0.0) and s["est_obs"] == (2.0, 0.0)


def test_main_options(CL, monkeypatch):
    """--validate builds the runner's ``validate`` dict; without it the keyword is absent."""
    seen = []

    class Prob:
        def close(self):
            pass

    import types
    import sys
    fake_cem = types.SimpleNamespace(CEM=lambda *a, **k: Prob())
    monkeypatch.setitem(sys.modules, "optimizer", types.SimpleNamespace(cem=fake_cem))
    monkeypatch.setitem(sys.modules, "optimizer.cem", fake_cem)
    monkeypatch.setattr(CL, "closed_loop", lambda *a, **k: seen.append(k))
    monkeypatch.setattr(sys, "path", list(sys.path))
    CL.main(["--synthetic", "--episodes", "2", "--ticks", "3", "--costs", "cvar", "--validate", "1000",
             "--risk-sigma", "0.1", "0.2"])
    CL.main(["--synthetic", "--episodes", "2", "--ticks", "3", "--costs", "cvar"])
    assert seen[0]["validate"] == dict(rollouts=1000, alpha=0.98, sigma=[0.1, 0.2])
    assert "validate" not in seen[1] and seen[1]["chained"] is True


def test_library_checks_without_a_device():
    """The symbols exist, the binding declares them, and a NULL world is refused before any HIP call."""
    from optimizer import _native as nat
    L = nat.lib()
    for s in ("mpcmmd_world_validate", "mpcmmd_world_validation_log", "mpcmmd_world_validation_inputs"):
        assert s in nat.SYMBOLS and hasattr(L, s), s
    assert L.mpcmmd_abi_version() == 5
    assert C.sizeof(nat.WorldValidation) == 4 + 4 + 4 + 8 * 4
    cfg = nat.WorldValidation(100, 0.98, 0)
    assert L.mpcmmd_world_validate(None, C.byref(cfg)) < 0 and b"null" in L.mpcmmd_last_error()
    assert L.mpcmmd_world_validation_log(None, 0, None, None, None, None, None) < 0
    assert L.mpcmmd_world_validation_inputs(None, None, None, None, None, None, None, None) < 0
