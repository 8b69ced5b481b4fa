"""The validation accounting of optimizer/closed_loop.py (--validate) without a
GPU: a fake episode runner with a hand-made val_* set, the figures of the second line (live rows
only), the npz keys, that nothing changes without --validate, the option parsing, and the error
codes the new entry points return before any HIP call."""
import ctypes as C

import numpy as np
import pytest

F32 = np.float32
R = 200
VAL = dict(rollouts=R, alpha=0.9, sigma=[0.1], overlap=True)


@pytest.fixture(scope="module")
def CL():
    from optimizer import closed_loop
    return closed_loop


def fake_run(prob, cost, vehicles, starts, ticks, **kw):
    """3 episodes x 4 ticks.  Episode 0 runs through; 1 is done at tick 1 (its rows 2, 3 carry
    values that must not count); 2 is done at tick 0."""
    T, E = int(ticks), 3
    assert (T, E) == (4, np.asarray(starts).shape[0])
    out = dict(log_d=np.zeros((T, E, 2)), log_f=np.zeros((T, E, 12), F32), log_i=np.zeros((T, E, 4), np.int32),
               done_tick=np.array([-1, 1, 0], np.int32), cx=np.zeros((T, E, 11), F32), cy=np.zeros((T, E, 11), F32),
               mean=np.zeros((T, E, 8), F32))
    out["log_d"][:, :, 0] = np.arange(T)[:, None]
    val = kw.get("validate")
    if val is None:
        assert "validate" not in kw
        return out
    assert val == VAL
    pos = np.zeros((T, E, 3), np.int32)
    pos[:, :, 0] = [[0, 20, 200], [10, 60, 111], [20, 199, 111], [50, 199, 111]]   # the obs channel
    pos[:, :, 1:] = 7                                                              # lanes: not in the figures
    cnt = np.zeros((T, E, 2), np.int32)
    cnt[:, :, 0] = [[0, 10, 100], [4, 30, 111], [8, 199, 111], [28, 199, 111]]
    cnt[:, :, 1] = 9
    st = np.full((T, E, 4, 3), 77.0, F32)
    st[:, :, 1, 0] = [[0.0, 0.5, 2.0], [0.25, 1.5, 9.0], [0.5, 9.0, 9.0], [0.25, 9.0, 9.0]]   # cvar of obs
    est = np.full((T, E, 2), 55.0, F32)
    est[:, :, 1] = [[1.0, 3.0, 8.0], [2.0, 5.0, 9.0], [3.0, 9.0, 9.0], [6.0, 9.0, 9.0]]      # cost_obs
    out.update(val_counts=cnt, val_count_pos=pos, val_stats=st, val_mmd=np.full((T, E, 3, 1), -1000.0, F32), val_est=est)
    return out


def test_validation_accounting(CL, tmp_path):
    lines = []
    res = CL.closed_loop(None, ["cvar"], None, np.zeros((3, 4)), 4, out_dir=str(tmp_path), run=fake_run,
                         log=lines.append, validate=VAL)
    s = res["cvar"][1]
    sd = lambda v: float(np.std(v, ddof=1))
    ms = lambda v: (float(np.mean(v)), sd(v))
    # per episode the mean over its live ticks (4, 2 and 1 of them), then mean and sample sd over the episodes
    assert s["p_collision"] == pytest.approx(ms([(0 + 10 + 20 + 50) / 4 / R, (20 + 60) / 2 / R, 200 / R]), rel=1e-12)
    assert s["count_share"] == pytest.approx(ms([(0 + 4 + 8 + 28) / 4 / R, (10 + 30) / 2 / R, 100 / R]), rel=1e-12)
    assert s["cvar_obs"] == pytest.approx(ms([1.0 / 4, 2.0 / 2, 2.0]), rel=1e-12)
    assert s["est_obs"] == pytest.approx(ms([12.0 / 4, 8.0 / 2, 8.0]), rel=1e-12)
    assert {"collision", "min_neg_clear", "lane_departure", "progress"} <= set(s)
    assert len(lines) == 2 and lines[0].startswith("cvar: 3 episodes x 4 ticks, collision share = ")
    assert lines[1].startswith(f"cvar: plans under {R} fresh noise rows, mean collision probability = 0.4333 +- ")
    assert "mean count / R = 0.2167 +- " in lines[1] and "mean validated CVaR(obs) = 1.0833 +- " in lines[1]
    assert "mean solver cost_obs = 5.0000 +- " in lines[1]
    with np.load(tmp_path / "closed_loop_cvar.npz") as z:
        assert sorted(z.files) == sorted(CL.KEYS + CL.VAL_KEYS)
        assert CL.VAL_KEYS == ("val_counts", "val_count_pos", "val_stats", "val_mmd", "val_est")
        assert z["val_stats"].shape == (4, 3, 4, 3) and z["val_counts"].shape == (4, 3, 2)
        assert z["val_mmd"].shape == (4, 3, 3, 1) and z["val_count_pos"][3, 0, 0] == 50


def test_nothing_changes_without_validate(CL, tmp_path):
    """The first line and the KEYS arrays do not depend on the stage; without it there is no second
    line and no val_* array in the file."""
    plain, with_val = [], []
    a, b = tmp_path / "a", tmp_path / "b"
    r0 = CL.closed_loop(None, ["saa"], None, np.zeros((3, 4)), 4, out_dir=str(a), run=fake_run, log=plain.append)
    CL.closed_loop(None, ["saa"], None, np.zeros((3, 4)), 4, out_dir=str(b), run=fake_run, log=with_val.append,
                   validate=VAL)
    assert len(plain) == 1 and len(with_val) == 2 and plain[0] == with_val[0]
    assert sorted(r0["saa"][1]) == ["collision", "lane_departure", "min_neg_clear", "progress"]
    with np.load(a / "closed_loop_saa.npz") as za, np.load(b / "closed_loop_saa.npz") as zb:
        assert sorted(za.files) == sorted(CL.KEYS)
        for k in CL.KEYS:
            assert za[k].dtype == zb[k].dtype and za[k].tobytes() == zb[k].tobytes(), k


def test_options(CL):
    a = CL.parse_args([])
    assert a.validate is None and CL.validation_of(a) == {}
    a = CL.parse_args(["--validate", "1000"])
    assert CL.validation_of(a) == dict(validate=dict(rollouts=1000, alpha=0.98, sigma=[], overlap=True))
    a = CL.parse_args(["--validate", "50", "--alpha", "0.9", "--risk-sigma", "0.1", "0.5", "--no-overlap", "--host-step"])
    assert CL.validation_of(a) == dict(validate=dict(rollouts=50, alpha=0.9, sigma=[0.1, 0.5], overlap=False))
    assert a.host_step
    a = CL.parse_args(["--alpha", "0.5", "--risk-sigma", "0.1"])   # without --validate they select nothing
    assert CL.validation_of(a) == {}


def test_command_line_hands_validate_on(CL, monkeypatch, tmp_path):
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
            E = starts.shape[0]
            out = dict(log_d=np.zeros((ticks, E, 2)), log_f=np.zeros((ticks, E, 12), F32),
                       log_i=np.zeros((ticks, E, 4), np.int32), done_tick=np.full(E, -1, np.int32),
                       cx=np.zeros((ticks, E, 11), F32), cy=np.zeros((ticks, E, 11), F32),
                       mean=np.zeros((ticks, E, 8), F32))
            if "validate" in kw:
                S = len(kw["validate"]["sigma"])
                out.update(val_counts=np.zeros((ticks, E, 2), np.int32), val_count_pos=np.zeros((ticks, E, 3), np.int32),
                           val_stats=np.zeros((ticks, E, 4, 3), F32), val_mmd=np.zeros((ticks, E, 3, S), F32),
                           val_est=np.zeros((ticks, E, 2), F32))
            return out

    monkeypatch.setattr(cem, "CEM", Prob)
    out = tmp_path / "o"
    CL.main(["--episodes", "2", "--ticks", "3", "--costs", "cvar", "--out", str(out), "--validate", "64",
             "--risk-sigma", "0.1"])
    assert seen[0]["validate"] == dict(rollouts=64, alpha=0.98, sigma=[0.1], overlap=True) and seen[0]["chained"] is True
    with np.load(out / "closed_loop_cvar.npz") as z:
        assert z["val_mmd"].shape == (3, 2, 3, 1)
    CL.main(["--episodes", "2", "--ticks", "3", "--costs", "cvar", "--out", str(out)])
    assert "validate" not in seen[1]
    with np.load(out / "closed_loop_cvar.npz") as z:
        assert sorted(z.files) == sorted(CL.KEYS)


def test_null_context_error_codes():
    """The new entry points refuse a NULL context with MPCMMD_E_INVALID before any HIP call."""
    from optimizer import _native
    L = _native.lib()
    for s in ("mpcmmd_mpc_validate", "mpcmmd_mpc_validation_log", "mpcmmd_mpc_validation_inputs"):
        assert s in _native.SYMBOLS and hasattr(L, s)
    cfg = _native.MpcValidation(100, 0.98, 1)
    cfg.sigma[0] = 0.1
    cfg.overlap = 1
    assert C.sizeof(_native.MpcValidation) == 4 * 12
    assert L.mpcmmd_mpc_validate(None, C.byref(cfg)) == -1 and b"null" in L.mpcmmd_last_error()
    assert L.mpcmmd_mpc_validate(None, None) == -1
    cn, cp = np.zeros(2, np.int32), np.zeros(3, np.int32)
    st, mm, es = np.zeros(12, F32), np.zeros(3, F32), np.zeros(2, F32)
    ip = C.POINTER(C.c_int32)
    assert L.mpcmmd_mpc_validation_log(None, 1, cn.ctypes.data_as(ip), cp.ctypes.data_as(ip), _native._fptr(st),
                                       _native._fptr(mm), _native._fptr(es)) == -1
    assert L.mpcmmd_mpc_validation_inputs(None, None, None, None, None, None, None) == -1
