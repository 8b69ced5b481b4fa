"""Batched CARLA solves without a GPU: the accounting of
``validate_replay(replicas=E)`` with a fake batched solver, inputs, validator
and risk function, the two C symbols, and the sanitizer run of the batch
setup's host code (tests/native/carla_batch_host.cpp: carla_rows_batch slices,
the [G][6][kMaxPath] path image, the [G][2][O][100] det track image, staged
pieces independent of G)."""
import importlib.util
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mpc-mmd_amd")
CARLA = os.path.join(PKG, "carla")
F32 = np.float32
STRIDE = 100000


def _driver():
    spec = importlib.util.spec_from_file_location("mpcmmd_carla_validate_replay_batch",
                                                  os.path.join(CARLA, "validate_replay.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_symbols_and_abi():
    from optimizer import _native
    L = _native.lib()
    assert _native.ABI_VERSION == 5 and L.mpcmmd_abi_version() == 5
    for s in ("mpcmmd_carla_begin_batch", "mpcmmd_carla_solve_batch"):
        assert s in _native.SYMBOLS and hasattr(L, s)


def test_null_arguments_need_no_gpu():
    """A null handle, array or path list: MPCMMD_E_INVALID before any HIP call."""
    from optimizer import _native
    L = _native.lib()
    assert L.mpcmmd_carla_begin_batch(None, 1, 2, None, None, None, None, None, None, None, None) == -1
    assert L.mpcmmd_last_error()
    assert L.mpcmmd_carla_solve_batch(None, 1, 2, None, None, None, None, None, None, None, None, None) == -1


class _Fakes:
    """A fake batched solver (and the single one), inputs, validator and risk function that record their calls."""

    def __init__(self, D):
        self.D = D
        self.inputs_seen, self.batch_seen, self.single_seen, self.calls = [], [], [], []

    def inputs(self, rec_, prob, k):
        self.inputs_seen.append(k)
        return np.full(6, k, F32), np.full((2, 100), k, F32), np.zeros((2, 100), F32), dict(tick=k)

    @staticmethod
    def _plan(k, e, mean):
        # the plan names its tick and chain; mean_param grows by 1 + chain per tick
        return None, None, np.full(100, k + 1000 * e, F32), np.full(100, -k, F32), np.asarray(mean, F32) + F32(1 + e)

    def solve_batch(self, prob, cost, idx, inits, means, cov, xo, yo, v_des, paths):
        E = len(idx)
        self.batch_seen.append((cost, list(idx), [np.array(m) for m in means], float(v_des)))
        assert len(inits) == len(means) == len(xo) == len(yo) == len(paths) == E
        assert np.array_equal(cov, self.D.COV)
        k = idx[0]
        # the chains share the tick's inputs (computed once: the same objects)
        assert all(i is inits[0] for i in inits) and all(p is paths[0] for p in paths) and paths[0]["tick"] == k
        return [self._plan(k, e, means[e]) for e in range(E)]

    def solve(self, prob, cost, k, init, mean, cov, xo, yo, v_des, path):
        self.single_seen.append((cost, k))
        return self._plan(k, 0, mean)

    @staticmethod
    def _counts(plans):
        t = np.array([p["tick"] for p in plans])
        e = np.array([int(p["v_best"][0]) // 1000 for p in plans])
        rows = np.where((t + e) % 2 == 0, t, 0)    # (tick + chain) even: `tick` of the rollouts collide
        return dict(count=rows // 2, count_rows=rows, count_lane=t + 100 + e)

    def validate(self, prob, plans, num_rollouts, seed):
        self.calls.append([(p["tick"], p["key"], int(p["v_best"][0]) // 1000) for p in plans])
        return self._counts(plans)

    def risk_fn(self, prob, plans, num_rollouts, seed, alpha, sigma):
        self.calls.append([(p["tick"], p["key"], int(p["v_best"][0]) // 1000) for p in plans])
        out = self._counts(plans)
        K = len(plans)
        e = np.array([int(p["v_best"][0]) // 1000 for p in plans], F32)
        out.update(count_pos=np.zeros((K, 3), np.int32), var=np.zeros((K, 3), F32),
                   cvar=np.repeat(e[:, None], 3, axis=1), mean=np.zeros((K, 3), F32), max=np.zeros((K, 3), F32),
                   mmd=np.zeros((K, 3, sigma.size), F32))
        return out


def test_replicas_accounting(tmp_path):
    D = _driver()
    assert D.REPLICA_KEY_STRIDE == STRIDE
    rec = dict(ego=np.zeros((10, 6), F32))
    E, ticks = 3, [3, 4, 5, 6]
    fk = _Fakes(D)
    lines = []
    res = D.validate_replay(rec, object(), costs=("cvar", "det"), ticks=ticks, num_rollouts=8, out_dir=str(tmp_path),
                            seed=5, solve_batch=fk.solve_batch, validate=fk.validate, inputs=fk.inputs,
                            log=lines.append, replicas=E)
    # inputs once per (cost, tick); one batched solve per (cost, tick) with the keys k + 100000 e
    assert fk.inputs_seen == ticks * 2
    assert [(c, idx) for c, idx, *_ in fk.batch_seen] == \
        [(c, [k + STRIDE * e for e in range(E)]) for c in ("cvar", "det") for k in ticks]
    # mean_param per chain: restarts per cost, chain e grows by 1 + e per tick
    for i, (c, idx, means, v_des) in enumerate(fk.batch_seen):
        assert v_des == 10.0
        for e in range(E):
            assert np.array_equal(means[e], D.MEAN + F32((i % 4) * (1 + e))), (i, e)
    # one validation call per cost: E x ticks plans, chain-major, the tick as every chain's key
    want = [(k, k, e) for e in range(E) for k in ticks]
    assert fk.calls == [want, want]
    for cost in ("cvar", "det"):
        with np.load(tmp_path / f"validate_{cost}.npz") as z:
            assert sorted(z.files) == ["count", "count_lane", "count_rows", "num_rollouts", "replica_key_stride", "tick"]
            assert int(z["replica_key_stride"]) == STRIDE and int(z["num_rollouts"]) == 8
            for k in ("count", "count_rows", "count_lane", "tick"):
                assert z[k].shape == (E, 4), k
            assert np.array_equal(z["tick"], np.tile(ticks, (E, 1)))
            assert np.array_equal(z["count_rows"], [[0, 4, 0, 6], [3, 0, 5, 0], [0, 4, 0, 6]])
            assert np.array_equal(z["count"], [[0, 2, 0, 3], [1, 0, 2, 0], [0, 2, 0, 3]])
            assert np.array_equal(z["count_lane"], np.array(ticks)[None, :] + 100 + np.arange(E)[:, None])
            assert all(np.array_equal(z[k], res[cost][k]) for k in z.files)
    # the line: mean +- sample standard deviation over the chains.  share: 0.5 for every chain;
    # mean count_rows / R per chain: 10/32, 8/32, 10/32
    assert len(lines) == 2 and lines[0].startswith("cvar: 4 ticks x 3 replicas") and lines[1].startswith("det:")
    p = np.array([10 / 32, 8 / 32, 10 / 32])
    assert "0.5000 +- 0.0000" in lines[0]
    assert f"{p.mean():.6f} +- {p.std(ddof=1):.6f}" in lines[0]


def test_replicas_risk_line_and_shapes(tmp_path):
    D = _driver()
    rec = dict(ego=np.zeros((10, 6), F32))
    fk = _Fakes(D)
    lines = []
    res = D.validate_replay(rec, object(), costs=("cvar",), ticks=[1, 2], num_rollouts=4, out_dir=str(tmp_path),
                            solve_batch=fk.solve_batch, risk_fn=fk.risk_fn, inputs=fk.inputs, log=lines.append,
                            risk=True, risk_sigma=(0.5, 1.0), replicas=2)
    out = res["cvar"]
    assert len(fk.calls) == 1 and len(fk.calls[0]) == 4
    assert out["risk_cvar"].shape == (2, 2, 3) and out["risk_mmd"].shape == (2, 2, 3, 2)
    assert out["risk_count_pos"].shape == (2, 2, 3) and out["count_rows"].shape == (2, 2)
    assert np.array_equal(out["risk_cvar"][:, :, 0], [[0, 0], [1, 1]])
    # obstacle CVaR per chain 0 and 1: mean 0.5, sample standard deviation sqrt(0.5)
    assert len(lines) == 2 and f"= 0.500000 +- {np.sqrt(0.5):.6f}" in lines[1]


def test_replicas_one_is_the_current_function(tmp_path):
    """replicas=1 takes the single-chain path: files and lines equal a run with ``replicas`` left out."""
    D = _driver()
    rec = dict(ego=np.zeros((10, 6), F32))
    outs = []
    for kw, sub in ((dict(), "a"), (dict(replicas=1), "b")):
        fk = _Fakes(D)
        lines = []
        res = D.validate_replay(rec, object(), costs=("cvar", "det"), ticks=range(3, 7), num_rollouts=8,
                                out_dir=str(tmp_path / sub), seed=5, solve=fk.solve, solve_batch=fk.solve_batch,
                                validate=fk.validate, inputs=fk.inputs, log=lines.append, **kw)
        assert fk.batch_seen == [] and len(fk.single_seen) == 8
        outs.append((res, lines, fk.calls))
    (ra, la, ca), (rb, lb, cb) = outs
    assert la == lb and ca == cb
    for cost in ("cvar", "det"):
        assert sorted(ra[cost]) == sorted(rb[cost]) == ["count", "count_lane", "count_rows", "num_rollouts", "tick"]
        assert ra[cost]["count_rows"].shape == (4,)
        with np.load(tmp_path / "a" / f"validate_{cost}.npz") as za, np.load(tmp_path / "b" / f"validate_{cost}.npz") as zb:
            assert za.files == zb.files and all(np.array_equal(za[k], zb[k]) and za[k].dtype == zb[k].dtype
                                                for k in za.files)


def test_replicas_chain0_is_the_single_chain():
    """Chain 0 of E chains sees the keys, means and plans of the single chain."""
    D = _driver()
    rec = dict(ego=np.zeros((10, 6), F32))
    f1, f3 = _Fakes(D), _Fakes(D)
    r1 = D.validate_replay(rec, object(), costs=("cvar",), ticks=range(2, 6), num_rollouts=8, solve=f1.solve,
                           validate=f1.validate, inputs=f1.inputs, log=lambda s: None)
    r3 = D.validate_replay(rec, object(), costs=("cvar",), ticks=range(2, 6), num_rollouts=8,
                           solve_batch=f3.solve_batch, validate=f3.validate, inputs=f3.inputs, log=lambda s: None,
                           replicas=3)
    for k in ("count", "count_rows", "count_lane", "tick"):
        assert np.array_equal(r3["cvar"][k][0], r1["cvar"][k]), k
    assert [idx[0] for _, idx, *_ in f3.batch_seen] == [k for _, k in f1.single_seen]


def test_replicas_tick_limit():
    D = _driver()
    rec = dict(ego=np.zeros((10, 6), F32))
    fk = _Fakes(D)
    with pytest.raises(ValueError, match="100000"):
        D.validate_replay(rec, object(), costs=("cvar",), ticks=[5, STRIDE], solve_batch=fk.solve_batch,
                          validate=fk.validate, inputs=fk.inputs, replicas=2)
    assert fk.batch_seen == [] and fk.inputs_seen == [], "refused before any solve"
    with pytest.raises(ValueError):
        D.validate_replay(rec, object(), costs=("cvar",), ticks=[5], solve_batch=fk.solve_batch,
                          validate=fk.validate, inputs=fk.inputs, replicas=0)
    # the largest tick allowed
    D.validate_replay(rec, object(), costs=("cvar",), ticks=[STRIDE - 1], solve_batch=fk.solve_batch,
                      validate=fk.validate, inputs=fk.inputs, replicas=2, log=lambda s: None)
    assert fk.batch_seen[0][1] == [STRIDE - 1, 2 * STRIDE - 1]


def test_batch_setup_host_program_under_sanitizers():
    """`make asan_batch` builds tests/native/carla_batch_host.cpp with the host-only sources under
    ASan / UBSan (-fno-sanitize-recover); its run, a child process with nothing preloaded, must exit 0
    with no sanitizer report."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    subprocess.run(["make", "-C", PKG, "asan_batch"], check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(PKG, "build_asan", "carla_batch_host")], capture_output=True, text=True, env=env,
                       timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.strip().splitlines()[-1] == "ok"
