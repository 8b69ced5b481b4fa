"""The library's host arithmetic (csrc/solve_host.cpp, csrc/carla_host.cpp)
on the CPU: the sanitizer harness (tests/native/asan_host.cpp, built by `make
-C mpc-mmd_amd asan`) runs every function at the smallest shapes where its
indexing can go wrong and records inputs and results; here they are held
against the oracle, at the bounds the GPU tests apply to the same quantities
(initial population: test_gpu_parity_baseline.py, rtol = atol = 1e-6; noisy
initial rows: test_gpu_carla.py, bit-equal; KKT columns: the fp64 product of
the oracle's KKT inverse with the oracle's boundary vectors, exact, as
test_asan_host.py holds the constants), and the pure permutations against a few
lines of NumPy, exactly.  No GPU."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mpc-mmd_amd")
sys.path[:0] = [ROOT, PKG]

from oracle import carla as K  # noqa: E402
from oracle import helper as Hh  # noqa: E402
from oracle.problem import Problem  # noqa: E402
from parity import close  # noqa: E402

F32, F64 = np.float32, np.float64
DTYPES = {"f32": F32, "f64": F64, "i32": np.int32}
BEGIN = [(2, 1), (100, 32)]                          # (H, O)
CARLA = [(2, 2, 1, 4), (4, 100, 32, 50), (6, 100, 32, 50)]   # (n, H, O, num_path)


@pytest.fixture(scope="module")
def rec(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    subprocess.run(["make", "-C", PKG, "asan"], check=True, capture_output=True)
    out = tmp_path_factory.mktemp("solve_host") / "record.txt"
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(PKG, "build_asan", "asan_host"), str(out)], capture_output=True, text=True,
                       env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    got = {}
    for ln in out.read_text().splitlines():
        name, ty, cnt, *vals = ln.split()
        assert len(vals) == int(cnt), name
        # decimal text with 9 / 17 significant digits round-trips fp32 / fp64
        got[name] = np.array([float(v) for v in vals], F64).astype(DTYPES[ty])
    return got


@pytest.fixture(scope="module")
def problems():
    cache = {}

    def get(H, O, variant="static", n=4):
        key = (H, O, variant, n)
        if key not in cache:
            cache[key] = Problem(n, O, 0.1, H, "gaussian", 0.0, 0.0, num_batch=20, variant=variant)
        return cache[key]
    return get


def _path(rec, P):
    c = f"path.P{P}/"
    return {k: rec[c + s] for k, s in (("x_path", "x"), ("y_path", "y"), ("arc_vec", "arc_vec"),
                                       ("Fx_dot", "Fx_dot"), ("Fy_dot", "Fy_dot"), ("kappa", "kappa"))}


@pytest.mark.parametrize("P", [4, 50])
def test_path_helpers_match_library(rec, P):
    """carla_host.cpp under the sanitizer == the product library's
    mpcmmd_path_* / mpcmmd_global_to_frenet (which test_carla_host.py holds
    against the oracle), bit for bit, at the minimum num_path and a short one."""
    from optimizer import _native
    c = f"path.P{P}/"
    xs, ys = _native.path_smoothing(rec[c + "x_wp"], rec[c + "y_wp"], 0.1)
    assert np.array_equal(xs, rec[c + "x"]) and np.array_equal(ys, rec[c + "y"])
    lib = _native.path_parameters(rec[c + "x"], rec[c + "y"])
    for a, name in zip(lib, ("Fx_dot", "Fy_dot", "Fx_ddot", "Fy_ddot", "arc_vec", "kappa", "arc_length")):
        assert np.array_equal(np.asarray(a, F32).reshape(-1), rec[c + name]), name
    pts = rec[c + "points"].reshape(-1, 6)
    got = _native.global_to_frenet(_path(rec, P), *(np.ascontiguousarray(pts[:, k]) for k in range(6)))
    assert np.array_equal(np.stack(got, axis=1), rec[c + "frenet"].reshape(-1, 7))


@pytest.mark.parametrize("H,O", BEGIN)
def test_handle_constants(rec, problems, H, O):
    p, c = problems(H, O), f"begin.H{H}.O{O}/"
    assert np.array_equal(rec[c + "basis"].reshape(3, 100, 11), np.stack([p.P, p.Pdot, p.Pddot]).astype(F32))
    assert np.array_equal(rec[c + "guess_g"].reshape(2, 11, 4), p.guess_G)
    pm = np.stack([p.proj_kinv_x[:11, :11], p.proj_kinv_y[:11, :11]])
    assert np.array_equal(rec[c + "proj_m"].reshape(2, 11, 11), pm)


@pytest.mark.parametrize("H,O", BEGIN)
def test_begin_quantities(rec, problems, H, O):
    p, c = problems(H, O), f"begin.H{H}.O{O}/"
    init = rec[c + "init_state"]
    # boundary vectors -> the four KKT columns, exact
    bx, by = Hh.compute_boundary_vec(p, init)
    ref = np.stack([p.kkt_rhs_const(p.guess_kinv_x, bx), p.kkt_rhs_const(p.guess_kinv_y, by),
                    p.kkt_rhs_const(p.proj_kinv_x, bx), p.kkt_rhs_const(p.proj_kinv_y, by)])
    assert np.array_equal(rec[c + "solve_c"].reshape(4, 11), ref)
    # st0 = (x, y, vx, vy, atan2f(vy, vx), 0, 0, 0); the heading within an ulp of pi of the fp64 value
    st0 = rec[c + "st0"]
    assert np.array_equal(st0[:4], init[:4]) and np.all(st0[5:] == 0)
    assert abs(float(st0[4]) - np.arctan2(float(init[3]), float(init[2]))) <= 2.4e-7
    # obstacle tracks [O][100] -> [2][O][H]
    ob = np.stack([rec[c + "x_obs"].reshape(O, 100)[:, :H], rec[c + "y_obs"].reshape(O, 100)[:, :H]])
    assert np.array_equal(rec[c + "obs"].reshape(2, O, H), ob)
    # external noise rows [T][3][S][H] -> [T][3][H][S]
    roll = rec[c + "roll"].reshape(1, 3, 3, H)
    assert np.array_equal(rec[c + "roll_t"].reshape(1, 3, H, 3), roll.transpose(0, 1, 3, 2))
    # initial population: sampling_param, both clips met in the second
    z, cov, mean = rec[c + "z"].reshape(20, 8), rec[c + "cov"].reshape(8, 8), rec[c + "mean"].reshape(2, 8)
    pop = rec[c + "pop"].reshape(2, 20, 8)
    for g in range(2):
        close(f"pop[{g}]", pop[g], Hh.sampling_param(p, mean[g], cov, z), rtol=1e-6, atol=1e-6)
    assert (pop[1, :, :4] == F32(0.1)).any() and (pop[1, :, :4] == F32(30.0)).any()
    assert rec[c + "not_pd_threw"][0] == 1


@pytest.mark.parametrize("H,O", BEGIN)
def test_plan_speed_and_controls(rec, problems, H, O):
    p, c = problems(H, O), f"begin.H{H}.O{O}/"
    # v_best = sqrt(xd^2 + yd^2), xd = fp32(sum_k Pdot[i][k] cx[k]) in fp64, sequential
    Pd = p.Pdot.astype(F64)
    sx, sy = np.zeros(100), np.zeros(100)
    for k in range(11):
        sx = sx + Pd[:, k] * F64(rec[c + "cx"][k])
        sy = sy + Pd[:, k] * F64(rec[c + "cy"][k])
    xd, yd = sx.astype(F32), sy.astype(F32)
    assert np.array_equal(rec[c + "v_best"], np.sqrt(xd * xd + yd * yd))
    # compute_controls: acc = diff([v, v_end]) / t over the first H plan points
    v, steer = rec[c + "plan_v"].reshape(2, 100), rec[c + "plan_steer"].reshape(2, 100)
    vn = np.concatenate([v[:, 1:], v[:, -1:]], axis=1)
    assert np.array_equal(rec[c + "plan_acc"].reshape(2, H), ((vn - v) / F32(0.15))[:, :H])
    assert np.array_equal(rec[c + "plan_steer_h"].reshape(2, H), steer[:, :H])


@pytest.mark.parametrize("n,H,O,P", CARLA)
def test_carla_rows_and_columns(rec, n, H, O, P):
    ora = K.CarlaCEM(n, 1, O, 0.1, H, "gaussian", "Town05", 0.0, 0.0, num_batch=20, maxiter_cem=1)
    p, path = ora.prob, _path(rec, P)
    for R in (1, n, n * n):
        c = f"carla.n{n}.R{R}/"
        init, eps = rec[c + "init_state"], rec[c + "eps"].reshape(R, 4)
        rows = rec[c + "rows"].reshape(n * n, 8)
        st = ora.noisy_init(init, eps)
        assert np.array_equal(rows[:R, :5], st), "noisy initial rows differ"
        assert np.all(rows[:R, 5:] == 0) and np.all(rows[R:] == 0)
        assert np.array_equal(rec[c + "velocity_heading"], st[0, 2:5])
        bx, by = ora.boundary(path, init, st)
        assert np.array_equal(rec[c + "bx"], bx.astype(F64)) and np.array_equal(rec[c + "by"], by.astype(F64))
        kx, ky = p.det_kinv() if R == 1 else (p.proj_kinv_x, p.proj_kinv_y)
        ref = np.stack([p.kkt_rhs_const(p.guess_kinv_x, bx), p.kkt_rhs_const(p.guess_kinv_y, by),
                        p.kkt_rhs_const(kx, bx), p.kkt_rhs_const(ky, by)])
        assert np.array_equal(rec[c + "solve_c"].reshape(4, 11), ref)
        if R == 1:
            assert np.array_equal(rec[c + "proj_m_det"].reshape(2, 11, 11), np.stack([kx[:11, :11], ky[:11, :11]]))


@pytest.mark.parametrize("n", [2, 4, 6])
def test_first_selection_tables(rec, n):
    c, M, npair = f"beta.n{n}/", n * n, 100 * n
    sel, sig = rec[c + "sel"], rec[c + "sig"]
    rp, pairs, rperm = rec[c + "rp0"], rec[c + "rpair0"].reshape(npair, 2), rec[c + "rperm"]
    assert rp.shape == (M + 1,) and rp[0] == 0 and rp[-1] == npair and np.all(np.diff(rp) >= 0)
    assert np.array_equal(np.sort(pairs[:, 0]), np.arange(npair))       # each pair once
    row_of = np.repeat(np.arange(M), np.diff(rp))
    assert np.array_equal(sel[pairs[:, 0]], row_of)                      # under its row
    assert np.array_equal(pairs[:, 1], sig.view(np.int32)[pairs[:, 0] // n])   # with its sample's sigma bits
    for r in range(M):                                                   # in draw order within a row
        assert np.all(np.diff(pairs[rp[r]:rp[r + 1], 0]) > 0)
    nsig = np.array([np.unique(pairs[rp[r]:rp[r + 1], 1]).size for r in range(M)])
    assert nsig[0] == 0 and nsig[1] == 1 and nsig.max() > 1             # no pair; one sigma; several
    assert np.array_equal(rperm, np.argsort(-nsig, kind="stable"))
    assert rec[c + "range_threw"][0] == 1


def _bz_index(j, s):
    jj = j & 15
    lane = ((s & 31) >> 1) + 16 * (jj & 3)
    idx = 6 * (jj >> 2) + 2 * (s >> 5) + (s & 1)
    return (j >> 4) * (16 * 96) + (idx >> 2) * 256 + lane * 4 + (idx & 3)


@pytest.mark.parametrize("n,pos_pad", [(2, 32), (4, 32), (6, 64)])
def test_beta_z_image(rec, n, pos_pad):
    M1, R = n * n + 1, 89
    img = rec[f"beta.n{n}/beta_z"]
    assert img.size == pos_pad * 96
    r, j = np.meshgrid(np.arange(R), np.arange(M1), indexing="ij")
    at = _bz_index(j, r)
    assert np.unique(at).size == R * M1 and at.max() < img.size          # no two on one slot
    z = (np.arange(R * M1) + 1).astype(F32).reshape(R, M1)
    assert np.array_equal(img[at], z)
    rest = np.ones(img.size, bool)
    rest[at.reshape(-1)] = False
    assert np.all(img[rest] == 0)
