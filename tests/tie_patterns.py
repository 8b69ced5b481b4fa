"""Inputs with exact ties and special values for the device selections
("Exact ties and special values"): sample rows for the
beta-CEM's top-n |beta| selection, a NumPy model of ``select_walk``'s dispatch
that labels which path a row takes, two-level beta-CEM draws whose ties survive
the elite mean, and Frenet closest-point cases with bit-equal (or sqrtf-equal)
distances.  Plain module like parity.py; the expected values of the GPU tests
come from the oracle, never from here.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from oracle import carla as K

F32 = np.float32
F64 = np.float64
SQRT20 = np.sqrt(20.0)

# launch_bselect's table (csrc/k_bsample.hip): largest n of the instance, keys
# per lane NQ, window capacity / 64 R, groups of the window threshold G (0: the
# bisection)
BSELECT_TABLE = ((8, 1, 1, 32), (11, 2, 1, 32), (16, 4, 1, 32), (22, 8, 1, 32), (24, 12, 1, 32), (27, 12, 2, 64),
                 (32, 16, 2, 64), (39, 24, 2, 64), (45, 32, 2, 64), (48, 40, 2, 64), (50, 40, 2, 0), (55, 48, 2, 0),
                 (64, 64, 2, 0))
BSELECT_N = tuple(r[0] for r in BSELECT_TABLE)


def bselect_instance(n):
    """(NQ, R, G) of the k_bselect instance that serves n."""
    for top, NQ, R, G in BSELECT_TABLE:
        if n <= top:
            return NQ, R, G
    raise ValueError(n)


def scaled(z0):
    """The first beta-iteration's samples of the draws z0: float32(sqrt(20) z0)."""
    return (SQRT20 * np.asarray(z0, F32).astype(F64)).astype(F32)


def abs_keys(row, M):
    """sort_key_abs of row[:M] (csrc/common.hpp)."""
    a = np.abs(np.asarray(row[:M], F32))
    u = a.view(np.uint32).astype(np.uint64)
    return np.where(np.isnan(a), np.uint64(0xFFFFFFFF), u | np.uint64(0x80000000))


def group_of(j, G):
    """Window-threshold group of key index j: lane j % 64, groups of 64 / G lanes."""
    return (np.asarray(j) % 64) // (64 // G)


def max_keys_per_group(M, G):
    return int(np.bincount(group_of(np.arange(M), G), minlength=G).max())


def select_path(row, M, n, NQ, R, G):
    """Which path of select_walk (csrc/betacem_select.hpp) the row takes:
    window_all (every key a candidate), window_group (the group-maxima window
    holds), overflow_exact (bisection that ends with exactly n keys above the
    threshold) or overflow_ties (bisection to the last bit: emit_top's tie
    branch).  Labels coverage only."""
    assert M <= 64 * NQ
    key = abs_keys(row, M)
    cap = 64 * R
    if M <= cap:
        return "window_all"
    if G > 0 and n <= G * 3 // 4:
        gmax = np.zeros(G, np.uint64)
        np.maximum.at(gmax, group_of(np.arange(M), G), key)
        T0 = np.sort(gmax)[::-1][n - 1]
        if int((key >= T0).sum()) <= cap:
            return "window_group"
    T = 0x80000000
    for bit in range(30, -1, -1):
        cand = T | (1 << bit)
        cnt = int((key >= np.uint64(cand)).sum())
        if cnt >= n:
            T = cand
        if cnt == n:
            return "overflow_exact"
    return "overflow_ties"


def _signs(rng, size):
    return np.where(rng.random(size) < 0.5, F32(1), F32(-1)).astype(F32)


def beta_rows(M, n, rng):
    """Named fp32 rows [M + 1] of beta_z0 draws (column M: sigma, finite and
    positive; the all-equal row's is below the 0.01 clip after the scaling)."""
    NQ, R, G = bselect_instance(n)
    rows = {}

    def put(name, v, sigma=None):
        r = np.empty(M + 1, F32)
        r[:M] = v
        r[M] = F32(rng.uniform(0.02, 1.5)) if sigma is None else F32(sigma)
        rows[name] = r

    put("random", rng.standard_normal(M))
    put("all_equal", np.full(M, rng.uniform(0.5, 2.0)) * (1 if rng.random() < 0.5 else -1), sigma=1e-3)
    put("zeros", np.where(rng.random(M) < 0.5, F32(0.0), F32(-0.0)))
    put("alternating", F32(rng.uniform(0.5, 2.0)) * np.where(np.arange(M) % 2 == 0, F32(1), F32(-1)))
    levels = np.sort(rng.uniform(0.1, 3.0, 5)).astype(F32)
    put("few_level", levels[rng.integers(0, 5, M)] * _signs(rng, M))
    # n - 3 distinct large values and a block of 40 equal magnitudes of which the top n takes three
    v = (rng.uniform(0.0, 0.1, M).astype(F32)) * _signs(rng, M)
    pos = rng.permutation(M)
    nl, nt = max(n - 3, 0), min(40, M - max(n - 3, 0))
    v[pos[:nl]] = (F32(2.0) + rng.permutation(nl).astype(F32) / F32(max(nl, 1))) * _signs(rng, nl)
    v[pos[nl:nl + nt]] = F32(1.0) * _signs(rng, nt)
    put("tie_block", v)
    # distinct large values filling n - 1 threshold groups (fewer than n: the n-th group maximum is tiny)
    Gg = G if G > 0 else 64
    groups = rng.permutation(Gg)[:min(n - 1, Gg - 1)]
    inc = np.isin(group_of(np.arange(M), Gg), groups)
    cnt = int(inc.sum())
    v = (F32(1e-4) * (F32(1) + rng.permutation(M).astype(F32) / F32(M))).astype(F32) * _signs(rng, M)
    v[inc] = (F32(5.0) + F32(1e-3) * rng.permutation(cnt).astype(F32)) * _signs(rng, cnt)
    put("cluster", v)
    v = np.where(rng.random(M) < 0.5, F32(0.0), F32(-0.0)).astype(F32)
    nz = rng.permutation(M)[:n // 2]
    v[nz] = rng.standard_normal(nz.size).astype(F32) + F32(0.01)
    put("sparse", v)
    v = rng.standard_normal(M).astype(F32)
    free = rng.permutation(np.setdiff1d(np.arange(M), [3, M - 1]))[:3]
    v[3] = v[M - 1] = np.nan
    v[free[0]], v[free[1]], v[free[2]] = np.inf, -np.inf, F32(1e-40)
    put("special", v)
    return rows


def two_level_z0(M, rng, layout="even_odd"):
    """beta_z0 [100, M + 1] whose rows have one magnitude on the even j and
    another on the odd j; the sign of a column varies with j and is shared by
    the rows, so the mean of any 11 rows has the same two exact tie classes
    (every column of a class sums the same eleven magnitudes in the same order).
    layout "three_quarters": the larger magnitude on the j with j % 4 != 0 -- at
    n = 10 the 50 tied keys of an even / odd row fit the 64-key window, 75 do
    not."""
    z = np.empty((100, M + 1), F32)
    first = np.arange(M) % 2 == 0 if layout == "even_odd" else np.arange(M) % 4 != 0
    sign = np.where(rng.random(M) < 0.5, F32(1), F32(-1)).astype(F32)
    for s in range(100):
        a, b = (F32(k) / F32(16) for k in rng.choice(np.arange(4, 40), 2, replace=False))
        if layout != "even_odd":
            a, b = max(a, b), min(a, b)
        z[s, :M] = np.where(first, a, b) * sign
        z[s, M] = F32(rng.uniform(0.05, 0.4))
    return z


# ---------------------------------------------------------------- Frenet cases
FRENET_INIT = np.array([10.0, 5.0, 8.0, 0.0, 0.02, 0.0], F32)   # init_state_global of every case
FrenetCase = namedtuple("FrenetCase", "point path index other name nan")


def frenet_oracle(num_obs=1, num_prime=2):
    return K.CarlaCEM(4, 1, num_obs, 0.0, num_prime, "gaussian", "Town05", 0.0, 0.0, num_batch=24, maxiter_cem=3)


def frenet_point(ora=None):
    """The point recorded at h = 0 with zero init_eps: the noisy-init row itself."""
    ora = frenet_oracle() if ora is None else ora
    row = ora.noisy_init(FRENET_INIT, np.zeros((1, 4), F32))[0]
    return F32(row[0]), F32(row[1])


def squares(point, x, y):
    """fp32 dx^2 + dy^2 of path points (x, y) as the scan forms them."""
    dx = np.asarray(x, F32) - point[0]
    dy = np.asarray(y, F32) - point[1]
    return (dx * dx + dy * dy).astype(F32)


def _base(P, p):
    """A far polyline (every point >= 25 m from p)."""
    k = np.arange(P, dtype=F32)
    return (p[0] + (k - F32(P // 2))).astype(F32), np.full(P, p[1] + F32(25.0), F32)


def _mirror(p, rng):
    """Two points with bit-equal squared distance from p (exact offsets)."""
    dx, dy = F32(0.25) * F32(rng.integers(8, 16)), F32(0.25) * F32(rng.integers(-6, 7))
    a, b = (F32(p[0] - dx), F32(p[1] + dy)), (F32(p[0] + dx), F32(p[1] + dy))
    sa, sb = squares(p, a[0], a[1]), squares(p, b[0], b[1])
    assert sa.view(np.uint32) == sb.view(np.uint32)
    return a, b


def _sqrt_pair(p, rng):
    """(small, large): squares 1-2 ulp apart with one sqrtf."""
    for _ in range(64):
        th = rng.uniform(0.0, 2.0 * np.pi, 4096)
        x = (p[0] + (2.2 * np.cos(th)).astype(F32)).astype(F32)
        y = (p[1] + (2.2 * np.sin(th)).astype(F32)).astype(F32)
        sq = squares(p, x, y)
        o = np.argsort(sq, kind="stable")
        s = sq[o]
        gap = s[1:].view(np.int32) - s[:-1].view(np.int32)
        ok = (gap >= 1) & (gap <= 2) & (np.sqrt(s[1:]) == np.sqrt(s[:-1]))
        if ok.any():
            k = int(np.argmax(ok))
            return (x[o[k]], y[o[k]]), (x[o[k + 1]], y[o[k + 1]])
    raise AssertionError("no sqrtf-equal pair found")


def frenet_cases(rng, point=None):
    """FrenetCase tuples (point, path, expected index, the other candidate
    index, name, nan).  ``index`` is the design's intent (the CPU test holds it
    against oracle.carla.closest_index); ``other`` the last minimum, or for the
    NaN cases the closest finite point."""
    p = frenet_point() if point is None else point
    cases = []

    def add(name, P, near, index, other, nan=()):
        x, y = _base(P, p)
        for j, (px, py) in near.items():
            x[j], y[j] = px, py
        path = K.make_path(x, y)   # arc, tangents and curvature of the clean polyline
        for j in nan:
            path["x_path"][j] = np.nan
        cases.append(FrenetCase(p, path, index, other, name, bool(nan)))

    for name, P, i, j in (("same_batch", 600, 161, 165), ("other_batch", 600, 10, 100),
                          ("quarters_0_3", 600, 20, 500), ("quarters_1_2", 600, 200, 400),
                          ("quarters_1_3", 600, 160, 470), ("ragged_37", 37, 5, 35), ("ragged_38", 38, 17, 37),
                          ("ends", 600, 0, 599)):
        a, b = _mirror(p, rng)
        add(name, P, {i: a, j: b}, i, j)
    small, large = _sqrt_pair(p, rng)
    add("sqrt_larger_first", 600, {40: large, 470: small}, 40, 470)
    add("sqrt_larger_first_same_quarter", 600, {165: large, 290: small}, 165, 290)
    add("sqrt_smaller_first", 600, {40: small, 470: large}, 40, 470)
    # P identical points: the xy columns only (arc and tangents of the base polyline)
    x, y = _base(600, p)
    path = K.make_path(x, y)
    path["x_path"] = np.full(600, F32(p[0] + F32(1.0)), F32)
    path["y_path"] = np.full(600, F32(p[1] + F32(2.0)), F32)
    cases.append(FrenetCase(p, path, 0, 599, "identical", False))
    a, _ = _mirror(p, rng)
    add("nan_after_minimum", 600, {100: a}, 300, 100, nan=(300, 450))
    add("nan_last_37", 37, {5: a}, 36, 5, nan=(36,))
    return cases


def frenet_of(point, path, idx):
    """(s, d) of a point with the closest index forced to idx
    (oracle.carla.frenet_points after its argmin)."""
    xp, yp, arc, Fxd, Fyd = (np.asarray(path[k], F32) for k in ("x_path", "y_path", "arc_vec", "Fx_dot", "Fy_dot"))
    s = arc[idx]
    Fx, Fy = K.interp(s, arc, Fxd), K.interp(s, arc, Fyd)
    nx, ny = -Fy, Fx
    nrm = np.sqrt(nx * nx + ny * ny)
    d = (F32(1) / nrm) * (nx * (point[0] - xp[idx]) + ny * (point[1] - yp[idx]))
    return F32(s), F32(d)


def frenet_at(case, idx):
    return frenet_of(case.point, case.path, idx)


def margin(prob, s, d, xo, yo):
    """Collision margin of carla_validation_ref.reference."""
    a2, b2 = F32(prob.a_obs ** 2), F32(prob.b_obs ** 2)
    ws, wd = F32(s) - F32(xo), F32(d) - F32(yo)
    return ((-(ws * ws)) / a2 - (wd * wd) / b2) + F32(1)


def frenet_obstacle(case, k):
    """The case's one obstacle, constant in time, in Frenet coordinates:
    (xo [1, 100], yo [1, 100], hit) -- on the oracle's (s, d) for even k (hit),
    on the other index's for odd k (no hit); for a NaN case 60 m past the other
    index, where only the reference's NaN margin counts."""
    if case.nan:
        s, d = frenet_at(case, case.other)
        s, hit = F32(s + F32(60.0)), True
    else:
        hit = k % 2 == 0
        s, d = frenet_at(case, case.index if hit else case.other)
    return np.full((1, 100), s, F32), np.full((1, 100), d, F32), hit


def frenet_plan(case, k):
    """The validate_carla tick of case k (validation.validate_plans' dict)."""
    xo, yo, hit = frenet_obstacle(case, k)
    return dict(init=FRENET_INIT, xo=xo, yo=yo, path=case.path, v_best=np.full(100, F32(8.0), F32),
                steering=np.zeros(100, F32), key=k + 1, tick=k, hit=hit)


def hairpin(point, P=600, gap=6.0, step=0.5):
    """A path that runs out along y = point.y + gap / 2 and back along y =
    point.y - gap / 2 (legs ``gap`` apart), with one point of each leg at the
    bit-equal distance gap / 2 straight above / below ``point``.  Returns
    (path dict, index on the first leg, index on the second leg)."""
    half = P // 2
    h = F32(gap / 2)
    k = np.arange(half, dtype=F32)
    i = half // 3
    x1 = (point[0] + F32(step) * (k - F32(i))).astype(F32)             # outbound; x1[i] == point.x
    x = np.concatenate([x1, x1[::-1]]).astype(F32)
    y = np.concatenate([np.full(half, point[1] + h, F32), np.full(P - half, point[1] - h, F32)]).astype(F32)
    j = P - 1 - i
    assert x[i] == point[0] and x[j] == point[0]
    return K.make_path(x, y), i, j


HAIRPIN_SHAPE = dict(n=4, B=24, H=60, O=3)   # the optimizer case of test_gpu_frenet_ties.py
CARLA_MEAN = np.array([10.0] * 4 + [0.0] * 4, F32)   # test_gpu_carla.py's MEAN / COV
CARLA_COV = np.diag([20.0] * 4 + [100.0] * 4).astype(F32)


def hairpin_oracle():
    s = HAIRPIN_SHAPE
    return K.CarlaCEM(s["n"], 1, s["O"], 0.0, s["H"], "gaussian", "Town05", 0.0, 0.0, num_batch=s["B"], maxiter_cem=1)


def hairpin_scenario(ora):
    """One cvar tick on the hairpin with zero noise and zero init_eps: every
    noisy-init row, hence every candidate's rollout point of h = 0, is the
    equidistant point.  Obstacle 0 sits on that point's Frenet coordinates of
    the first leg at h = 0 and leaves at 40 m per step; the others are far.
    Returns (init, path, xo, yo, draws, i, j)."""
    O = HAIRPIN_SHAPE["O"]
    point = frenet_point(ora)
    path, i, j = hairpin(point)
    s_i, d_i = frenet_of(point, path, i)
    h = np.arange(100, dtype=F32)
    xo = np.stack([s_i + F32(40.0) * h] + [np.full(100, F32(5000.0 + 100.0 * o), F32) for o in range(1, O)])
    yo = np.stack([np.full(100, d_i, F32)] + [np.zeros(100, F32)] * (O - 1))
    draws = K.CarlaDraws.random(ora.prob, np.random.default_rng(7), idx_mpc=5, with_beta_cem=False)
    draws.init_eps = np.zeros_like(draws.init_eps)
    return FRENET_INIT, path, xo.astype(F32), yo.astype(F32), draws, i, j


def closest_index_last(x, y, xp, yp, chunk=8192):
    """oracle.carla.closest_index with the LAST minimum instead of the first
    (the wrong tie-break, for the discrimination assertions only)."""
    x, y = np.asarray(x, F32), np.asarray(y, F32)
    xf, yf = x.reshape(-1), y.reshape(-1)
    out = np.empty(xf.shape[0], np.int64)
    for a in range(0, xf.shape[0], chunk):
        dx = xp[None, :] - xf[a:a + chunk, None]
        dy = yp[None, :] - yf[a:a + chunk, None]
        d = np.sqrt(dx * dx + dy * dy)
        d = np.where(np.isnan(d), -np.inf, d)
        out[a:a + chunk] = d.shape[1] - 1 - np.argmin(d[:, ::-1], axis=1)
    return out.reshape(x.shape)
