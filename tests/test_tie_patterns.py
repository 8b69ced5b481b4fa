"""The tie patterns of tie_patterns.py do what the GPU tests rely on: the
beta rows reach every path of select_walk that a size can reach, the two-level
draws keep their ties through the elite mean, and each Frenet case's obstacle
tells the oracle's closest index from the other candidate.  CPU only."""
import numpy as np
import pytest

import carla_validation_ref as ref
import tie_patterns as tp
from oracle import beta_cem as bc
from oracle import carla as K

F32 = np.float32


def _paths(M, n, seeds=range(3)):
    NQ, R, G = tp.bselect_instance(n)
    seen = {}
    for seed in seeds:
        for name, row in tp.beta_rows(M, n, np.random.default_rng(1000 * n + seed)).items():
            seen.setdefault(tp.select_path(tp.scaled(row), M, n, NQ, R, G), set()).add(name)
    return seen


@pytest.mark.parametrize("n", tp.BSELECT_N)
def test_beta_rows_reach_every_path(n):
    M = n * n
    NQ, R, G = tp.bselect_instance(n)
    assert M <= 64 * NQ
    seen = _paths(M, n)
    if M <= 64 * R:
        need = {"window_all"}
    else:
        need = {"overflow_ties"}
        if G > 0:
            need.add("window_group")
        # a window overflow without ties needs more than 64 R large keys in fewer than n groups
        if G == 0 or (n - 1) * tp.max_keys_per_group(M, G) > 64 * R:
            need.add("overflow_exact")
    assert need <= set(seen), f"n={n}: paths {sorted(seen)} lack {sorted(need - set(seen))}"
    if M > 64 * R and G > 0:   # ties inside the window too, not only past it
        assert seen["window_group"] & {"tie_block", "few_level", "special"}
        assert "overflow_exact" not in need or "cluster" in seen["overflow_exact"]
    if G == 0:
        assert "random" in seen["overflow_exact"]


@pytest.mark.parametrize("n", tp.BSELECT_N)
def test_select_top_distinct(n):
    M = n * n
    rows = tp.beta_rows(M, n, np.random.default_rng(n))
    assert {"random", "all_equal", "zeros", "alternating", "few_level", "tie_block", "cluster", "sparse",
            "special"} <= set(rows)
    S = tp.scaled(np.stack(list(rows.values())))
    assert np.all(np.isfinite(S[:, M]) & (S[:, M] > 0))
    top = bc.select_top(S, M, n)
    for name, t in zip(rows, top):
        assert len(set(t.tolist())) == n and t.min() >= 0 and t.max() < M, name
    sp = rows["special"]
    assert np.isnan(sp[3]) and np.isnan(sp[M - 1]) and np.isposinf(sp).any() and np.isneginf(sp).any()
    assert np.array_equal(top[list(rows).index("special")][-2:], [3, M - 1]), "NaNs last, by index"
    assert ((np.abs(sp[:M]) > 0) & (np.abs(sp[:M]) < np.finfo(F32).tiny)).any()


TWO_LEVEL = [(6, "even_odd", "window_all"), (10, "even_odd", "window_group"), (10, "three_quarters", "overflow_ties"),
             (16, "even_odd", "overflow_ties"), (22, "even_odd", "overflow_ties")]


@pytest.mark.parametrize("n,layout,path", TWO_LEVEL)
def test_two_level_draws_keep_ties(n, layout, path):
    """Any 11 rows of the two-level draws average to a row with the same two
    tie classes, so the 89 samples of beta-iteration 1 (beta_z[0] = 0) tie too.
    Every n >= 10 takes emit_top's tie branch: n = 16 and 22 with the even / odd
    rows, n = 10 (100 keys, 50 tied: they fit its 64-key window, where the ties
    rank by the words' index half) with the three-quarters layout."""
    M = n * n
    rng = np.random.default_rng(n)
    s0 = tp.scaled(tp.two_level_z0(M, rng, layout))
    NQ, R, G = tp.bselect_instance(n)
    cls = np.arange(M) % 2 == 0 if layout == "even_odd" else np.arange(M) % 4 != 0
    for _ in range(5):
        E = s0[rng.permutation(100)[:11]].astype(np.float64)
        mean = E.mean(axis=0).astype(F32)
        a = np.abs(mean[:M])
        assert np.unique(a[cls]).size == 1 and np.unique(a[~cls]).size == 1 and a[cls][0] != a[~cls][0]
        assert tp.select_path(mean, M, n, NQ, R, G) == path
    assert {tp.select_path(r, M, n, NQ, R, G) for r in s0} == {path}


# ---------------------------------------------------------------- Frenet cases
@pytest.fixture(scope="module")
def frenet():
    ora = tp.frenet_oracle()
    cases = tp.frenet_cases(np.random.default_rng(5), tp.frenet_point(ora))
    return ora, cases


def _last_minimum(case):
    d = np.sqrt(tp.squares(case.point, case.path["x_path"], case.path["y_path"]))
    if case.nan:
        return int(np.nanargmin(d))
    return int(np.nonzero(d == d.min())[0][-1])


def test_frenet_cases_tie_as_designed(frenet):
    ora, cases = frenet
    names = [c.name for c in cases]
    assert len(set(names)) == len(names) >= 14
    for c in cases:
        xp, yp = c.path["x_path"], c.path["y_path"]
        got = int(K.closest_index(np.array([c.point[0]]), np.array([c.point[1]]), xp, yp)[0])
        assert got == c.index, (c.name, got, c.index)
        assert _last_minimum(c) == c.other and c.other != c.index, c.name
        sq = tp.squares(c.point, xp, yp)
        if c.name.startswith("sqrt"):
            gap = int(sq[c.index].view(np.int32)) - int(sq[c.other].view(np.int32))
            assert 1 <= abs(gap) <= 2 and np.sqrt(sq[c.index]) == np.sqrt(sq[c.other]), c.name
            assert (gap > 0) == ("larger_first" in c.name), c.name
            assert c.index < c.other
        elif not c.nan:
            assert sq[c.index].view(np.uint32) == sq[c.other].view(np.uint32), c.name
        else:
            assert np.isnan(sq[c.index]) and sq[c.other] == np.nanmin(sq) and c.other < c.index
    # the quarters of the quad scan (csrc/frenet.hpp: frenet_quarter) the tied pairs fall in
    quarter = lambda P: -(-(-(-P // 4)) // 8) * 8
    where = {c.name: (c.index // quarter(len(c.path["x_path"])), c.other // quarter(len(c.path["x_path"])),
                      c.index // 8 == c.other // 8) for c in cases}
    assert where["same_batch"] == (1, 1, True) and where["other_batch"] == (0, 0, False)
    assert where["quarters_0_3"][:2] == (0, 3) and where["quarters_1_2"][:2] == (1, 2)
    assert where["ragged_37"][:2] == (0, 2) and where["ragged_38"][:2] == (1, 2)
    assert where["sqrt_larger_first"][:2] == (0, 3) and where["sqrt_larger_first_same_quarter"][:2] == (1, 1)


def test_frenet_obstacles_discriminate(frenet):
    """With the oracle's index the margin is >= +0.1 and with the other index
    <= -0.1, or the reverse (a NaN case: NaN, which the reference counts, and
    <= -0.1), so count_oh[0][0] is R or 0 and a wrong index flips it; the lane
    count tells the two indices apart in at least two cases."""
    ora, cases = frenet
    p = ora.prob
    lane_differs = 0
    for k, c in enumerate(cases):
        plan = tp.frenet_plan(c, k)
        m_exp = tp.margin(p, *tp.frenet_at(c, c.index), plan["xo"][0, 0], plan["yo"][0, 0])
        m_oth = tp.margin(p, *tp.frenet_at(c, c.other), plan["xo"][0, 0], plan["yo"][0, 0])
        if c.nan:
            assert np.isnan(m_exp) and m_oth <= -0.1 and plan["hit"], c.name
        elif plan["hit"]:
            assert m_exp >= 0.1 and m_oth <= -0.1, (c.name, m_exp, m_oth)
        else:
            assert m_exp <= -0.1 and m_oth >= 0.1, (c.name, m_exp, m_oth)
        # the oracle composition of one row (zero noise, zero init_eps) agrees with the forced-index evaluation
        r = ref.reference(ora, plan["init"], plan["v_best"], plan["steering"], plan["xo"], plan["yo"], plan["path"],
                          np.zeros((3, 1, 2), F32), np.zeros((1, 4), F32))
        s0, d0 = r["frenet"][0][0, 0], r["frenet"][1][0, 0]
        se, de = tp.frenet_at(c, c.index)
        assert np.array_equal([s0, d0], [se, de], equal_nan=True), c.name
        if not c.nan:
            assert int(r["count_oh"][0, 0]) == int(plan["hit"]) and ref.near_share(r) == 0.0, c.name
            assert np.all(np.abs(r["lb"]) > ref.TOL) and np.all(np.abs(r["ub"]) > ref.TOL), c.name

            def lane(idx):
                d = tp.frenet_at(c, idx)[1]
                lb = [-d + F32(p.y_lb) > 0, r["lb"][0, 1] > 0]
                ub = [d - F32(p.y_ub) > 0, r["ub"][0, 1] > 0]
                return int(max(lb)) + int(max(ub))
            assert lane(c.index) == r["count_lane"], c.name
            lane_differs += lane(c.index) != lane(c.other)
    assert lane_differs >= 2, f"count_lane tells the indices apart in {lane_differs} cases"


def test_hairpin_tells_the_minima_apart(monkeypatch):
    """The hairpin of test_gpu_frenet_ties.py: the noisy-init point is
    bit-equidistant from one point of each leg (6 m apart), the oracle takes
    the first, and an oracle that takes the last moves a candidate's obstacle
    cost by more than 100 x the lockstep tolerance (1e-5 + 1e-4 |obs|)."""
    MEAN, COV = tp.CARLA_MEAN, tp.CARLA_COV
    ora = tp.hairpin_oracle()
    init, path, xo, yo, draws, i, j = tp.hairpin_scenario(ora)
    p = tp.frenet_point(ora)
    sq = tp.squares(p, path["x_path"], path["y_path"])
    assert i < j and sq[i].view(np.uint32) == sq[j].view(np.uint32) == sq.min().view(np.uint32)
    assert np.nonzero(sq == sq.min())[0].tolist() == [i, j]
    assert abs(path["y_path"][i] - path["y_path"][j]) == 6.0
    st = ora.init_carla("cvar", init, MEAN, COV, path, draws)
    assert np.all(st["rows0"][:, 0] == p[0]) and np.all(st["rows0"][:, 1] == p[1])
    pr, acc, steer = ora.front_carla(st, path)
    obs, _, _, extra = ora.candidate_costs_carla("cvar", st, acc, steer, xo, yo, path, draws, 0)
    assert np.all(extra["frenet"][0][:, :, 0] == path["arc_vec"][i])
    monkeypatch.setattr(K, "closest_index", tp.closest_index_last)
    obs_last, _, _, extra_last = ora.candidate_costs_carla("cvar", st, acc, steer, xo, yo, path, draws, 0)
    assert np.all(extra_last["frenet"][0][:, :, 0] == path["arc_vec"][j])
    tol = 1e-5 + 1e-4 * np.abs(obs)
    assert np.any(np.abs(obs_last - obs) > 100 * tol), (obs, obs_last)
