"""The inputs of tests/front_scenarios.py reach the paths of k_front they are
built for -- asserted on the oracle alone, on the CPU.  A scenario that stops
reaching its path fails here and does not pass silently on the GPU
(tests/test_gpu_front_edges.py runs the same inputs through the kernel).
"""
import numpy as np
import pytest

import front_scenarios as F

F32 = np.float32


@pytest.fixture(scope="module")
def prob():
    return F.static_oracle().prob


def _probe(prob, sc):
    return F.probe(prob, F.oracle_state(prob, sc))


def _excused_ok(prob, sc, g, kappa_y=None):
    ex = F.excused(prob, g, kappa_y)
    if sc.group in F.NO_EXCUSE:
        assert not ex.any(), f"{sc.name}: candidates {np.nonzero(ex)[0]} sit on a decision boundary"
    assert ex.mean() <= F.EXCUSED_CAP, f"{sc.name}: {int(ex.sum())} of {ex.size} candidates excused"


def test_default_input_reaches_none_of_it(prob):
    """The gap: the lockstep's input (DEFAULT_INIT, the sampler's draw) has no
    velocity-heading wrap, no clipped d_v, no d_a at 18 and no exact +-pi step."""
    g = _probe(prob, F.default_input())
    assert F.wrap_rows(g["av_raw"]).sum() == 0
    assert F.clipped_low(g["dv"], prob.v_min) == 0 and F.clipped_high(g["dv"], prob.v_max) == 0
    assert F.clipped_high(g["da"], prob.a_max) == 0
    for a in (g["av_raw"], g["aa_raw"]):
        assert F.exact_pi_steps(a, +1) == 0 and F.exact_pi_steps(a, -1) == 0
    # what it does reach: short wraps of the acceleration heading, none of them past the first register's carry
    assert F.wrap_rows(g["aa_raw"]).max() >= 1
    assert not F.winding_features(g["aa_raw"], g["aa"])["carry"].any()


def test_straight(prob):
    n = {(h, s): 0 for h in ("av", "aa") for s in (+1, -1)}
    for sc in F.straight():
        g = _probe(prob, sc)
        assert np.all(g["yd"] == 0) and np.all(g["ydd"] == 0), f"{sc.name}: the guess leaves the line"
        for h, s in n:
            n[(h, s)] += F.exact_pi_steps(g[h + "_raw"], s)
        _excused_ok(prob, sc, g)
    for (h, s), c in n.items():
        assert c >= 1, f"no heading step of exactly {s:+d} * float32(pi) on {h}"


def test_standstill(prob):
    for sc in F.standstill():
        g = _probe(prob, sc)
        assert F.clipped_low(g["dv"], prob.v_min) >= F.B, sc.name
        if sc.name != "crawl":
            assert (g["speed_proj"] < 1e-10).sum() >= 1, sc.name
        if sc.name == "denormal":
            sq = g["xd"] * g["xd"]
            assert ((sq > 0) & (sq < np.finfo(F32).tiny)).sum() >= F.B, "xd * xd of the guess is no fp32 subnormal"
        _excused_ok(prob, sc, g)


def test_reverse(prob):
    (sc,) = F.reverse()
    g = _probe(prob, sc)
    assert (F.wrap_rows(g["av_raw"]) > 0).all(), "every candidate wraps the velocity heading"
    assert g["pr"]["res_norm"].max() < 1e-5, "every candidate is feasible"
    _excused_ok(prob, sc, g)


def test_overspeed(prob):
    (sc,) = F.overspeed()
    g = _probe(prob, sc)
    assert F.clipped_high(g["dv"], prob.v_max) > g["dv"].size // 2
    _excused_ok(prob, sc, g)


def test_hard_acc(prob):
    (sc,) = F.hard_acc()
    g = _probe(prob, sc)
    assert F.clipped_high(g["da"], prob.a_max) >= F.B
    _excused_ok(prob, sc, g)


def test_off_lane(prob):
    for sc in F.off_lane():
        g = _probe(prob, sc)
        rows = F.UPPER if "+" in sc.name else F.LOWER
        assert F.slack0_share(g, rows) >= 0.05, f"{sc.name}: {F.slack0_share(g, rows):.3f} of the rows at slack 0"
        s = sc.carries["s_lane"]
        assert (s > 0).all() and (s > prob.y_ub - prob.y_lb).any(), "written slacks: nonzero, some beyond the lane width"
        assert sc.stages == 2
        _excused_ok(prob, sc, g)
    assert [float(sc.init[1]) for sc in F.off_lane()] == [5.0, -5.0, 2.25, -2.25]


def _winding_found(prob, scenarios):
    found = set()
    for sc in scenarios:
        g = _probe(prob, sc)
        for h in ("v", "a"):
            for f, m in F.winding_features(g[f"a{h}_raw"], g[f"a{h}"]).items():
                if m.any():
                    found.add((h, f))
    return found


def test_winding(prob):
    want = {(h, f) for h in ("v", "a") for f in F.WINDING_FEATURES}
    assert _winding_found(prob, F.winding()) == want
    for sc in F.winding():
        assert sc.pop[:, :4].min() >= 0 and sc.pop[:, :4].max() <= 0.5
        _excused_ok(prob, sc, _probe(prob, sc))
    # the default draw in the same states reaches less: the predicate notices a weakened construction
    weak = [F.Scenario(sc.name, sc.init, F.default_input().pop) for sc in F.winding()]
    assert _winding_found(prob, weak) != want


def test_special(prob):
    clean, dirty = F.special()
    rows = F.special_rows(dirty)
    assert rows.reshape(-1, 4).sum(axis=1).tolist() == [1] * (F.B // 4), "one special candidate per workgroup"
    assert set(np.nonzero(rows)[0] % 4) == {0, 1, 2, 3}, "every wave position carries one"
    assert np.isnan(dirty.pop[1, 1]), "wave 1 of the first workgroup carries the NaN speed"
    assert np.array_equal(clean.pop[~rows], dirty.pop[~rows])
    kinds = {(int(np.nonzero(~np.isfinite(r))[0][0]) < 4, "nan" if np.isnan(r).any() else ("+" if (r == np.inf).any() else "-"))
             for r in dirty.pop[rows]}
    assert kinds == {(True, "nan"), (False, "nan"), (True, "+"), (True, "-")}
    _excused_ok(prob, dirty, _probe(prob, dirty))


def test_ragged():
    for full, part in F.ragged():
        assert part.B == 30 and np.array_equal(full.pop[:30], part.pop)
    assert {f.group for f, _ in F.ragged()} == {"straight", "winding"}


def test_carla():
    ora = F.carla_oracle()
    ends, curve = F.carla_scenarios()
    arc = ends.path["arc_vec"]
    pr, _, steer, g, ky = F.carla_front(ora, ends)
    assert (pr["x"] < 0).sum() >= 1, "no projected station below the path's start"
    assert (pr["x"] > arc[-1]).sum() >= 1, "no projected station beyond the path's end"
    assert np.isin(pr["x"][:, 1:], arc[1:-1]).sum() >= 1, "no station on an interior knot after t = 0"
    ex = F.excused(ora.prob, g, ky)
    assert ex.mean() <= F.EXCUSED_CAP
    pr, _, steer, g, ky = F.carla_front(ora, curve)
    assert F.excused_points(ky).sum() >= 1, "1 - y kappa stays away from 0"
    assert float(np.abs(curve.path["kappa"]).max()) > 0.02
    ex = F.excused(ora.prob, g, ky)
    assert ex.mean() <= F.EXCUSED_CAP, f"{int(ex.sum())} of {ex.size} candidates excused"


def test_det():
    ora = F.carla_oracle()
    coincide, nonfinite = F.det_scenarios()
    pr, _, _, g, ky = F.carla_front(ora, coincide)
    assert len(F.coincidences(coincide, g)) >= 2, "no obstacle on a guess point"
    assert np.isfinite(pr["res_norm"]).all()
    assert F.excused(ora.prob, g, ky).mean() <= F.EXCUSED_CAP
    xn, yn = nonfinite.det_tracks
    assert np.isposinf(xn[:, 63]).any() and np.isposinf(yn[:, 0]).any() and np.isposinf(yn[:, 99]).any()
    assert np.isnan(xn[:, 64]).any()
    # an obstacle coordinate that is not finite reaches every candidate (the tracks are shared) and, through
    # rho_obs A_obs^T b_obs, every coefficient: the oracle's outputs are NaN throughout
    pr = F.carla_front(ora, nonfinite)[0]
    assert np.isnan(pr["c_x"]).all() and np.isnan(pr["c_y"]).all() and np.isnan(pr["res_norm"]).all()
