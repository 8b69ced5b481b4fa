"""The Frenet closest-point scan on the GPU (csrc/frenet.hpp:
frenet_point_quad, in mpcmmd_validate_carla and in the optimizer's k_frenet)
on path points at bit-equal distance, at sqrtf-equal distance with squares an
ulp or two apart, and with NaN coordinates: it must return jnp.argmin's index
(the first minimum of the sqrtf values, the first NaN if any).  Each case's
obstacle sits where only that index collides -- or where only the other tied
index does (tie_patterns.py; test_tie_patterns.py asserts the margins) -- so a
wrong index flips count_oh from R to 0 or back."""
import numpy as np
import pytest

import carla_validation_ref as ref
import tie_patterns as tp
from parity import close

pytestmark = pytest.mark.gpu

F32 = np.float32


@pytest.mark.parametrize("R", [1, 65])
def test_validate_carla_closest_point_ties(native, R):
    """Zero noise, zero init_eps, H = 2: the point recorded at h = 0 is the
    noisy-init row itself, the same for every rollout.  One tick per case, one
    call per path length (600, 37, 38: a call has one num_path)."""
    ora = tp.frenet_oracle()
    cases = tp.frenet_cases(np.random.default_rng(5), tp.frenet_point(ora))
    plans = [tp.frenet_plan(c, k) for k, c in enumerate(cases)]
    for P in sorted({len(c.path["x_path"]) for c in cases}):
        ks = [k for k, c in enumerate(cases) if len(c.path["x_path"]) == P]
        g = lambda name: [plans[k][name] for k in ks]
        draws, eps = np.zeros((len(ks), 3, R, 2), F32), np.zeros((len(ks), R, 4), F32)
        out = native.validate_carla(g("init"), g("v_best"), g("steering"), g("xo"), g("yo"), g("path"), g("key"), 2,
                                    "gaussian", 0.0, 0.0, 0.0, num_rollouts=R, variant="carla_town05", draws=draws,
                                    init_eps=eps, count_oh=True)
        for i, k in enumerate(ks):
            c, p = cases[k], plans[k]
            got = dict(count=out["count"][i], count_rows=out["count_rows"][i], count_lane=out["count_lane"][i],
                       count_oh=out["count_oh"][i])
            want = R if p["hit"] else 0
            assert int(got["count_oh"][0, 0]) == want, \
                f"{c.name} (P={P}, R={R}): count_oh[0][0] = {got['count_oh'][0, 0]}, the oracle's index gives {want}"
            if c.nan:   # the NaN margin counts (count_nonzero(max(0, NaN))); the bracket below takes finite margins
                continue
            r = ref.reference(ora, p["init"], p["v_best"], p["steering"], p["xo"], p["yo"], p["path"], draws[i],
                              eps[i])
            assert ref.near_share(r) == 0.0
            assert ref.check_counts(r, got, R, f"{c.name} P={P} R={R}"), "the bracket is exact here"
            assert int(got["count_lane"]) == r["count_lane"]


def test_frenet_hairpin_cvar_iteration(native):
    """One cvar iteration of the CARLA optimizer (k_frenet) on a hairpin path
    whose legs, 6 m apart, each hold one point bit-equidistant from the
    noisy-init point (zero noise, zero init_eps: the h = 0 point of every
    rollout): test_carla_tick_lockstep's checks and tolerances.  An oracle that
    takes the last minimum instead moves the obstacle costs by more than 100 x
    that tolerance (test_tie_patterns.py: test_hairpin_tells_the_minima_apart)."""
    MEAN, COV = tp.CARLA_MEAN, tp.CARLA_COV
    n, B, H, O = (tp.HAIRPIN_SHAPE[k] for k in ("n", "B", "H", "O"))
    T = 1
    ora = tp.hairpin_oracle()
    init, path, xo, yo, draws, i, j = tp.hairpin_scenario(ora)
    trace = []
    cx, cy, v_best, steer_best, mean_param, _ = ora.solve_carla("cvar", 5, init, MEAN, COV, xo, yo, 10.0, path, draws,
                                                                trace=trace)
    assert np.ptp(trace[0]["obs"]) == 0 and trace[0]["obs"][0] > 0, "every candidate meets obstacle 0 at h = 0 only"
    nat = native.Handle(native.make_config(n, O, 0.0, H, "gaussian", 0.0, 0.0, num_batch=B, maxiter_cem=T,
                                           variant="carla_town05"))
    try:
        nat.carla_begin("cvar", 5, init, MEAN, COV, xo, yo, 10.0, path, draws)
        st0 = ora.init_carla("cvar", init, MEAN, COV, path, draws)
        R = st0["rows0"].shape[0]
        assert np.array_equal(nat.read("st0r").reshape(-1, 8)[:R, :5], st0["rows0"]), "noisy initial rows differ"
        nat.iterate(0, 1)
        nat.sync()
        tr = trace[0]
        close("steer", nat.read("steer").reshape(-1, 100)[:B], tr["steer"], rtol=0, atol=0)
        close("kappa", nat.read("kappa_i").reshape(-1, 100)[:B], tr["kappa"], rtol=0, atol=0)
        obs_g, lane_g, des_g = nat.read("obs_cost")[:B], nat.read("lane_cost")[:B], nat.read("lane_des")[:B]
        fl = 1e-5
        ok = np.abs(obs_g - tr["obs"]) <= fl + 1e-4 * np.abs(tr["obs"])
        ok &= np.abs(lane_g - tr["lane"]) <= fl + 1e-4 * np.abs(tr["lane"])
        ok &= np.abs(des_g - tr["des"]) <= fl + 1e-4 * np.abs(tr["des"])
        assert ok.all(), (f"candidates {np.nonzero(~ok)[0]} differ: obs {obs_g[~ok]} vs {tr['obs'][~ok]}, lane "
                          f"{lane_g[~ok]} vs {tr['lane'][~ok]}")
        assert np.array_equal(nat.read("tr_proj", np.int32).reshape(T, B)[0], tr["perm"])
        assert np.array_equal(nat.read("tr_obs", np.int32).reshape(T, 20)[0], tr["elite_obs"])
        assert np.array_equal(nat.read("tr_cem", np.int32).reshape(T, 5)[0], tr["elite_cem"])
        got = nat.finish()
        close("cx", got["cx"], cx, rtol=1e-4, atol=1e-4)
        close("cy", got["cy"], cy, rtol=1e-4, atol=1e-4)
        close("v_best", got["v_best"], v_best, rtol=1e-4, atol=1e-4)
        close("steering", got["steering"], steer_best, rtol=1e-4, atol=1e-5)
        close("mean_param", got["mean_param"], mean_param, rtol=1e-4, atol=1e-4)
    finally:
        nat.close()
