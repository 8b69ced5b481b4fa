"""The scenarios of test_gpu_risk_shapes.py are not degenerate: the same
conditions that the GPU test asserts on the oracle's values with the GPU's
controls, here with the oracle's own controls (they agree to 1e-3), so a
change to the oracle or to the scenario that empties a case shows without a
GPU.  The two num_reduced = 1024 shapes (5 s each) are left to the GPU test.
"""
import numpy as np
import pytest

from risk_scenarios import (assert_not_degenerate, collision_scenario, make_oracle, noisy_rollouts, saa_brackets)

CASES = [("cvar", "gaussian", 2, 1, 2, False), ("cvar", "gaussian", 51, 2, 8, False),
         ("cvar", "gaussian", 24, 3, 12, False), ("cvar", "gaussian", 65, 64, 20, False),
         ("cvar", "gaussian", 101, 8, 100, False), ("cvar", "gaussian", 513, 65, 12, False),
         ("cvar", "gaussian", 201, 64, 20, False), ("cvar", "gaussian", 1000, 4, 20, False),
         ("saa", "gaussian", 24, 3, 12, False), ("saa", "gaussian", 65, 64, 20, False),
         ("saa", "gaussian", 513, 65, 12, False), ("mmd_random", "gaussian", 24, 3, 12, False),
         ("mmd_random", "gaussian", 65, 64, 20, False), ("mmd_random", "gaussian", 513, 65, 12, False),
         ("cvar", "beta", 65, 2, 8, False), ("cvar", "gaussian", 24, 3, 12, True),
         ("mmd_random", "gaussian", 65, 64, 20, True), ("cvar", "gaussian", 1000, 4, 20, True)]


@pytest.mark.parametrize("cost,noise,S,O,H,overtaker", CASES)
def test_scenario_not_degenerate(cost, noise, S, O, H, overtaker):
    ora, draws, st, acc, steer = make_oracle(cost, noise, S, O, H)
    xo, yo = collision_scenario(ora, st, acc, steer, cost, overtaker)
    obs, lane, _ = ora.candidate_costs(cost, st, acc, steer, xo, yo, draws, 0)
    assert_not_degenerate(ora, cost, obs, lane, xo)
    if cost == "saa":   # the counts lie in their brackets, and the brackets are narrow
        xr, yr = noisy_rollouts(ora, st, acc, steer, draws)
        for got, (lo, hi) in zip((obs, lane), saa_brackets(ora, xr, yr, xo, yo)):
            cnt = np.rint(got.astype(np.float64) * S)
            assert np.all(hi - lo <= 0.02 * S) and np.all((lo <= cnt) & (cnt <= hi))
    if overtaker:       # at step 2 the overtaker is outside no rollout's window, at step 0 outside every one
        x = noisy_rollouts(ora, st, acc, steer, draws)[0]
        a = np.float32(ora.prob.a_obs)
        assert np.all(np.abs(x[..., 0] - xo[2, 0]) >= a) and np.all(np.abs(x[..., 2] - xo[2, 2]) < 0.1)
        assert np.all(xo[np.arange(O) != 2, 2] > xo[2, 2] + 1.0)
