"""Monte-Carlo validation of CARLA plans on the GPU (``mpcmmd_validate_carla``,
``mpcmmd_validate_carla_risk``, include/mpcmmd.h).

The reference measures the safety of its CARLA runs with the live simulator's
collision sensor only.  Without the simulator, the question the paper asks --
which cost gives plans that collide less under the noise model -- is answered
here by the optimizer's own risk model: for every simulator tick the returned
plan (``v_best``, ``steering_best``) is rolled out ``num_rollouts`` times from
fresh noisy initial states with fresh control noise, mapped to the tick's
Frenet frame and compared with the obstacle ellipses and the lane bounds, and
the hits are counted as ``synthetic_static_obs/validation.py:153-169`` counts
them.  All ticks run in ONE launch.  ``risk_plans`` takes the same rollouts to
the optimizer's own cost terms instead: per rollout the maximum obstacle and
lane costs, and per tick their SAA / VaR / CVaR / mean / max and the
uniform-weight MMD, beside the counts of the same pass.
"""
from __future__ import annotations

import numpy as np

from ._lib import native

NUM_ROLLOUTS = 1000  # validation.py:173 (_num_batch)


def validate_plans(prob, plans, num_rollouts=NUM_ROLLOUTS, draws=None, init_eps=None, seed=0, count_oh=False,
                   timing=False):
    """Counts of every plan of ``plans`` under ``prob``'s noise model.

    prob: the CARLA ``CEM`` drop-in (town, noise, levels, H, O are taken from
    it).  plans: per-tick dicts with ``init`` (init_state_global [6]), ``xo``,
    ``yo`` (Frenet obstacle tracks [O, 100]), ``path`` (dict of the six path
    arrays), ``v_best``, ``steering`` ([100], the solve's return) and ``key``
    (the tick's Philox key, e.g. the tick index).  Returns the dict of
    ``_native.validate_carla``: count, count_lane, count_rows [len(plans)]."""
    N = native()
    g = lambda name: [p[name] for p in plans]
    return N.validate_carla(g("init"), g("v_best"), g("steering"), g("xo"), g("yo"), g("path"), g("key"),
                            prob.num_prime, prob.noise, prob.sigma_acc, prob.acc_const_noise, prob.steer_const_noise,
                            num_rollouts=num_rollouts, variant=prob.variant, draws=draws, init_eps=init_eps,
                            seed=seed, device=prob._cfg.device, count_oh=count_oh, timing=timing)


def risk_plans(prob, plans, num_rollouts=NUM_ROLLOUTS, alpha=0.98, sigma=(), draws=None, init_eps=None, seed=0,
               return_costs=False, counts=True, timing=False):
    """Risk statistics of every plan of ``plans`` (as ``validate_plans`` takes
    them) under ``prob``'s noise model: the dict of
    ``_native.validate_carla_risk`` -- count_pos, saa, var, cvar, mean, max
    [len(plans), 3] over the channels (obs, lane_lb, lane_ub), mmd
    [len(plans), 3, len(sigma)], cvar_lane, mmd_lane -- and with ``counts`` the
    count arrays of ``validate_plans`` from the same rollouts."""
    N = native()
    g = lambda name: [p[name] for p in plans]
    sg = np.asarray(sigma, np.float32)
    return N.validate_carla_risk(g("init"), g("v_best"), g("steering"), g("xo"), g("yo"), g("path"), g("key"),
                                 prob.num_prime, prob.noise, prob.sigma_acc, prob.acc_const_noise,
                                 prob.steer_const_noise, num_rollouts=num_rollouts, variant=prob.variant, draws=draws,
                                 init_eps=init_eps, seed=seed, device=prob._cfg.device, alpha=alpha,
                                 sigma=sg if sg.size else None, return_costs=return_costs, counts=counts,
                                 timing=timing)
