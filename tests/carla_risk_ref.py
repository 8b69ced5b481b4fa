"""Expected values of ``mpcmmd_validate_carla_risk`` (include/mpcmmd.h): the
three per-rollout cost channels from the margins of
``carla_validation_ref.reference`` (its ``m``, ``lb``, ``ub``), the statistics
from ``risk_stats_ref.stats``; and the synthetic three-tick fixture the CPU and
the GPU tests share.  Not a test.

Acceptance rule of the costs (``check_costs``).  The device functions are the
ones test_carla_tick_lockstep shows bit-identical to the oracle pieces, so bit
equality is expected and printed; asserted is |gpu - ref| <= TOL, and the same
zero / non-zero pattern except in rows whose decisive margin (the row maximum)
is within TOL of zero, whose share must be <= MAX_NEAR on the reference side.
"""
import numpy as np

import carla_validation_ref as vref
from oracle import carla as K

F32 = np.float32
TOL, MAX_NEAR = vref.TOL, vref.MAX_NEAR
CHANNELS = ("obs", "lane_lb", "lane_ub")


def _relu_max(t, axis):
    """max over ``axis`` of max(0, t), NaN-propagating (jnp.maximum, jnp.max), fp32."""
    with np.errstate(invalid="ignore"):
        return np.max(np.maximum(F32(0), np.asarray(t, F32)), axis=axis).astype(F32)


def channels(ref):
    """[3][R] fp32 costs of one tick's reference: obs = max(0, max_{o,h} m), the lanes likewise from lb, ub."""
    return np.stack([_relu_max(ref["m"], (0, 2)), _relu_max(ref["lb"], 1), _relu_max(ref["ub"], 1)])


def decisive(ref):
    """[3][R] the row maxima of the margins: the value whose sign decides zero / non-zero."""
    with np.errstate(invalid="ignore"):
        return np.stack([np.max(ref["m"], axis=(0, 2)), np.max(ref["lb"], axis=1), np.max(ref["ub"], axis=1)])


def check_costs(ref, got, label=""):
    """The acceptance rule on one tick: got [3][R] fp32.  Returns the share of bit-equal entries."""
    want, dec = channels(ref), decisive(ref)
    got = np.asarray(got, F32)
    assert got.shape == want.shape, (label, got.shape, want.shape)
    near = np.abs(dec) <= TOL
    assert near.mean() <= MAX_NEAR, f"{label}: {near.mean()} of the decisive margins within {TOL} of zero"
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{label}: NaN pattern"
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))[~nan]
    bits = float((got.view(np.uint32) == want.view(np.uint32)).mean())
    print(f"{label}: costs bit-equal share {bits:.6f}, max |gpu - ref| {err.max() if err.size else 0.0:.3e}, "
          f"near-zero decisive share {near.mean():.2e}")
    assert np.all(err <= TOL), f"{label}: max |gpu - ref| = {err.max()}"
    assert np.array_equal((got != 0)[~near], (want != 0)[~near]), f"{label}: zero / non-zero pattern"
    return bits


# ------------------------------------------------------------------ the fixture
FIX_O, FIX_H, FIX_R, FIX_P = 3, 30, 257, 200
FIX_LEVEL, FIX_CONST = 0.3, (0.05, 0.01)
# (psi0, steering amplitude, (y of the even obstacles, y of the odd ones))
FIX_PLANS = ((-0.04, 0.0, (-5.0, 1.4)), (0.02, 0.03, (-5.3, 1.7)), (0.02, 0.0, (-6.5, 3.0)))
# the CPU oracle's count_pos (obs, lb, ub) and var of the three plans, and the counts the notes name
FIX_COUNT_POS = ((223, 20, 0), (28, 0, 13), (0, 0, 1))
FIX_VAR = ((0.2517, 0.4167, 0.0), (0.0736, 0.0, 0.1235), (0.0, 0.0, 0.0))


def fixture_plan(psi0, amp, oy, P=FIX_P, num_obs=FIX_O, length=120.0, key=1, tick=0):
    """A plan along a straight path, built like ``_straight`` of test_gpu_carla_validation.py."""
    xs = np.linspace(0.0, length, P).astype(F32)
    path = K.make_path(xs, np.zeros(P, F32))
    h = np.arange(100, dtype=F32)
    o = np.arange(num_obs, dtype=F32)[:, None]
    xo = (F32(1.5) + F32(3.0) * o + F32(0.3) * h[None, :]).astype(F32)
    yo = np.broadcast_to(np.where(o % 2 == 0, F32(oy[0]), F32(oy[1])), xo.shape).astype(F32)
    return dict(init=np.array([0.0, -1.75, 8.0, 0.0, psi0, 0.0], F32), xo=xo, yo=yo, path=path,
                v_best=(F32(8.0) + F32(0.2) * np.sin(F32(0.3) * h)).astype(F32),
                steering=(F32(amp) * np.cos(F32(0.2) * h)).astype(F32), key=key, tick=tick)


def fixture():
    """(plans, draws [3, 3, R, H], init_eps [3, R, 4]): the same draws for every tick."""
    plans = [fixture_plan(*p, key=i + 1, tick=i) for i, p in enumerate(FIX_PLANS)]
    rng = np.random.default_rng(21)
    draws = rng.standard_normal((3, FIX_R, FIX_H)).astype(F32)
    eps = rng.standard_normal((FIX_R, 4)).astype(F32)
    n = len(plans)
    return plans, np.broadcast_to(draws, (n,) + draws.shape).copy(), np.broadcast_to(eps, (n,) + eps.shape).copy()


def fixture_oracle():
    return K.CarlaCEM(4, 1, FIX_O, FIX_LEVEL, FIX_H, "gaussian", "Town05", FIX_CONST[0], FIX_CONST[1], num_batch=24,
                      maxiter_cem=3)


def fixture_refs(ora=None):
    """The fixture with the reference of every tick: (plans, draws, eps, refs)."""
    ora = ora or fixture_oracle()
    plans, draws, eps = fixture()
    refs = [vref.reference(ora, p["init"], p["v_best"], p["steering"], p["xo"], p["yo"], p["path"], draws[i], eps[i])
            for i, p in enumerate(plans)]
    return plans, draws, eps, refs
