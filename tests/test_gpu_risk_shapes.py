"""The baseline risk stage (k_risk_baseline: cvar, saa, mmd_random) against
the oracle on scenarios that really collide, at the shapes where its
branches change: the per-step obstacle window and its carried start, the
full scan above 64 obstacles or with a NaN coordinate, one or two rollout
rows per thread, block_cvar's window over the group maxima, H = 2 and 100,
and the largest shape mpcmmd_create accepts.

Each case drives the stage as the lockstep of test_gpu_parity_baseline.py
does (begin, front, the GPU's controls handed to the oracle, risk) and first
asserts on the ORACLE's values that the case is not degenerate
(risk_scenarios.assert_not_degenerate).  Tolerances are the contract's
(parity.py): cvar 1e-4 / 1e-4, mmd_random 1e-4 / 1e-2, the
lane cost as its obstacle cost; saa, a count, is bracketed per candidate by
the oracle's fp64 margins (risk_scenarios.saa_brackets).  Measured on an
MI355X: worst |GPU - oracle| of a cvar cost 5.4e-7 (obstacle) and 1.5e-5
(lane, at H = 100), of an mmd_random cost 1.4e-3; H = 100, twice the longest
horizon compared before, needed no tolerance of its own.
"""
import ctypes

import numpy as np
import pytest

from parity import DEFAULT_COV, DEFAULT_MEAN, close
from risk_scenarios import (ACC_C, B, DELTA, RISK_INIT, STEER_C, assert_not_degenerate, collision_scenario,
                            make_oracle, noisy_rollouts, saa_brackets)

pytestmark = pytest.mark.gpu

ATOL = {"cvar": 1e-4, "saa": 1e-4, "mmd_random": 1e-2}
E_UNSUPPORTED = -3


def gpu_risk(native, cost, noise, S, O, H, xo, yo, draws):
    """Front and risk stage of iteration 0 on a fresh handle: the GPU's
    controls acc, steer [B, 100] and its obs_cost, lane_cost [B]."""
    level = 0.1 if noise == "gaussian" else 0.3
    cfg = native.make_config(S, O, level, H, noise, ACC_C, STEER_C, num_batch=B, maxiter_cem=1, device=0, seed=0)
    nat = native.Handle(cfg)
    try:
        nat.begin(cost, 123, RISK_INIT[cost], DEFAULT_MEAN, DEFAULT_COV, xo, yo, 15.0, draws)
        nat.run_stage(1, 0)
        acc = nat.read("acc").reshape(B, 100).copy()
        steer = nat.read("steer").reshape(B, 100).copy()
        nat.run_stage(2, 0)
        return acc, steer, nat.read("obs_cost")[:B].copy(), nat.read("lane_cost")[:B].copy()
    finally:
        nat.close()


def compare(cost, noise, ora, st, draws, xo, yo, gpu, degenerate_ok=False):
    """The GPU's costs of one case against the oracle's on the GPU's controls."""
    acc, steer, obs_g, lane_g = gpu
    S = ora.prob.num_reduced
    obs, lane, _ = ora.candidate_costs(cost, st, acc, steer, xo, yo, draws, 0)
    if not degenerate_ok:
        assert_not_degenerate(ora, cost, obs, lane, xo)
    if cost == "saa" and not degenerate_ok:
        xr, yr = noisy_rollouts(ora, st, acc, steer, draws)
        for name, got, (lo, hi) in zip(("obs", "lane"), (obs_g, lane_g), saa_brackets(ora, xr, yr, xo, yo)):
            cnt = got.astype(np.float64) * S
            print(f"saa {name}: GPU counts {np.rint(cnt).astype(int).tolist()}, widest bracket {int((hi - lo).max())}")
            assert np.all(hi - lo <= 0.02 * S), f"saa {name}: {int((hi - lo).max())} samples within {DELTA} of 0"
            assert np.all(np.abs(cnt - np.rint(cnt)) < 1e-3), f"saa {name}: S * cost is no integer: {cnt}"
            assert np.all((lo <= np.rint(cnt)) & (np.rint(cnt) <= hi)), \
                f"saa {name}: counts {np.rint(cnt).astype(int)} outside [{lo}, {hi}]"
        return
    frac = 0.05 if noise == "beta" else 0.0   # rejection-sampler ulps (test_gpu_parity_baseline.py)
    with np.errstate(invalid="ignore"):
        print(f"{cost} obs: worst |GPU - oracle| {np.nanmax(np.abs(obs_g - obs), initial=0):.3g}, "
              f"lane {np.nanmax(np.abs(lane_g - lane), initial=0):.3g}")
    close("obs_cost", obs_g, obs, rtol=1e-4, atol=ATOL[cost], frac_ok=frac)
    close("lane_cost", lane_g, lane, rtol=1e-4, atol=ATOL[cost], frac_ok=frac)


def run_case(native, cost, noise, S, O, H, overtaker=False):
    ora, draws, st, acc_o, steer_o = make_oracle(cost, noise, S, O, H)
    xo, yo = collision_scenario(ora, st, acc_o, steer_o, cost, overtaker)
    compare(cost, noise, ora, st, draws, xo, yo, gpu_risk(native, cost, noise, S, O, H, xo, yo, draws))


# (S, O, H): S = 2 (lo = 0, hi = 1); S - 1 a multiple of 50 (51, 101, 201: 0.98 (S - 1) on an integer);
# 65 / 513 / 1024 (a second wave, a second row per thread, the most rows); O = 1, the window's last size
# 64 and the full scan's first 65; H = 2 and H = 100
CVAR_SHAPES = [(2, 1, 2), (51, 2, 8), (24, 3, 12), (65, 64, 20), (101, 8, 100), (513, 65, 12), (1024, 81, 100),
               (201, 64, 20), (1000, 4, 20)]
OTHER_SHAPES = [(24, 3, 12), (65, 64, 20), (513, 65, 12)]


@pytest.mark.parametrize("S,O,H", CVAR_SHAPES)
def test_cvar_shapes(native, S, O, H):
    run_case(native, "cvar", "gaussian", S, O, H)


@pytest.mark.parametrize("S,O,H", OTHER_SHAPES)
@pytest.mark.parametrize("cost", ["saa", "mmd_random"])
def test_saa_mmd_random_shapes(native, cost, S, O, H):
    run_case(native, cost, "gaussian", S, O, H)


@pytest.mark.parametrize("S,O,H", [(65, 2, 8), (513, 8, 20)])
def test_cvar_beta_noise_shapes(native, S, O, H):
    run_case(native, "cvar", "beta", S, O, H)


@pytest.mark.parametrize("S,O,H", [(24, 3, 12), (65, 64, 20), (1000, 4, 20)])
@pytest.mark.parametrize("cost", ["cvar", "mmd_random"])
def test_window_start_walks_back(native, cost, S, O, H):
    """An obstacle that comes from behind the window (collision_scenario's
    overtaker): the start index carried over from the previous step is too
    far on, and without the walk back every sample misses its nearest
    obstacle.  In the sweep above the ego outruns every obstacle, so the
    carried start only ever moves on."""
    run_case(native, cost, "gaussian", S, O, H, overtaker=True)


def risk_lds_bytes(O, H, S):
    """k_risk_baseline's dynamic LDS as its launcher sizes it (risk_lds_bytes,
    csrc/k_risk.hip): 4 O H + 2 H + 3 S floats, S 8-byte sort words, and
    ReduceScratch (block.hpp: 16 doubles, 16 ints, an int, two floats, a
    64-bit word and 128 16-byte-aligned 64-bit words = 1248 bytes)."""
    up = lambda v: (v + 15) & ~15
    return up(up((4 * O * H + 2 * H + 3 * S) * 4) + 8 * S) + 1248


def device_lds_per_block(native):
    """Device 0's shared memory per workgroup, asked of the HIP runtime that
    libmpcmmd has loaded (hipDeviceGetAttribute)."""
    native.lib()
    with open("/proc/self/maps") as f:
        path = next(line.split()[-1] for line in f if "libamdhip64" in line)
    value = ctypes.c_int(0)
    kMaxSharedMemoryPerBlock = 74   # hipDeviceAttributeMaxSharedMemoryPerBlock (hip_runtime_api.h)
    rc = ctypes.CDLL(path).hipDeviceGetAttribute(ctypes.byref(value), kMaxSharedMemoryPerBlock, 0)
    assert rc == 0, f"hipDeviceGetAttribute: {rc}"
    return value.value


def test_largest_accepted_shape(native):
    """num_obs * num_prime = 8192 at num_reduced = 1024, the most mpcmmd_create's
    range check accepts: either the device can launch its 150 KiB of LDS and
    the stage agrees with the oracle, or create refuses the shape."""
    S, O, H = 1024, 128, 64
    need = risk_lds_bytes(O, H, S)
    have = device_lds_per_block(native)
    assert 64 * 1024 <= have <= 1024 * 1024, f"shared memory per workgroup: {have} B"
    print(f"risk stage LDS: {need} B needed, {have} B per workgroup")
    if need <= have:
        run_case(native, "cvar", "gaussian", S, O, H)
        return
    cfg = native.make_config(S, O, 0.1, H, "gaussian", ACC_C, STEER_C, num_batch=B, maxiter_cem=1, device=0, seed=0)
    with pytest.raises(native.NativeError, match=f"error {E_UNSUPPORTED}:"):
        native.Handle(cfg)


@pytest.mark.parametrize("cost", ["cvar", "saa", "mmd_random"])
def test_window_equals_full_scan(native, cost):
    """64 obstacles take the sorted window; the same 64 and one parked 10 km
    away take the full scan, and the far one contributes nothing on either
    path; the 64 in reversed input order are sorted into the same steps.  All
    three handles must give the same bits."""
    S, O, H = 65, 64, 20
    ora, draws, st, acc_o, steer_o = make_oracle(cost, "gaussian", S, O, H)
    xo, yo = collision_scenario(ora, st, acc_o, steer_o, cost)
    base = gpu_risk(native, cost, "gaussian", S, O, H, xo, yo, draws)
    compare(cost, "gaussian", ora, st, draws, xo, yo, base)     # and the values are the oracle's
    far = gpu_risk(native, cost, "gaussian", S, O + 1, H, np.vstack([xo, np.full((1, 100), 1e4, np.float32)]),
                   np.vstack([yo, np.zeros((1, 100), np.float32)]), draws)
    rev = gpu_risk(native, cost, "gaussian", S, O, H, xo[::-1].copy(), yo[::-1].copy(), draws)
    for name, other in (("65 obstacles (full scan)", far), ("reversed input order", rev)):
        assert np.array_equal(base[0], other[0]) and np.array_equal(base[1], other[1]), f"{name}: controls differ"
        for k, what in ((2, "obs_cost"), (3, "lane_cost")):
            assert np.array_equal(base[k].view(np.uint32), other[k].view(np.uint32)), \
                f"{name}: {what} differs from the window's: {base[k]} vs {other[k]}"


SPECIAL = {
    "x_inf": (np.inf, None),        # no contribution, costs finite
    "x_nan": (np.nan, None),
    "y_nan_x_far": (500.0, np.nan),  # |x - x_obs| >= a_obs for every rollout
    "y_nan_x_near": (None, np.nan),
}


@pytest.mark.parametrize("cost", ["cvar", "saa", "mmd_random"])
@pytest.mark.parametrize("special", list(SPECIAL))
def test_special_obstacle_values(native, cost, special):
    """One coordinate of obstacle 1 is special at step 5; the others collide
    as usual.  The expected values are the oracle's unchanged: np.maximum(0,
    NaN) is NaN for every sample of that step, so a NaN coordinate makes every
    residual NaN (cvar and saa 0, mmd_random NaN) wherever the obstacle's x
    is, and leaves the lane cost, which no obstacle enters, alone."""
    S, O, H = 65, 3, 12
    ora, draws, st, acc_o, steer_o = make_oracle(cost, "gaussian", S, O, H)
    # the in-lane obstacles for saa too: 0 is expected where a lost NaN would count every sample
    xo, yo = collision_scenario(ora, st, acc_o, steer_o, "cvar")
    xv, yv = SPECIAL[special]
    if xv is not None:
        xo[1, 5] = xv
    if yv is not None:
        yo[1, 5] = yv
    gpu = gpu_risk(native, cost, "gaussian", S, O, H, xo, yo, draws)
    with np.errstate(invalid="ignore"):
        obs, lane, _ = ora.candidate_costs(cost, st, gpu[0], gpu[1], xo, yo, draws, 0)
        if special == "x_inf":
            assert np.all(np.isfinite(obs)) and np.count_nonzero(obs) >= B / 4
        else:
            assert np.all(np.isnan(obs)) if cost == "mmd_random" else not obs.any()
        assert cost == "mmd_random" or np.count_nonzero(lane) >= 1
        print(f"{cost} {special}: GPU obs {gpu[2][:4]}, oracle {obs[:4]}; lane {gpu[3][:4]}, oracle {lane[:4]}")
        assert np.array_equal(np.isnan(gpu[2]), np.isnan(obs)), f"obs_cost NaN-ness: {gpu[2]} vs {obs}"
        assert np.array_equal(np.isnan(gpu[3]), np.isnan(lane)), f"lane_cost NaN-ness: {gpu[3]} vs {lane}"
        compare(cost, "gaussian", ora, st, draws, xo, yo, gpu, degenerate_ok=True)
