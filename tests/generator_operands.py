"""The walk that tests/test_gpu_generator_operands.py compares against
recorded arrays and tests/golden/make_generator_operands_golden.py records:
beta-iterations 0..2 of outer iteration 0 through the stage API (stages 5, 6,
7: the per-iteration kernels), then the risk stage as a whole (stage 2: the
fused k_bcem_small where the handle qualifies, else the per-iteration kernels
in their candidate groups), on fixed draws.

Kept per step, for the first two candidates: the W plane of ``gen``, ``genm``,
``phib``, the real rows of ``ygen`` (89 new samples x M + 1 positions) and
``belite`` -- everything the generators' producers (k_belite, k_bgen /
k_bgen_wave) and consumers (k_bsample / k_bsample_chunks, k_bsigma,
k_bcem_small) read or write, except the second plane of ``gen``, which is not
part of the contract (layout.hpp)."""
import numpy as np

from parity import DEFAULT_COV, DEFAULT_INIT, DEFAULT_MEAN, make_pair

NCAND = 2
TBS = (0, 1, 2)
# (n, B, MPCMMD_GENWAVE or None).  n: 6 (M + 1 = 37: three used blocks, one
# pure padding block, one chunk), 12 (145: ten blocks, two chunks, a last block
# whose only position is the sigma coordinate), 22 (485: 31 + 1 blocks, four
# chunks).  B = 384: k_bsample's one-wave walker (nb >= 384), with the quad
# k_bgen of large handles pinned (a 384-candidate handle would take
# k_bgen_wave); B = 20, the smallest batch a handle accepts: k_bsample_chunks,
# k_bgen_wave and, at n <= 16, k_bcem_small in stage 2.
CASES = [(n, B, gw) for n in (6, 12, 22) for B, gw in ((384, "0"), (20, None))]


def case_id(n, B):
    return f"n{n}_B{B}"


def pos_pad(M):
    return (M + 1 + 31) & ~31


def _grab(nat, n, B, with_samples):
    M = n * n
    M1, Pp, nblk = M + 1, pos_pad(M), (M + 1 + 15) // 16
    ys = (M1 + 31) & ~31
    out = {
        "genw": nat.read("gen", np.float64).reshape(B, 2, Pp, 12)[:NCAND, 0].copy(),
        "genm": nat.read("genm", np.float64).reshape(B, Pp)[:NCAND].copy(),
        "phib": nat.read("phib", np.float64).reshape(B, nblk, 66)[:NCAND].copy(),
        "belite": nat.read("belite", np.float32).reshape(2, B, 11, M1)[:, :NCAND].copy(),
    }
    if with_samples:
        out["ygen"] = nat.read("ygen", np.float32).reshape(B, 96, ys)[:NCAND, :89, :M1].copy()
    return out


def walk(native, n, B):
    """{step: {name: array}}, steps "tb0", "tb1", "tb2", "stage2"; and the
    handle's info (gen_wave, fused_small).  The caller sets MPCMMD_GENWAVE."""
    import oracle
    H, O = 10, 3
    ora, nat, xo, yo = make_pair(native, "mmd_opt", "gaussian", n=n, O=O, H=H, B=B, T=2, acc_c=0.05, steer_c=0.01)
    draws = oracle.Draws.random(ora.prob, np.random.default_rng(1000 + n), idx_mpc=11, seed=0, with_beta_cem=True)
    nat.begin("mmd_opt", 11, DEFAULT_INIT, DEFAULT_MEAN, DEFAULT_COV, xo, yo, 15.0, draws)
    nat.run_stage(1, 0)
    nat.run_stage(4, 0)
    steps = {}
    for tb in TBS:
        nat.run_stage(5, tb)
        nat.sync()
        ysamp = _grab(nat, n, B, True)["ygen"] if tb > 0 else None
        nat.run_stage(6, tb)
        nat.run_stage(7, tb)
        nat.sync()
        steps[f"tb{tb}"] = _grab(nat, n, B, False)
        if ysamp is not None:
            steps[f"tb{tb}"]["ygen"] = ysamp
    nat.run_stage(2, 0)
    nat.sync()
    steps["stage2"] = _grab(nat, n, B, True)
    for k in ("beta", "sigma", "res_beta"):
        a = nat.read(k)
        steps["stage2"][k] = a.reshape(B, -1)[:NCAND].copy()
    info = {k: nat.info(k) for k in ("gen_wave", "fused_small")}
    nat.close()
    return steps, info
