"""The sampler's block walk (betacem_sample.hpp: walk_blocks) on the block
counts the recorded shapes of test_gpu_generator_operands.py skip, one-wave
walker against k_bsample_chunks, bit for bit.

walk_blocks takes blocks in pairs and peels the last one, alone or after an
unpaired predecessor; the pair loop's stores are the interior ones (no clip,
raw buffer stores in the walker), the last block's the generic one:

  n = 4   17 positions, two blocks: no full pair, the peeled two-block tail,
          whose second block holds the sigma coordinate alone
  n = 5   26 positions, two blocks: the same tail with nine positions and the
          sigma coordinate in the second block
  n = 8   65 positions, five blocks: two pairs, then a single peeled block
          that holds the sigma coordinate alone (two chunks: a fold after the
          second pair)

For each n the same 20 control rows run beta-iterations 0..2 through the stage
API on a 20-candidate handle (k_bsample_chunks: one tile and one chunk of
blocks per wave; MPCMMD_FUSED=0) and, tiled (row j = small row j mod 20), on a
384-candidate handle (k_bsample: one wave walks six tiles and every chunk), as
test_gpu_launch_invariance.py pairs its handles.  After each sampling and
selection (stage 5) the real rows of ``ygen`` (89 new samples x M + 1
positions; from beta-iteration 1, the first that samples), ``bsel`` and
``bsig`` of every large-handle candidate carry the bits of its small-handle
row.  Nothing is compared to a tolerance: both kernels issue block_mfma's
MFMAs on the same operands in the same order.
"""
import numpy as np
import pytest

import oracle
from parity import DEFAULT_COV, DEFAULT_INIT, DEFAULT_MEAN, make_pair

pytestmark = pytest.mark.gpu

F32 = np.float32
BS, BL = 20, 384   # the smallest batch a handle accepts; the smallest launch that takes the walker
KNOBS = ("MPCMMD_GROUPS", "MPCMMD_SMALL_GROUPS", "MPCMMD_SEL_CAP", "MPCMMD_KER_TARGET", "MPCMMD_DIR_TARGET",
         "MPCMMD_DIR_PAIRS", "MPCMMD_QP_SMALL", "MPCMMD_GENWAVE", "MPCMMD_FUSED")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_rows(what, big, small):
    """Row j of ``big`` [BL, ...] carries the bits of row j mod BS of ``small`` [BS, ...]."""
    assert big.shape == (BL,) + small.shape[1:] and small.shape[0] == BS, f"{what}: shapes {big.shape} / {small.shape}"
    ne = _bits(big) != _bits(small)[np.arange(BL) % BS]
    print(f"{what}: {int(ne.sum())} of {ne.size} words differ")
    if ne.any():
        at = np.argwhere(ne)[0].tolist()
        raise AssertionError(f"{what}: {int(ne.sum())} of {ne.size} words differ, first at large row {at[0]} "
                             f"(small row {at[0] % BS}), element {at[1:]}")


def _grab(nat, B, n, with_samples):
    M1 = n * n + 1
    ys = (M1 + 31) & ~31
    out = {"bsel": nat.read("bsel", np.int32).reshape(B, -1).copy(),
           "bsig": nat.read("bsig", F32).reshape(B, -1).copy()}
    if with_samples:
        out["ygen"] = nat.read("ygen", F32).reshape(B, 96, ys)[:, :89, :M1].copy()
    return out


@pytest.mark.parametrize("n", [4, 5, 8])
def test_walker_bits_match_chunks(native, monkeypatch, n):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("MPCMMD_GENWAVE", "0")   # the generators' kernel follows the capacity: pinned on both
    monkeypatch.setenv("MPCMMD_FUSED", "0")
    kw = dict(n=n, O=3, H=10, T=2, acc_c=0.05, steer_c=0.01)
    ora_s, nat_s, xo, yo = make_pair(native, "mmd_opt", "gaussian", B=BS, **kw)
    ora_l, nat_l, _, _ = make_pair(native, "mmd_opt", "gaussian", B=BL, **kw)
    assert nat_s.info("gen_wave") == 0 and nat_l.info("gen_wave") == 0
    sh_s, sh_l = oracle.Draws.shapes(ora_s.prob, True), oracle.Draws.shapes(ora_l.prob, True)
    for k in ("roll", "beta_z0", "beta_z"):
        assert sh_s[k] == sh_l[k], f"draws {k} depend on num_batch: {sh_s[k]} / {sh_l[k]}"
    rng = np.random.default_rng(2000 + n)
    d_s = oracle.Draws.random(ora_s.prob, rng, idx_mpc=11, seed=0, with_beta_cem=True)
    d_l = oracle.Draws(rng.standard_normal(sh_l["pop0"]).astype(F32), d_s.roll,
                       rng.standard_normal(sh_l["resample"]).astype(F32), d_s.beta_z0, d_s.beta_z, idx_mpc=11, seed=0)
    for nat, d in ((nat_s, d_s), (nat_l, d_l)):
        nat.begin("mmd_opt", 11, DEFAULT_INIT, DEFAULT_MEAN, DEFAULT_COV, xo, yo, 15.0, d)
        nat.run_stage(1, 0)
    tile = np.arange(BL) % BS
    for k in ("acc", "steer"):   # k_mother reads a candidate's controls from these rows only
        nat_l.write(k, nat_s.read(k).reshape(BS, 100)[tile])
    for nat in (nat_s, nat_l):
        nat.run_stage(4, 0)
    for tb in range(3):
        got = {}
        for nat, B in ((nat_s, BS), (nat_l, BL)):
            nat.run_stage(5, tb)
            nat.sync()
            got[B] = _grab(nat, B, n, tb > 0)
            nat.run_stage(6, tb)
            nat.run_stage(7, tb)
        for k, small in got[BS].items():
            assert small.dtype.kind != "f" or np.all(np.isfinite(small)), f"{k} at beta-iteration {tb}: not finite"
            _same_rows(f"n = {n}: {k} at beta-iteration {tb}", got[BL][k], small)
        if tb > 0:   # written at all: every position's samples vary, the sigma coordinate is clipped
            y = got[BL]["ygen"]
            assert np.all(np.ptp(y, axis=1) > 0) and np.all(y[:, :, n * n] >= F32(0.01))
    nat_s.close()
    nat_l.close()
