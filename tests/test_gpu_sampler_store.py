"""The samplers' stores into ``ygen`` (betacem_sample.hpp: block_store,
block_store_rows): every real (sample, position) element written exactly once
with the right value, nothing else in the sample rows' range touched.

Which lane and register of a block's MFMA result holds a (sample, position)
element is the samplers' choice, and so is the width of a store; the plane is
not.  Where the sigma coordinate M lands in its block depends on M = n^2 mod
16, which is 0, 1, 4 or 9 only: n = 4, 6, 7, 5 in that order (for a map that
gives a lane four consecutive positions, lane group and register (0, 0),
(0, 1), (1, 0), (2, 1)).  In the one-wave walker the lanes of tiles 4 and 5
whose samples are >= 89 must drop their stores: rows 89..95 of the plane are
never written.

For each n the plane is overwritten with a NaN bit pattern before the samples
of beta-iteration 1 are drawn (stage 5), on a 384-candidate handle (k_bsample,
one wave walks six tiles: raw buffer stores for interior blocks, the generic
store for the last) and on a 20-candidate handle (k_bsample_chunks, one tile
per wave; MPCMMD_FUSED=0), paired as test_gpu_sampler_walk.py pairs them.
Afterwards rows 0..88 x positions 0..M are finite, position M is >= 0.01, the
two handles carry the same bits, and rows 89..95 still hold the pattern.

The fused k_bcem_small (bsample_unit_lds) draws its samples inside one launch
of all 20 beta-iterations, so at n = 6 its plane is overwritten before the
outer iteration and holds the last beta-iteration's samples after it; the
per-iteration kernels of a second 20-candidate handle give the bits.
"""
import numpy as np
import pytest

import oracle
from parity import DEFAULT_COV, DEFAULT_INIT, DEFAULT_MEAN, make_pair

pytestmark = pytest.mark.gpu

F32 = np.float32
BS, BL = 20, 384   # the smallest batch a handle accepts; the smallest launch that takes the walker
ROWS, NEW = 96, 89   # sample rows of a candidate's plane; the rows a beta-iteration draws
POISON = np.uint32(0x7FC0BEEF)   # a quiet NaN
KNOBS = ("MPCMMD_GROUPS", "MPCMMD_SMALL_GROUPS", "MPCMMD_SEL_CAP", "MPCMMD_KER_TARGET", "MPCMMD_DIR_TARGET",
         "MPCMMD_DIR_PAIRS", "MPCMMD_QP_SMALL", "MPCMMD_GENWAVE", "MPCMMD_FUSED")


def _stride(n):
    return (n * n + 1 + 31) & ~31


def _poison(nat):
    words = nat.buffer_bytes("ygen") // 4
    nat.write("ygen", np.full(words, POISON, np.uint32))


def _plane(nat, B, n):
    """The candidates' planes as words: [B, 96, stride]."""
    return nat.read("ygen", np.uint32).reshape(-1, ROWS, _stride(n))[:B].copy()


def _check_plane(what, w, n):
    """Real elements written and sane, the padding rows untouched."""
    M = n * n
    y = w[:, :NEW, :M + 1].view(F32)
    bad = ~np.isfinite(y)
    low = y[:, :, M] < F32(0.01)
    pad = w[:, NEW:, :] != POISON
    print(f"{what}: {int(bad.sum())} of {bad.size} real elements not finite, {int(low.sum())} sigma values below 0.01, "
          f"{int(pad.sum())} of {pad.size} words of rows {NEW}..{ROWS - 1} overwritten")
    assert not bad.any(), f"{what}: element {np.argwhere(bad)[0].tolist()} (candidate, sample, position) not written"
    assert not low.any(), f"{what}: sigma coordinate of {np.argwhere(low)[0].tolist()} (candidate, sample) not clipped"
    assert not pad.any(), f"{what}: padding row word {np.argwhere(pad)[0].tolist()} overwritten"


def _same_bits(what, big, small, n):
    """Candidate j of ``big`` carries the bits of candidate j mod len(small), real elements."""
    M1 = n * n + 1
    a, b = big[:, :NEW, :M1], small[:, :NEW, :M1][np.arange(big.shape[0]) % small.shape[0]]
    ne = a != b
    print(f"{what}: {int(ne.sum())} of {ne.size} words differ")
    assert not ne.any(), f"{what}: first difference at {np.argwhere(ne)[0].tolist()} (candidate, sample, position)"


@pytest.mark.parametrize("n", [4, 5, 6, 7])
def test_walker_and_chunks_write_every_element_once(native, monkeypatch, n):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("MPCMMD_GENWAVE", "0")   # the generators' kernel follows the capacity: pinned on both
    monkeypatch.setenv("MPCMMD_FUSED", "0")
    kw = dict(n=n, O=3, H=10, T=2, acc_c=0.05, steer_c=0.01)
    ora_s, nat_s, xo, yo = make_pair(native, "mmd_opt", "gaussian", B=BS, **kw)
    ora_l, nat_l, _, _ = make_pair(native, "mmd_opt", "gaussian", B=BL, **kw)
    sh_l = oracle.Draws.shapes(ora_l.prob, True)
    rng = np.random.default_rng(3000 + n)
    d_s = oracle.Draws.random(ora_s.prob, rng, idx_mpc=11, seed=0, with_beta_cem=True)
    d_l = oracle.Draws(rng.standard_normal(sh_l["pop0"]).astype(F32), d_s.roll,
                       rng.standard_normal(sh_l["resample"]).astype(F32), d_s.beta_z0, d_s.beta_z, idx_mpc=11, seed=0)
    for nat, d in ((nat_s, d_s), (nat_l, d_l)):
        nat.begin("mmd_opt", 11, DEFAULT_INIT, DEFAULT_MEAN, DEFAULT_COV, xo, yo, 15.0, d)
        nat.run_stage(1, 0)
    tile = np.arange(BL) % BS
    for k in ("acc", "steer"):   # k_mother reads a candidate's controls from these rows only
        nat_l.write(k, nat_s.read(k).reshape(BS, 100)[tile])
    got = {}
    for nat, B in ((nat_s, BS), (nat_l, BL)):
        nat.run_stage(4, 0)
        for s in (5, 6, 7):
            nat.run_stage(s, 0)
        nat.sync()
        _poison(nat)
        nat.run_stage(5, 1)
        nat.sync()
        got[B] = _plane(nat, B, n)
        nat.close()
    _check_plane(f"n = {n}: k_bsample_chunks", got[BS], n)
    _check_plane(f"n = {n}: k_bsample", got[BL], n)
    _same_bits(f"n = {n}: k_bsample against k_bsample_chunks", got[BL], got[BS], n)


def test_fused_small_writes_every_element_once(native, monkeypatch):
    n, H, O, T = 6, 10, 3, 2
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    got = {}
    draws = None
    for fused in (0, 1):
        monkeypatch.setenv("MPCMMD_FUSED", str(fused))
        ora, nat, xo, yo = make_pair(native, "mmd_opt", "gaussian", n=n, O=O, H=H, B=BS, T=T, acc_c=0.05, steer_c=0.01)
        assert nat.info("fused_small") == fused
        if draws is None:
            draws = oracle.Draws.random(ora.prob, np.random.default_rng(3100), idx_mpc=11, seed=0, with_beta_cem=True)
        nat.begin("mmd_opt", 11, DEFAULT_INIT, DEFAULT_MEAN, DEFAULT_COV, xo, yo, 15.0, draws)
        _poison(nat)
        nat.iterate(0, 1)
        nat.sync()
        got[fused] = _plane(nat, BS, n)
        nat.close()
    _check_plane("n = 6: per-iteration kernels", got[0], n)
    _check_plane("n = 6: k_bcem_small", got[1], n)
    _same_bits("n = 6: k_bcem_small against the per-iteration kernels", got[1], got[0], n)
