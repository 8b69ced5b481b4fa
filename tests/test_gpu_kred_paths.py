"""k_bkernel's three ways to K_red leave the same bits.

K_red of a sample is exp2(D[sel_k][sel_kk] * cs) over its n (n - 1) / 2 row
pairs.  k_bkernel forms the distances D per workgroup by one of three paths,
chosen by the size U of the union of the rows its candidate's samples select:

  table    U (U - 1) / 2 distances of the union once, then lookups
           (ker_tab_bytes(U) <= scratch: U <= 144 .. 165 by n);
  gather   a wave per sample stages the sample's n rows from global memory
           (larger unions);
  image    the union's feature rows once into LDS, every entry from two of
           its rows (U * 112 bytes <= scratch; only when asked for: it
           measured slower than the gather).

MPCMMD_KER_PATH = 0 is the default (table, else gather), 1 never uses the
table (image, else gather), 2 uses the gather for every candidate.  All
three form a distance from the same feature values in the same order
(features 0..21, sequential fp32 sum) and apply the same exp2, so nothing here is a tolerance: what stage 6 writes (bkred, brow,
btop, bcost) is bit-equal between handles made under the three settings and
walked through the beta-iterations on the same draws.

Each case also checks, from bsel, that it ran what it claims: the union
sizes that put a candidate on each path.
"""
import numpy as np
import pytest

import oracle
from parity import DEFAULT_COV, DEFAULT_INIT, DEFAULT_MEAN, make_pair
from test_gpu_launch_invariance import KNOBS, _same, _Side

pytestmark = pytest.mark.gpu

F32 = np.float32
H, O = 10, 3
TBS = (0, 1, 2, 19)
TAB_ROWS = 165          # the largest union whose distance table fits kKerTabMax
ROW_BYTES = 28 * 4      # a feature row staged in LDS (kKerRowPitch floats)


def _scratch(n):
    """ker_scratch: k_bkernel's LDS scratch bytes at reduced size n under
    MPCMMD_KER_PATH=1 (every beta-iteration)."""
    M = n * n
    up = lambda b: (b + 15) & ~15
    fixed = sum(up(b) for b in (100 * n * 2, 400, 800, n * (n - 1), 2 * M, 2 * M, 128))   # ker_lds' persistent pieces
    tab = min(max((79 * 1024 - fixed) & ~15, 55 * 1024), 71 * 1024)                          # ker_tab_budget
    return max(16 * n * ROW_BYTES, min(M * 16 * 4, 64 * 1024), tab)


def _handles(native, monkeypatch, n, B, paths):
    """One handle per MPCMMD_KER_PATH setting, begun on the same draws, after
    stage 1 (and the same controls); the oracle is only asked for shapes."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    sides, ora, d = [], None, None
    for path in paths:
        monkeypatch.setenv("MPCMMD_KER_PATH", str(path))
        if ora is None:
            ora, nat, xo, yo = make_pair(native, "mmd_opt", "gaussian", n=n, O=O, H=H, B=B, T=2, acc_c=0.05,
                                         steer_c=0.01)
            d = oracle.Draws.random(ora.prob, np.random.default_rng(7), idx_mpc=11, seed=0, with_beta_cem=True)
        else:
            nat = native.Handle(native.make_config(n, O, 0.1, H, "gaussian", 0.05, 0.01, num_batch=B,
                                                   variant="static", maxiter_cem=2, device=0, seed=0))
        assert nat.info("ker_path") == path
        nat.begin("mmd_opt", 11, DEFAULT_INIT, DEFAULT_MEAN, DEFAULT_COV, xo, yo, 15.0, d)
        nat.run_stage(1, 0)
        sides.append(_Side(nat, B, n))
    monkeypatch.delenv("MPCMMD_KER_PATH")
    return sides


def _unions(side, s_lo):
    """Distinct mother rows among the selections of samples s_lo.. per candidate."""
    sel = side.get("bsel").reshape(side.B, 100, side.n)[:, s_lo:]
    return np.array([np.unique(c).size for c in sel])


@pytest.mark.parametrize("n,B", [(4, 24), (5, 24), (8, 24), (13, 24), (17, 24), (22, 24), (33, 20)],
                         ids=lambda v: str(v))
def test_kred_paths_bits(native, monkeypatch, n, B):
    """n = 4 (6 entries), 5 (10): fewer entries than lanes, unions of at most
    16 / 25 rows.  n = 8: M = 64, a union of one whole wave.  n = 13: the
    smallest n whose first-iteration union (169 rows) exceeds the table's 165.
    n = 17: two float4s per lane of a distance row, 136 entries in three
    passes of 64 lanes.  n = 22: the benchmark's size, a first-iteration union
    of nearly all 484 rows.  n = 33: the first iteration's union does not fit
    the image either, so the gather runs under every setting, and the
    wave-per-QP kernel follows it."""
    sides = _handles(native, monkeypatch, n, B, (0, 1, 2))
    for s in sides:
        s.nat.run_stage(4, 0)
    for tb in range(20):
        s_lo = 11 if tb > 0 else 0
        for s in sides:
            s.nat.run_stage(5, tb)
            s.nat.run_stage(6, tb)
        if tb in TBS:
            U = _unions(sides[0], s_lo)
            print(f"n = {n}, beta-iteration {tb}: union sizes {U.min()}..{U.max()}, "
                  f"{int((U > TAB_ROWS).sum())} of {B} above the table, "
                  f"{int((U * ROW_BYTES > _scratch(n)).sum())} above the image")
            if tb == 0 and n >= 13:
                assert (U > TAB_ROWS).any(), f"no union above {TAB_ROWS} rows: the table served every candidate"
            if tb == 0 and n == 33:
                assert (U * ROW_BYTES > _scratch(n)).any(), "every union fits the image: the gather never ran"
            if n <= 8:
                assert U.max() <= min(n * n, TAB_ROWS)
            ref = {k: sides[2].get(k) for k in ("bsel", "bkred", "brow", "btop", "bcost")}
            for path, s in zip((0, 1), sides[:2]):
                what = f"MPCMMD_KER_PATH={path} against 2, n = {n}, beta-iteration {tb}"
                _same(f"bsel ({what})", s.get("bsel"), ref["bsel"])
                for k in ("bkred", "brow"):
                    _same(f"{k} ({what})", s.get(k)[:, s_lo:], ref[k][:, s_lo:])
                for k in ("btop", "bcost"):
                    _same(f"{k} ({what})", s.get(k), ref[k])
        for s in sides:
            s.nat.run_stage(7, tb)
    assert np.all(np.isfinite(sides[0].get("bcost")))
    for s in sides:
        s.nat.close()


def test_kred_paths_whole_solve(native, monkeypatch):
    """The whole risk stage (stage 2, default candidate groups) at n = 22,
    B = 24 under MPCMMD_KER_PATH = 0 and 2: the same final outputs."""
    n, B = 22, 24
    sides = _handles(native, monkeypatch, n, B, (0, 2))
    for s in sides:
        s.nat.run_stage(2, 0)
    for k in ("beta", "sigma", "bestsel", "obs_cost", "lane_cost"):
        _same(f"{k} (stage 2, MPCMMD_KER_PATH=0 against 2)", sides[0].get(k), sides[1].get(k))
    assert np.all(np.isfinite(sides[0].get("obs_cost")))
    for s in sides:
        s.nat.close()
