"""A candidate's beta-CEM does not depend on the launch it runs in.

The beta-CEM's launch geometry follows the number of candidates of a launch
(nb), the handle's capacity and a few environment knobs: k_bkernel<true> +
k_bdirect_pairs (nb <= 256) or k_bkernel<false> + the row-sorted k_bdirect,
the parts per candidate of both row-sum kernels (ker_split), k_bqp at 64 or
128 threads, the waves per candidate of k_bselect (sel_waves), k_bsample or
k_bsample_chunks (nb >= 384), the fused k_bcem_small, and candidate groups on
separate streams with b0 offsets.  handle.hip claims "a candidate's bits do
not depend on how the batch is split into groups or whether k_bcem_small
runs it"; these tests hold every candidate of a launch to that claim:

  test_candidate_bits_launch_size   the same 24 control rows in a handle of
      24 candidates and, tiled (row j = small row j mod 24), in one of 521:
      every sub-stage output of every one of the 521 candidates carries the
      bits of its small-handle row, and so do the outputs of the whole risk
      stage (stage 2), which is where the fused kernel and the candidate
      groups (default, and MPCMMD_GROUPS=2: 261 + 260 on two streams) apply;
  test_knob_bits                    each launch-geometry knob alone against a
      run with none set;
  test_small_groups_capped          MPCMMD_SMALL_GROUPS above the handle's
      stream slots is capped to them and changes no bit.

Nothing here compares to a tolerance: no launch-size branch or knob reorders
a sum (each row sum and each QP is computed by the same lanes in the same
order wherever its workgroup sits), so every buffer is held bit-equal.
"""
import numpy as np
import pytest

import oracle
from parity import DEFAULT_COV, DEFAULT_INIT, DEFAULT_MEAN, make_pair

pytestmark = pytest.mark.gpu

F32 = np.float32
BS, BL = 24, 521   # 521 = 21 * 24 + 17: every small row at many packing positions and group offsets

KNOBS = ("MPCMMD_GROUPS", "MPCMMD_SMALL_GROUPS", "MPCMMD_SEL_CAP", "MPCMMD_KER_TARGET", "MPCMMD_DIR_TARGET",
         "MPCMMD_DIR_PAIRS", "MPCMMD_QP_SMALL", "MPCMMD_GENWAVE", "MPCMMD_FUSED")


def _same_rows(what, big, small):
    """Row j of ``big`` [BL, ...] carries the bits of row j mod BS of ``small``
    [BS, ...]; on a mismatch the first (large row, small row, element)."""
    assert big.shape[1:] == small.shape[1:] and small.shape[0] == BS, f"{what}: shapes {big.shape} / {small.shape}"
    for j0 in range(0, big.shape[0], BS):
        g = big[j0:j0 + BS]
        r = small[:g.shape[0]]
        if np.array_equal(g, r, equal_nan=True):
            continue
        ne = g != r
        if g.dtype.kind == "f":
            ne &= ~(np.isnan(g) & np.isnan(r))
        at = np.argwhere(ne.reshape(g.shape[0], -1))[0]
        row, el = int(at[0]), int(at[1])
        raise AssertionError(f"{what}: large row {j0 + row} differs from small row {row} at element {el}: "
                             f"{g.reshape(g.shape[0], -1)[row, el]!r} vs {r.reshape(g.shape[0], -1)[row, el]!r} "
                             f"({int(ne.sum())} elements of this block of rows differ)")


def _same(what, got, ref):
    if not np.array_equal(got, ref, equal_nan=True):
        ne = got != ref
        if got.dtype.kind == "f":
            ne &= ~(np.isnan(got) & np.isnan(ref))
        raise AssertionError(f"{what}: {int(ne.sum())} elements differ, first at {np.argwhere(ne)[0].tolist()}")


class _Side:
    """One handle and typed reads of its per-candidate buffers [B, ...]."""

    def __init__(self, nat, B, n):
        self.nat, self.B, self.n, self.M = nat, B, n, n * n
        self.Md = (self.M + 255) & ~255
        self.ntri = n * (n - 1) // 2
        self.tri = (self.ntri + 3) & ~3

    def get(self, name):
        B, n, M = self.B, self.n, self.M
        r = self.nat.read
        if name in ("bsel", "bestsel"):
            return r(name, np.int32).reshape(B, -1)
        if name == "bdist":
            return r(name, F32, (B, M, self.Md))[:, :, :M]   # the real columns; the pads are +inf (test_gpu_free_run)
        if name == "bkred":
            return r(name, F32, (B, 100, self.tri))[:, :, :self.ntri]
        if name in ("brow", "btop"):
            return r(name, F32, (B, 100, n))
        if name == "belite":
            return r(name, F32, (2, B, 11, M + 1))
        return r(name).reshape(B, -1)

    def poison(self):
        """Overwrite the beta-CEM's outputs: a launch that skipped a candidate
        would otherwise leave the (equal) values of an earlier run behind."""
        for k in ("beta", "sigma", "res_beta", "btrace", "obs_cost", "lane_cost", "bcost", "btop", "brow", "bsig",
                  "belite"):
            self.nat.write(k, np.full(self.nat.buffer_bytes(k) // 4, np.nan, F32))
        for k in ("bsel", "bestsel"):   # indices: a valid value (a stale read must stay in bounds)
            self.nat.write(k, np.zeros(self.nat.buffer_bytes(k) // 4, np.int32))


FINALS = ("beta", "sigma", "bestsel", "res_beta", "btrace", "obs_cost", "lane_cost")
LEFT = ("bsel", "bsig", "brow", "btop", "bcost", "belite")   # what the last beta-iterations leave behind


@pytest.mark.parametrize("groups", ["default", "groups2"])
@pytest.mark.parametrize("n,genwave", [(6, 0), (6, 1), (17, 0), (17, 1), (33, 0)],
                         ids=["n6-bgen", "n6-bgenwave", "n17-bgen", "n17-bgenwave", "n33-bgen"])
def test_candidate_bits_launch_size(native, monkeypatch, n, genwave, groups):
    """n = 6: M = 36, 220 pad columns; with k_bgen_wave the small handle's
    stage 2 is the fused k_bcem_small, the large one's (nb > 512) the
    per-iteration kernels.  n = 17: the smallest M above 256 (289, two float4s
    per lane), the 24-row quad QP, pair list against row-sorted direct sums,
    8 k_bkernel parts against 1.  n = 33: five float4s per lane, the
    wave-per-QP kernel.  The generators' variant is the one documented
    capacity dependence, so MPCMMD_GENWAVE pins it on both handles.

    The sub-stages (stages 4, then 5 / 6 / 7 per beta-iteration, then 8) go
    through the stage API, which launches all nb candidates of a handle at
    once on its stream: nb = 24 against nb = 521.  The candidate groups and
    k_bcem_small belong to the risk stage as a whole, so stage 2 then runs
    again on both handles over poisoned outputs and must reproduce the
    walked results: the final outputs of every candidate on both handles,
    and on the large handle also what the last beta-iterations leave in the
    per-iteration buffers."""
    H, O, M = 10, 3, n * n
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("MPCMMD_GENWAVE", str(genwave))
    ora_s, nat_s, xo, yo = make_pair(native, "mmd_opt", "gaussian", n=n, O=O, H=H, B=BS, T=2, acc_c=0.05, steer_c=0.01)
    if groups == "groups2":
        monkeypatch.setenv("MPCMMD_GROUPS", "2")
    ora_l, nat_l, _, _ = make_pair(native, "mmd_opt", "gaussian", n=n, O=O, H=H, B=BL, T=2, acc_c=0.05, steer_c=0.01)
    assert nat_l.info("groups") == (2 if groups == "groups2" else 1) and nat_s.info("gen_wave") == genwave
    # the rollout noise rows and the beta tables do not depend on num_batch: both handles get the same ones
    sh_s, sh_l = oracle.Draws.shapes(ora_s.prob, True), oracle.Draws.shapes(ora_l.prob, True)
    for k in ("roll", "beta_z0", "beta_z"):
        assert sh_s[k] == sh_l[k], f"draws {k} depend on num_batch: {sh_s[k]} / {sh_l[k]}"
    rng = np.random.default_rng(5)
    d_s = oracle.Draws.random(ora_s.prob, rng, idx_mpc=11, seed=0, with_beta_cem=True)
    d_l = oracle.Draws(rng.standard_normal(sh_l["pop0"]).astype(F32), d_s.roll,
                       rng.standard_normal(sh_l["resample"]).astype(F32), d_s.beta_z0, d_s.beta_z, idx_mpc=11, seed=0)
    S, L = _Side(nat_s, BS, n), _Side(nat_l, BL, n)
    for side, d in ((S, d_s), (L, d_l)):
        side.nat.begin("mmd_opt", 11, DEFAULT_INIT, DEFAULT_MEAN, DEFAULT_COV, xo, yo, 15.0, d)
        side.nat.run_stage(1, 0)
    tile = np.arange(BL) % BS
    for k in ("acc", "steer"):   # k_mother reads a candidate's controls from these rows only
        nat_l.write(k, nat_s.read(k).reshape(BS, 100)[tile])

    def both(what, names, tb=None, sl=None):
        for k in names:
            a, b = L.get(k), S.get(k)
            if sl is not None:
                a, b = sl(k, a), sl(k, b)
            _same_rows(f"{k}{'' if tb is None else f' at beta-iteration {tb}'} ({what})", a, b)

    for side in (S, L):
        side.nat.run_stage(4, 0)
    both("stage 4", ("ctrl_n", "feat", "bdist", "bmom"))
    for tb in range(20):
        s_lo = 11 if tb > 0 else 0   # rows 0..10 are the carried elites: not rewritten
        for side in (S, L):
            side.nat.run_stage(5, tb)
        both("stage 5", ("bsel", "bsig"), tb)
        for side in (S, L):
            side.nat.run_stage(6, tb)
        both("stage 6", ("brow",) + (("bkred",) if tb in (0, 1, 19) else ()), tb, lambda k, a: a[:, s_lo:])
        both("stage 6", ("btop", "bcost"), tb)
        for side in (S, L):
            side.nat.run_stage(7, tb)
        both("stage 7", ("belite",), tb, lambda k, a: a[(tb + 1) & 1])
        both("stage 7", ("res_beta", "btrace"), tb, lambda k, a: a[:, tb])
    both("after the last beta-iteration", ("beta", "sigma", "bestsel"))
    for side in (S, L):
        side.nat.run_stage(8, 0)
    both("stage 8", ("obs_cost", "lane_cost"))
    assert np.all(np.isfinite(S.get("obs_cost"))) and np.all(np.isfinite(S.get("bcost")))
    # the risk stage as a whole: k_bcem_small where the handle qualifies, candidate groups where it has them
    walked = {side: {k: side.get(k).copy() for k in FINALS + LEFT} for side in (S, L)}
    for side in (S, L):
        side.poison()
        side.nat.run_stage(2, 0)
    for k in FINALS:
        _same_rows(f"{k} (stage 2 of both handles)", L.get(k), S.get(k))
        for side, nm in ((S, "small"), (L, "large")):
            _same(f"{k} ({nm} handle: stage 2 against its sub-stage walk)", side.get(k), walked[side][k])
    for k in LEFT:
        _same(f"{k} (large handle: stage 2, {groups}, against its sub-stage walk)", L.get(k), walked[L][k])
    nat_s.close()
    nat_l.close()


# -- the launch-geometry knobs ---------------------------------------------------

_REF = {}


def _run_knobs(native, monkeypatch, n, B, env):
    from test_gpu_bcem_small import _run
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return _run(native, monkeypatch, True, "mmd_opt", n, B, 10, 3, 2, keys=("brow",))


def _reference(native, monkeypatch, n, B):
    """The run with no knob set, once per shape."""
    if (n, B) not in _REF:
        _REF[(n, B)] = _run_knobs(native, monkeypatch, n, B, {})
    return _REF[(n, B)]


def _same_run(what, got, ref):
    (og, rg), (orf, rr) = got, ref
    for t, (g, r) in enumerate(zip(og, orf)):
        for k in r:
            if k == "tr":
                assert all(np.array_equal(a, b) for a, b in zip(g[k], r[k])), f"{what}: iteration {t}: elites differ"
            else:
                _same(f"{what}: iteration {t}: {k}", g[k], r[k])
    for k, v in rr.items():
        _same(f"{what}: result {k}", np.asarray(rg[k]), np.asarray(v))


@pytest.mark.parametrize("n,B,knob", [(17, 100, k) for k in (
    "MPCMMD_GROUPS=1", "MPCMMD_GROUPS=3", "MPCMMD_GROUPS=4", "MPCMMD_QP_SMALL=0", "MPCMMD_SEL_CAP=1",
    "MPCMMD_SEL_CAP=16", "MPCMMD_KER_TARGET=1", "MPCMMD_KER_TARGET=100000", "MPCMMD_DIR_TARGET=1",
    "MPCMMD_DIR_TARGET=100000", "MPCMMD_DIR_PAIRS=0")] + [(33, 64, k) for k in (
        "MPCMMD_GROUPS=1", "MPCMMD_GROUPS=4", "MPCMMD_DIR_PAIRS=0")])
def test_knob_bits(native, monkeypatch, n, B, knob):
    """mmd_opt, static, H = 10, O = 3, two outer iterations; n = 17 at B = 100
    and n = 33 at B = 64.  Every setting selects a launch geometry that a
    default run reaches at some batch size (candidate groups, k_bqp's
    workgroup size, k_bselect's waves, the parts of k_bkernel and of the
    direct sums, the row-sorted k_bdirect -- MPCMMD_DIR_PAIRS=0 -- at two and
    at five float4s per lane).  Per outer iteration the
    beta-CEM outputs, the row sums left in brow, the costs and elite sets,
    and the finished result carry the bits of the run with no knob set."""
    ref = _reference(native, monkeypatch, n, B)
    got = _run_knobs(native, monkeypatch, n, B, dict(kv.split("=") for kv in knob.split(",")))
    _same_run(knob, got, ref)


def test_small_groups_capped(native, monkeypatch):
    """MPCMMD_SMALL_GROUPS=9 on a handle of 100 candidates: the handle has
    four group streams, so it runs four groups (it used to index nine), and
    the outputs carry the bits of MPCMMD_SMALL_GROUPS=4."""
    n, B = 17, 100
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("MPCMMD_SMALL_GROUPS", "9")
    h = native.Handle(native.make_config(n, 3, 0.1, 10, "gaussian", 0.0, 0.0, num_batch=B, maxiter_cem=2))
    groups = h.info("groups")
    h.close()
    assert groups == 4
    got = _run_knobs(native, monkeypatch, n, B, {"MPCMMD_SMALL_GROUPS": "9"})
    ref = _run_knobs(native, monkeypatch, n, B, {"MPCMMD_SMALL_GROUPS": "4"})
    _same_run("MPCMMD_SMALL_GROUPS=9 against 4", got, ref)
    _same_run("MPCMMD_SMALL_GROUPS=4 against the default", ref, _reference(native, monkeypatch, n, B))
