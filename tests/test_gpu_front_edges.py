"""k_front (guess QP, one ADMM projection, controls) against the oracle at the
states a closed loop reaches (tests/front_scenarios.py): straight-line
drivers with heading steps of exactly +-float32(pi), standstill and crawl,
overspeed, hard acceleration, an ego off its lane, winding headings whose
unwrap corrects at every place the two-register layout treats specially,
non-finite population entries, a ragged last workgroup, the CARLA steering
branch at the path's ends / on a knot / where 1 - y kappa passes 0, and the
det projection's obstacle terms.  tests/test_front_scenarios.py asserts on
the CPU that each input reaches its path.

Every case is one stage (two for off_lane) on 32 candidates, compared through
parity.close at the lockstep's tolerances (test_gpu_parity_baseline.py):
rtol 1e-4; atol 1e-4 for coefficients and trajectories, 1e-5 for res_norm,
s_lane and steer, 1e-3 for lam_* and acc.  A candidate is left out only where
the oracle's own values sit within 1e-6 (relative, fp64) of a decision
boundary (front_scenarios.excused), at most 5 % per scenario and nobody in
scenarios a, c, d, e, g and h.

Those tolerances cannot see the unwrap: the unwrapped heading enters the
outputs through cos / sin alone, so a missed or extra 2 pi correction moves
them by the fp32 rounding of alpha + 2 pi, about 1e-7 d.  Every comparison is
therefore made a second time at the precision of the number formats (TIGHT).
Kernel and oracle do the same fp32 operations in the same order with
correctly rounded transcendentals; only the order of the fp64 sums behind a
basis product differs (wave reduction against a sequential sum).  That changes
an fp64 sum of n <= 200 terms by at most n 2^-53 sum|terms|, which shows in
the fp32 result as a residue below 1e-12 where the terms cancel to 0, and
otherwise as at most a flipped rounding, one fp32 ulp, that the linear maps
behind it may carry to a few: |gpu - oracle| <= 1e-12 + 4 * 2^-23 |oracle|,
elementwise.  Left at the lockstep's tolerance alone are the outputs that
divide such a residue by a small number: ``steer`` of the straight-line
drivers (y'' x' - y' x'' over |v|^3 where the oracle's y is exactly 0 and
|v| passes 0), and in ``denormal`` the y side, ``lam_y`` and ``steer`` (its
projected velocity is itself of the order of 1e-18; lam_y differs by 1.2e-8
there).
"""
import numpy as np
import pytest

import front_scenarios as F
from parity import DEFAULT_COV, DEFAULT_MEAN, close, make_pair

pytestmark = pytest.mark.gpu

TRAJ = ("x", "y", "xd", "yd", "xdd", "ydd")
TIGHT_ATOL, TIGHT_RTOL = 1e-12, 4 * 2.0 ** -23
LOOSE_ONLY = {"straight": ("steer",), "denormal": ("steer", "cy", "y", "yd", "ydd", "lam_y")}
ATOL = dict(cx=1e-4, cy=1e-4, res_norm=1e-5, lam_x=1e-3, lam_y=1e-3, s_lane=1e-5, acc=1e-3, steer=1e-5, kappa=1e-4,
            **{k: 1e-4 for k in TRAJ})


def _read(nat, nb, carla=False):
    traj = nat.read("traj").reshape(6, -1, 100)[:, :nb]
    out = dict(cx=nat.read("cx").reshape(-1, 11)[:nb], cy=nat.read("cy").reshape(-1, 11)[:nb],
               res_norm=nat.read("res_norm")[:nb], lam_x=nat.read("lam_x").reshape(-1, 11)[:nb],
               lam_y=nat.read("lam_y").reshape(-1, 11)[:nb], s_lane=nat.read("s_lane").reshape(-1, 198)[:nb],
               acc=nat.read("acc").reshape(-1, 100)[:nb], steer=nat.read("steer").reshape(-1, 100)[:nb])
    out.update({k: traj[i] for i, k in enumerate(TRAJ)})
    if carla:
        out["kappa"] = nat.read("kappa_i").reshape(-1, 100)[:nb]
    return {k: v.copy() for k, v in out.items()}


def _reference(pr, acc, steer):
    ref = dict(cx=pr["c_x"], cy=pr["c_y"], res_norm=pr["res_norm"], lam_x=pr["lam_x"], lam_y=pr["lam_y"],
               s_lane=pr["s_lane"], acc=acc[:, :100], steer=steer)
    ref.update({k: pr[k] for k in TRAJ})
    if "kappa" in pr:
        ref["kappa"] = pr["kappa"]
    return ref


def _compare(name, got, ref, keep, skip_points=None, loose_only=()):
    """parity.close on every output over the candidates ``keep``, at the lockstep's tolerance and then at TIGHT
    (but for the outputs ``loose_only``); returns the worst differences."""
    worst = {}
    for k, r in ref.items():
        g, r = got[k][keep], np.asarray(r)[keep]
        if k == "steer" and skip_points is not None:   # points inside the band |1 - y kappa| < 1e-3
            g, r = np.where(skip_points[keep], 0, g), np.where(skip_points[keep], 0, r)
        worst[k] = close(f"{name}:{k}", g, r, atol=ATOL[k])
        if k not in loose_only:
            close(f"{name}:{k} (fp32 precision)", g, r, rtol=TIGHT_RTOL, atol=TIGHT_ATOL)
    print(f"{name}: {int((~keep).sum())} excused; worst |gpu - oracle| " + " ".join(f"{k}={v:.3g}" for k, v in worst.items()))
    return worst


def _write_inputs(nat, sc):
    nat.write("pop", np.concatenate([sc.pop, sc.pop]))   # both halves: stage t reads half t & 1
    for k, v in sc.carries.items():
        nat.write(k, np.asarray(v, np.float32))


def _static_stage(native, sc):
    """begin, write the scenario, run the front ``sc.stages`` times; the GPU's outputs after every stage,
    each checked against the oracle on the carries the GPU's stage started from."""
    ora, nat, xo, yo = make_pair(native, "cvar", "gaussian", n=F.N_S, O=F.O, H=F.H, B=sc.B, T=3, acc_c=0.05,
                                 steer_c=0.01)
    nat.begin("cvar", 123, sc.init, DEFAULT_MEAN, DEFAULT_COV, xo, yo, 15.0)
    _write_inputs(nat, sc)
    st = F.oracle_state(ora.prob, sc)
    outs = []
    for t in range(sc.stages):
        g = F.probe(ora.prob, st)
        ex = F.excused(ora.prob, g)
        assert ex.mean() <= F.EXCUSED_CAP and not (ex.any() and sc.group in F.NO_EXCUSE)
        nat.run_stage(1, t)
        got = _read(nat, sc.B)
        with np.errstate(all="ignore"):
            pr, acc, steer = ora.front(st)
        loose = LOOSE_ONLY.get("straight" if sc.name.startswith("straight") else sc.name, ())
        _compare(f"{sc.name}[{t}]", got, _reference(pr, acc, steer), ~ex, loose_only=loose)
        outs.append(got)
        # the next stage starts from the GPU's own carries, as the lockstep's does
        st["lam_x"], st["lam_y"], st["s_lane"] = got["lam_x"].copy(), got["lam_y"].copy(), got["s_lane"].copy()
    nat.close()
    return outs


STATIC = ["straight-brake", "straight-fwd-rev", "straight-rev-fwd", "standstill", "crawl", "denormal", "reverse",
          "overspeed", "hard_acc", "off_lane+5", "off_lane-5", "off_lane+bound", "off_lane-bound", "winding-reverse",
          "winding-slow_swing", "winding-back_cut", "winding-jerk"]


def _by_name(name):
    return {sc.name: sc for sc in F.static_scenarios()}[name]


def test_names():
    assert STATIC + ["special"] == [sc.name for sc in F.static_scenarios()]


@pytest.mark.parametrize("name", STATIC)
def test_static(native, name):
    _static_stage(native, _by_name(name))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_special(native):
    """NaN / +-inf population entries, one per workgroup on every wave in turn:
    the other candidates are bit-equal to a run without them (wave 1's NaN
    reaches no other wave), the special ones follow the oracle (NaN == NaN)."""
    clean, dirty = F.special()
    ref = _static_stage(native, clean)[0]
    got = _static_stage(native, dirty)[0]
    rows = F.special_rows(dirty)
    for k in ref:
        assert np.array_equal(_bits(ref[k][~rows]), _bits(got[k][~rows])), f"{k}: a special entry reached a neighbour"


@pytest.mark.parametrize("i", range(7))
def test_ragged(native, i):
    """B = 30 (two candidates in the last workgroup): bit-equal to the first 30 of the B = 32 run."""
    full, part = F.ragged()[i]
    ref = _static_stage(native, full)[0]
    got = _static_stage(native, part)[0]
    for k in ref:
        assert np.array_equal(_bits(ref[k][:30]), _bits(got[k])), f"{part.name}: {k} differs from the B = 32 run"


def _carla_stage(native, sc):
    ora = F.carla_oracle()
    nat = native.Handle(native.make_config(F.CARLA_N, F.O, 0.1, F.CARLA_H, "gaussian", 0.0, 0.0, num_batch=sc.B,
                                           maxiter_cem=3, variant="carla_town05"))
    nat.carla_begin(sc.cost, 5, sc.init, F.CARLA_MEAN, F.CARLA_COV, sc.x_obs, sc.y_obs, 10.0, sc.path,
                    F.carla_draws(ora))
    _write_inputs(nat, sc)
    if sc.det_tracks is not None:
        nat.write("obs_full", np.stack([sc.det_tracks[0], sc.det_tracks[1]]).astype(np.float32))
    nat.run_stage(1, 0)
    got = _read(nat, sc.B, carla=True)
    nat.close()
    pr, acc, steer, g, ky = F.carla_front(ora, sc)
    ex = F.excused(ora.prob, g, ky)
    assert ex.mean() <= F.EXCUSED_CAP
    band = F.excused_points(ky)
    ex &= ~band.any(axis=1)     # a candidate in the band only: its steering is left out at those points alone
    _compare(sc.name, got, _reference(pr, acc, steer), ~ex, skip_points=band)
    return got


@pytest.mark.parametrize("i", range(2))
def test_carla(native, i):
    """The p.carla block against CarlaCEM.front_carla: stations clipped at either end of the path, a station on
    an interior knot, and an off-lane ego on the path's curve where 1 - y kappa passes 0."""
    _carla_stage(native, F.carla_scenarios()[i])


@pytest.mark.parametrize("i", range(2))
def test_det(native, i):
    """k_front<true> against compute_projection_det: an obstacle bit-for-bit on a guess point (atan2(0, 0), d
    raised to 1); obstacle coordinates that are not finite.  The oracle's outputs are then NaN throughout, and so
    must the kernel's be: a d_obs of the guess that is not finite makes b_obs, hence every coefficient, NaN, so
    this case holds the NaN propagation (kappa_i through the station clip's NaN guard) and cannot see the one-point
    shift of the kernel's ``nonfin`` flags, which changes no output (k_front.hip says why)."""
    sc = F.det_scenarios()[i]
    got = _carla_stage(native, sc)
    if i == 1:
        assert all(np.isnan(got[k]).all() for k in ("cx", "cy", "res_norm", "lam_x", "lam_y", "steer"))


def _ulps(a, b):
    def key(x):
        i = _bits(x).astype(np.int64)
        return np.where(i < 0x80000000, i, 0x80000000 - i)
    return np.abs(key(a) - key(b))


@pytest.mark.parametrize("name", ["reverse", "default"])
def test_feasible_res_norm(native, name):
    """res_norm of feasible candidates is rounding noise of x - d cos(atan2) (a few 1e-6): the lockstep's atol
    of 1e-5 holds nothing there.  Printed: the share of candidates whose res_norm is bit-equal to the oracle's,
    the worst difference in ulps and the worst relative difference of the multipliers (MI355X: 1.000, 0 ulp, 0
    for both inputs).  Asserted: res_norm within 2 ulp -- it is the fp32 sum of three
    fp32-rounded square roots of fp64 sums, whose order of summation alone differs between the two sides, so a
    rounding may flip in a term and once more in the sum."""
    sc = F.default_input() if name == "default" else _by_name(name)
    got = _static_stage(native, sc)[0]
    ora = F.static_oracle()
    st = F.oracle_state(ora.prob, sc)
    pr, _, _ = ora.front(st)
    ok = pr["res_norm"] < 1e-5
    u = _ulps(got["res_norm"][ok], pr["res_norm"][ok])
    lam = 0.0
    for k in ("lam_x", "lam_y"):
        d, r = np.abs(got[k][ok].astype(np.float64) - pr[k][ok]), np.abs(pr[k][ok].astype(np.float64))
        lam = max(lam, float(np.max(np.where(d == 0, 0.0, d / np.maximum(r, 1e-300)))))
    print(f"{name}: {int(ok.sum())} feasible candidates; res_norm bit-equal {float((u == 0).mean()):.3f}, worst {int(u.max())} "
          f"ulp; worst relative lam difference {lam:.3g}")
    assert ok.sum() >= 1 and u.max() <= 2, f"res_norm of a feasible candidate {int(u.max())} ulp from the oracle's"
