"""Inputs of the front stage (csrc/k_front.hip: guess QP, one ADMM projection,
controls) at the states a closed loop reaches, and one predicate per code
path that says, on the oracle alone, how often an input reaches it.  NumPy and
the oracle only: tests/test_front_scenarios.py asserts the predicates on the
CPU, tests/test_gpu_front_edges.py runs the same inputs through the kernel.

An input is an initial state, a population [B, 8] written over the half of
``pop`` the stage reads (not passed through the sampler's clip: speeds outside
[v_min, v_max] and negative speeds are legal) and, optionally, the carries
``lam_x`` / ``lam_y`` / ``s_lane`` written before the stage.
"""
from __future__ import annotations

import functools

import numpy as np

import oracle
from oracle import helper as Hh
from oracle.helper import cr
from oracle.projection import basis_eval, compute_projection, unwrap

F32 = np.float32
F64 = np.float64
PI = F32(np.pi)
B = 32
N_S, O, H = 24, 3, 12          # the lockstep's handle shape; none of them enters the front
MARGIN = 1e-6                  # relative fp64 margin to a discontinuity below which a candidate is excused
EXCUSED_CAP = 0.05
NO_EXCUSE = ("straight", "overspeed", "hard_acc", "off_lane", "special", "ragged")


class Scenario:
    def __init__(self, name, init, pop, carries=None, stages=1, group=None):
        self.name = name
        self.group = group or name
        self.init = np.asarray(init, F32)
        self.pop = np.ascontiguousarray(pop, F32)
        assert self.pop.ndim == 2 and self.pop.shape[1] == 8
        self.carries = carries or {}
        self.stages = stages

    @property
    def B(self):
        return self.pop.shape[0]

    def __repr__(self):
        return self.name


@functools.lru_cache(maxsize=None)
def static_oracle(num_batch=B):
    return oracle.CEM(N_S, O, 0.1, H, "gaussian", 0.05, 0.01, num_batch=num_batch, maxiter_cem=3)


def oracle_state(prob, sc):
    """The oracle's carry for the scenario's first stage."""
    nb = sc.B
    st = dict(pop=sc.pop.copy(), lam_x=np.zeros((nb, 11), F32), lam_y=np.zeros((nb, 11), F32),
              s_lane=np.zeros((nb, 2 * (prob.num - 1)), F32))
    for k, v in sc.carries.items():
        st[k] = np.array(v, F32).reshape(st[k].shape)
    st["b_eq_x"], st["b_eq_y"] = Hh.compute_boundary_vec(prob, sc.init)
    return st


# ------------------------------------------------------------------ the probe
def unwrap_steps(alpha):
    """(dd, ph) of jnp.unwrap's diff / correction, as oracle.projection.unwrap forms them: [.., 99]."""
    two_pi = F32(2 * np.pi)
    dd = np.diff(np.asarray(alpha, F32), axis=-1)
    with np.errstate(invalid="ignore"):
        ddmod = np.mod(dd + PI, two_pi) - PI
        ddmod = np.where((ddmod == -PI) & (dd > 0), PI, ddmod).astype(F32)
        ph = np.where(np.abs(dd) < PI, F32(0), ddmod - dd).astype(F32)
    return dd, ph


def _polar_raw(wx, wy, do_unwrap):
    """alpha before / after the unwrap and the unclipped d of oracle.projection._polar."""
    raw = cr(np.arctan2, wy, wx)
    alpha = unwrap(raw) if do_unwrap else raw
    ca, sa = cr(np.cos, alpha), cr(np.sin, alpha)
    with np.errstate(invalid="ignore", over="ignore"):
        d = (F32(1.0) * (wx * ca + wy * sa)) / (F32(1.0) * (ca * ca + sa * sa))
    return raw, alpha, d


def probe(prob, st, det_obs=None):
    """The oracle's intermediate values of one front stage on the carry ``st``
    (not modified): guess derivatives, headings before and after the unwrap,
    unclipped d on the guess and on the projected trajectory, the projection's
    outputs ``pr``, s_lane and res_lane."""
    from oracle.projection import compute_projection_det
    with np.errstate(all="ignore"):
        cxb, cyb = Hh.compute_x_guess(prob, st["b_eq_x"], st["b_eq_y"], st["pop"])
        g = dict(cxb=cxb, cyb=cyb)
        g["x"], g["y"] = basis_eval(prob.P, cxb), basis_eval(prob.P, cyb)
        g["xd"], g["yd"] = basis_eval(prob.Pdot, cxb), basis_eval(prob.Pdot, cyb)
        g["xdd"], g["ydd"] = basis_eval(prob.Pddot, cxb), basis_eval(prob.Pddot, cyb)
        g["av_raw"], g["av"], g["dv"] = _polar_raw(g["xd"], g["yd"], True)
        g["aa_raw"], g["aa"], g["da"] = _polar_raw(g["xdd"], g["ydd"], True)
        if det_obs is None:
            pr = compute_projection(prob, st["b_eq_x"], st["b_eq_y"], st["lam_x"], st["lam_y"], cxb, cyb,
                                    st["s_lane"])
        else:
            pr = compute_projection_det(prob, st["b_eq_x"], st["b_eq_y"], st["lam_x"], st["lam_y"], cxb, cyb,
                                        st["s_lane"], det_obs[0], det_obs[1])
        nm1 = prob.num - 1
        b_lane = np.concatenate([np.full(nm1, F32(prob.gamma * prob.y_ub)),
                                 np.full(nm1, F32(-prob.gamma * prob.y_lb))]).astype(F32)
        Ac = basis_eval(prob.A_lane, pr["c_y"])
        g["res_lane"] = ((Ac - b_lane[None, :]) + pr["s_lane"]).astype(F32)
        g["s_lane"] = pr["s_lane"]
        _, _, g["dv_proj"] = _polar_raw(pr["xd"], pr["yd"], False)
        _, _, g["da_proj"] = _polar_raw(pr["xdd"], pr["ydd"], False)
        g["speed_proj"] = np.sqrt(pr["xd"] * pr["xd"] + pr["yd"] * pr["yd"])
        g["pr"] = pr
    return g


# ------------------------------------------------------------------ predicates
def exact_pi_steps(alpha_raw, sign):
    """Number of heading steps of exactly sign * float32(pi)."""
    dd, _ = unwrap_steps(alpha_raw)
    return int((dd == F32(sign) * PI).sum())


def corrections(alpha_raw):
    """The nonzero-correction mask of the unwrap [.., 99] (diff index i is the step t = i -> i + 1)."""
    _, ph = unwrap_steps(alpha_raw)
    return ph != 0


def wrap_rows(alpha_raw):
    """Corrections per row."""
    return corrections(alpha_raw).sum(axis=-1)


def clipped_low(d, lo):
    return int((np.asarray(d) < F32(lo)).sum())


def clipped_high(d, hi):
    return int((np.asarray(d) > F32(hi)).sum())


def slack0_share(g, rows):
    """Share of the lane rows ``rows`` (a slice of the 198) whose slack is exactly 0 while the bound is violated."""
    s, r = g["s_lane"][:, rows], g["res_lane"][:, rows]
    return float(((s == 0) & (r != 0)).mean())


UPPER, LOWER = slice(0, 99), slice(99, 198)

WINDING_FEATURES = tuple(f"corr@{i}" for i in (0, 62, 63, 64, 98)) + ("carry", "both_signs", "beyond_2pi")


def winding_features(alpha_raw, alpha):
    """name -> mask [B] of the rows that show the feature (issue, scenario f)."""
    _, ph = unwrap_steps(alpha_raw)
    nz = ph != 0
    out = {f"corr@{i}": nz[:, i] for i in (0, 62, 63, 64, 98)}
    # diff indices 0..62 are the steps into t = 1..63 (the first register), 63.. into t = 64..99
    out["carry"] = (nz[:, :63].sum(axis=1) >= 2) & (nz[:, 63:].sum(axis=1) >= 1)
    out["both_signs"] = (ph > 0).any(axis=1) & (ph < 0).any(axis=1)
    out["beyond_2pi"] = (np.abs(alpha) > F32(2 * np.pi)).any(axis=1)
    return out


def excused(prob, g, kappa_y=None):
    """Candidates [B] whose oracle values sit within MARGIN (relative, fp64) of
    a discontinuity: |dd| against pi in the guess's unwrap (exact +-pi steps are
    NOT excused: both sides hold correctly rounded headings there and the branch
    under test decides them), an unclipped d against a clip bound it is not
    exactly on, and (CARLA) 1 - y kappa against 0 (``kappa_y`` = y * kappa)."""
    nb = g["av_raw"].shape[0]
    ex = np.zeros(nb, bool)
    with np.errstate(invalid="ignore"):
        for a in (g["av_raw"], g["aa_raw"]):
            dd = np.abs(np.diff(a.astype(F64), axis=-1))
            near = (np.abs(dd - np.pi) < MARGIN * np.pi) & (np.abs(np.diff(a, axis=-1)) != PI)
            ex |= near.any(axis=1)
        for d, bounds in ((g["dv"], (prob.v_min, prob.v_max)), (g["dv_proj"], (prob.v_min, prob.v_max)),
                          (g["da"], (prob.a_max,)), (g["da_proj"], (prob.a_max,))):
            d64 = d.astype(F64)
            for bd in bounds:
                near = (np.abs(d64 - F64(F32(bd))) < MARGIN * bd) & (d != F32(bd))
                ex |= near.any(axis=1)
        if kappa_y is not None:
            ex |= (np.abs(1.0 - kappa_y.astype(F64)) < 1e-3).any(axis=1)
    return ex


def excused_points(kappa_y):
    """CARLA: the points [B, 100] inside the band |1 - y kappa| < 1e-3 (issue, scenario i)."""
    return np.abs(1.0 - np.asarray(kappa_y, F64)) < 1e-3


# ------------------------------------------------------------------ static scenarios a - h
def _pop(speeds, targets, nb=B):
    pop = np.empty((nb, 8), F32)
    pop[:, :4] = np.asarray(speeds, F32)
    pop[:, 4:] = np.asarray(targets, F32)
    return pop


def _init(vx=0.0, y=0.0, x=0.0, vy=0.0, ax=0.0, ay=0.0):
    return np.array([x, y, vx, vy, ax, ay], F32)


def straight():
    """a. y0 = vy0 = ay0 = 0 and every lateral target 0: the guess has y' = y''
    = 0 exactly, so its headings are 0 or +-pi and every step is 0 or exactly
    +-float32(pi).  One scenario per group (the initial state is per solve)."""
    z = np.zeros((B, 4), F32)
    scale = np.linspace(0.8, 1.2, B, dtype=F32)[:, None]
    return [
        Scenario("straight-brake", _init(vx=5.0), _pop(np.array([25, 25, 2, 2], F32)[None] * scale, z), group="straight"),
        Scenario("straight-fwd-rev", _init(vx=3.0), _pop(np.full((B, 4), -5, F32) * scale, z), group="straight"),
        Scenario("straight-rev-fwd", _init(vx=-3.0), _pop(np.full((B, 4), 5, F32) * scale, z), group="straight"),
    ]


def _small_targets():
    rng = np.random.default_rng(21)
    return rng.uniform(-0.5, 0.5, (B, 4)).astype(F32)


def standstill():
    """b. standstill, crawl (init speed 0.05) and denormal (1e-20: xd * xd is an fp32 subnormal)."""
    z = np.zeros((B, 4), F32)
    t = _small_targets()
    # half of the denormal candidates keep y = 0, so that the projected speed stays of the order of 1e-20
    td = t.copy()
    td[::2] = 0
    return [Scenario("standstill", _init(), _pop(z, t), group="standstill"),
            Scenario("crawl", _init(vx=0.05), _pop(z, t), group="standstill"),
            Scenario("denormal", _init(vx=1e-20), _pop(z, td), group="standstill")]


def reverse():
    """An ego that reverses and keeps reversing: feasible (the unwrapped heading stays near pi and d = |v|), so
    res_norm is rounding noise; the velocity heading crosses atan2's cut with every sign change of vy."""
    rng = np.random.default_rng(27)
    return [Scenario("reverse", _init(vx=-5.0, y=1.75), _pop(rng.uniform(-12, -2, (B, 4)), rng.uniform(-2, 2, (B, 4))))]


def overspeed():
    """c. init speed 35, speeds in [28, 45]."""
    rng = np.random.default_rng(22)
    return [Scenario("overspeed", _init(vx=35.0, y=1.75), _pop(rng.uniform(28, 45, (B, 4)), rng.uniform(-2, 2, (B, 4))))]


def hard_acc():
    """d. initial acceleration (25, -20), beyond a_max = 18."""
    rng = np.random.default_rng(23)
    return [Scenario("hard_acc", _init(vx=5.0, y=1.75, ax=25.0, ay=-20.0),
                     _pop(rng.uniform(2, 25, (B, 4)), rng.uniform(-2, 2, (B, 4))))]


def _written_slack(seed, push=0):
    """Nonzero s_lane, a quarter of the entries larger than the lane width
    (4.5).  The projection's lane term pulls y towards (s_lb - s_ub) / 2, so
    ``push`` = +1 keeps the large entries to the lower rows and the upper rows
    small (the written slack then pushes y over the upper bound), -1 the
    reverse, 0 leaves both alike."""
    rng = np.random.default_rng(seed)
    s = rng.uniform(0.0, 2.0, (B, 198)).astype(F32)
    big = rng.random((B, 198)) < 0.25
    s[big] = rng.uniform(5.0, 9.0, int(big.sum())).astype(F32)
    if push:
        small, large = (UPPER, LOWER) if push > 0 else (LOWER, UPPER)
        s[:, small] = rng.uniform(0.01, 0.1, (B, 99)).astype(F32)
        s[:, large] = np.maximum(s[:, large], rng.uniform(3.0, 6.0, (B, 99)).astype(F32))
    return s


def off_lane():
    """e. an ego off its lane, and exactly on either bound; written nonzero
    slacks; two stages (the second on the first one's carries)."""
    rng = np.random.default_rng(24)
    out = []
    for name, y0, tg in (("off_lane+5", 5.0, rng.uniform(3, 7, (B, 4))), ("off_lane-5", -5.0, rng.uniform(-7, -3, (B, 4))),
                         ("off_lane+bound", 2.25, np.full((B, 4), 2.25)), ("off_lane-bound", -2.25, np.full((B, 4), -2.25))):
        tg = np.asarray(tg, F32)
        if "bound" in name:   # a third of the candidates turns back into the lane, the rest leaves it
            out_of = np.sign(y0) * rng.uniform(0.3, 3.0, (B, 4))
            tg = tg + np.where(np.arange(B)[:, None] % 3 == 0, -np.sign(y0) * rng.uniform(0.3, 1.5, (B, 4)), out_of).astype(F32)
        out.append(Scenario(name, _init(vx=5.0, y=y0), _pop(rng.uniform(2, 12, (B, 4)), tg),
                            carries=dict(s_lane=_written_slack(25, int(np.sign(y0)) if "bound" in name else 0)), stages=2,
                            group="off_lane"))
    return out


# f. winding: the seeded search.  Each state is one scenario (the initial state
# is per solve); its 32 candidates are picked from WINDING_DRAWS random ones
# (speeds in [0, 0.5], lateral targets of alternating sign and amplitude up to 8
# with a random first sign) so that the set as a whole shows every feature of
# WINDING_FEATURES on both headings.
WINDING_SEED = 7
WINDING_DRAWS = 4096
WINDING_STATES = (
    ("reverse", dict(vx=-0.3)),
    ("slow_swing", dict(vx=0.2)),
    ("back_cut", dict(vx=-0.02, vy=0.001, ay=-0.05)),
    ("jerk", dict(vx=0.12, ax=-0.02, ay=0.01)),
)


def _winding_draws(rng, n):
    pop = np.empty((n, 8), F32)
    pop[:, :4] = 0.5 * rng.uniform(0.0, 1.0, (n, 4)) ** 3   # in [0, 0.5], dense near 0
    sign = np.where(rng.random((n, 1)) < 0.5, -1.0, 1.0) * np.array([1, -1, 1, -1])[None]
    # amplitudes up to 8, spread (squared uniform) so that the heading crosses its cut at every time index
    pop[:, 4:] = sign * 8.0 * rng.uniform(0.0, 1.0, (n, 4)) ** 2
    return pop


def winding_search():
    """[(name, init, pop [B, 8])]: greedy cover of the features still missing
    over the set, then the rows with the most corrections."""
    prob = static_oracle().prob
    rng = np.random.default_rng(WINDING_SEED)
    need = {(h, f) for h in ("v", "a") for f in WINDING_FEATURES}
    out = []
    for name, kw in WINDING_STATES:
        init = _init(**kw)
        pop = _winding_draws(rng, WINDING_DRAWS)
        bx, by = Hh.compute_boundary_vec(prob, init)
        cxb, cyb = Hh.compute_x_guess(prob, bx, by, pop)
        feats, count = {}, np.zeros(len(pop), int)
        for h, (M, tag) in (("v", (prob.Pdot, "v")), ("a", (prob.Pddot, "a"))):
            raw = cr(np.arctan2, basis_eval(M, cyb), basis_eval(M, cxb))
            for f, m in winding_features(raw, unwrap(raw)).items():
                feats[(h, f)] = m
            count += wrap_rows(raw)
        pick = []
        for key in sorted(need):
            rows = np.nonzero(feats[key])[0]
            rows = [r for r in rows if r not in pick]
            if rows and len(pick) < B - 8:
                pick.append(max(rows, key=lambda r: (sum(bool(feats[k][r]) for k in need), count[r])))
        need -= {k for k in need if any(feats[k][r] for r in pick)}
        rest = [r for r in np.argsort(-count, kind="stable") if r not in pick]
        pick += rest[:B - len(pick)]
        out.append((name, init, pop[np.array(pick)]))
    return out


@functools.lru_cache(maxsize=None)
def _winding_cached():
    return tuple(winding_search())


def winding():
    return [Scenario(f"winding-{name}", init, pop, group="winding") for name, init, pop in _winding_cached()]


SPECIALS = (("nan_speed", 1, np.nan), ("nan_target", 6, np.nan), ("inf_speed", 2, np.inf), ("ninf_speed", 0, -np.inf))


def special():
    """g. (clean, dirty): the dirty population carries one special entry in one
    candidate of each four-candidate workgroup, on every wave position in turn
    (wave 1's NaN first)."""
    rng = np.random.default_rng(26)
    pop = _pop(rng.uniform(2, 25, (B, 4)), rng.uniform(-2, 2, (B, 4)))
    dirty = pop.copy()
    for wg in range(B // 4):
        _, col, val = SPECIALS[wg % 4]
        dirty[4 * wg + (1 + wg) % 4, col] = val
    init = _init(vx=5.0, y=1.75)
    return Scenario("special-clean", init, pop, group="special"), Scenario("special", init, dirty, group="special")


def special_rows(sc):
    return ~np.isfinite(sc.pop).all(axis=1)


def ragged():
    """h. scenarios a and f in a handle of B = 30 (B % 4 = 2): (full, first 30)."""
    out = []
    for sc in straight() + winding():
        out.append((sc, Scenario(sc.name + "-30", sc.init, sc.pop[:30], group="ragged")))
    return out


def default_input():
    """The lockstep's input (tests/test_gpu_parity_baseline.py): DEFAULT_INIT and the sampler's first draw."""
    from parity import DEFAULT_COV, DEFAULT_INIT, DEFAULT_MEAN
    ora = static_oracle()
    draws = oracle.Draws.random(ora.prob, np.random.default_rng(3), idx_mpc=123, seed=0, with_beta_cem=False)
    st = ora.init_state(DEFAULT_INIT, DEFAULT_MEAN, DEFAULT_COV, draws)
    return Scenario("default", DEFAULT_INIT, st["pop"])


def static_scenarios():
    """Every single-handle static scenario of B = 32 (a - f and g's dirty population)."""
    return straight() + standstill() + reverse() + overspeed() + hard_acc() + off_lane() + winding() + [special()[1]]


# ------------------------------------------------------------------ i. the CARLA steering branch
CARLA_TICK, CARLA_H, CARLA_N = 60, 60, 4
CARLA_MEAN = np.array([10.0] * 4 + [0.0] * 4, F32)
CARLA_COV = np.diag([20.0] * 4 + [100.0] * 4).astype(F32)
CURVE_SEED, CURVE_DRAWS = 31, 512


def _replay():
    import importlib.util
    import os
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("mpcmmd_carla_replay",
                                                  os.path.join(here, "mpc-mmd_amd", "carla", "replay.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def carla_oracle(num_batch=B):
    from oracle import carla as K
    return K.CarlaCEM(CARLA_N, 1, O, 0.1, CARLA_H, "gaussian", "Town05", 0.0, 0.0, num_batch=num_batch, maxiter_cem=3)


def carla_draws(ora):
    from oracle import carla as K
    return K.CarlaDraws.random(ora.prob, np.random.default_rng(7), idx_mpc=5, with_beta_cem=False)


@functools.lru_cache(maxsize=None)
def _carla_tick():
    """(init_state_global, x_obs, y_obs, path) of the synthetic replay's tick
    (mpc-mmd_amd/carla/replay.py) as test_gpu_carla.py builds them, through the
    oracle's path helpers (no GPU library on the CPU side)."""
    from oracle import carla as K
    R = _replay()
    rec = R.record_synthetic(ticks=CARLA_TICK + 1)
    init, xw, yw, ob = R.tick_raw_inputs(rec, CARLA_TICK, O)
    xp, yp = K.custom_path_smoothing(xw, yw, 0.1)
    path = K.make_path(xp, yp)
    prob = carla_oracle().prob
    xi, yi, vxi, vyi, pi = K.global_to_frenet_obs(path, ob[:, 0], ob[:, 1], ob[:, 2], ob[:, 3], ob[:, 4])
    xo, yo, _ = Hh.compute_obs_trajectories(prob, xi, yi, vxi, vyi, pi)
    return init, xo, yo, {k: np.asarray(v, F32) for k, v in path.items()}


class CarlaScenario(Scenario):
    def __init__(self, name, init, pop, path, x_obs, y_obs, det_tracks=None, carries=None):
        super().__init__(name, init, pop, carries=carries, group="carla" if det_tracks is None else "det")
        self.path, self.x_obs, self.y_obs = path, x_obs, y_obs
        self.det_tracks = det_tracks      # (x_obs [O, 100], y_obs [O, 100]) written over obs_full before the stage
        self.cost = "cvar" if det_tracks is None else "det"


def carla_state(ora, sc):
    """The oracle's carry after carla_begin, with the scenario's population written."""
    st = ora.init_carla(sc.cost, sc.init, CARLA_MEAN, CARLA_COV, sc.path, carla_draws(ora))
    nb = sc.B     # the front is per candidate: any number of them on the handle's boundary vectors
    st.update(pop=sc.pop.copy(), lam_x=np.zeros((nb, 11), F32), lam_y=np.zeros((nb, 11), F32),
              s_lane=np.zeros((nb, 198), F32))
    for k, v in sc.carries.items():
        st[k] = np.array(v, F32).reshape(st[k].shape)
    return st


def carla_front(ora, sc):
    """(pr, acc, steer, g, kappa_y) of the oracle on the scenario: front_carla's
    outputs, the probe's intermediates and y * kappa [B, 100]."""
    st = carla_state(ora, sc)
    g = probe(ora.prob, st, sc.det_tracks)
    with np.errstate(all="ignore"):
        pr, acc, steer = ora.front_carla(st, sc.path, sc.det_tracks)
        ky = (pr["y"] * pr["kappa"]).astype(F32)
    return pr, acc, steer, g, ky


def _off_path(path, idx, d, v):
    """The global state of an ego ``d`` to the left of path point ``idx``, heading along the path at speed v."""
    fx, fy = float(path["Fx_dot"][idx]), float(path["Fy_dot"][idx])
    n = np.hypot(fx, fy)
    return np.array([path["x_path"][idx] - fy / n * d, path["y_path"][idx] + fx / n * d, v, 0.0, np.arctan2(fy, fx), 0.0],
                    F32)


@functools.lru_cache(maxsize=None)
def _carla_cached():
    ora = carla_oracle()
    init, xo, yo, path = _carla_tick()
    rng = np.random.default_rng(CURVE_SEED)
    # ends: a third reverses past the path's start, a third overruns its end, a third drives on it
    sp = np.concatenate([rng.uniform(-8, -1, (11, 4)), rng.uniform(28, 45, (11, 4)), rng.uniform(4, 12, (10, 4))])
    ends = CarlaScenario("carla-ends", init, _pop(sp, rng.uniform(-3, 0, (B, 4))), path, xo, yo)
    # knot: one interior knot of arc_vec moved onto a projected station of a candidate that drives on the path.
    # The boundary vectors read arc_vec / kappa at the ego's knots (0, 1) only, so the stations do not move
    pr = carla_front(ora, ends)[0]
    arc = path["arc_vec"].copy()
    xs = pr["x"][B - 1, 50]
    i = int(np.argmin(np.abs(arc - xs)))
    assert 3 <= i < arc.size - 1 and arc[i - 1] < xs < arc[i + 1]
    arc[i] = xs
    path = dict(path, arc_vec=arc)
    ends.path = path
    # curve: an ego far to the left of the path's long curve (kappa ~ 0.025), at 0.9 of its radius; written lower
    # slacks push every candidate's y outwards (the lane term pulls y towards the lane centre + (s_lb - s_ub) / 2),
    # through 1 / kappa.  One candidate with a point inside the band |1 - y kappa| < 1e-3 (the cap on excused
    # candidates allows one of 32), the rest outside it but within 0.05
    kap = path["kappa"]
    i0 = int(np.nonzero(kap > 0.024)[0][0]) + 8
    r = 1.0 / float(kap[i0])
    cinit = _off_path(path, i0, 0.9 * r, 0.5)
    pool = _pop(rng.uniform(0.5, 3, (CURVE_DRAWS, 4)), rng.uniform(-3, 0, (CURVE_DRAWS, 4)), CURVE_DRAWS)
    slack = np.zeros((CURVE_DRAWS, 198), F32)
    slack[:, LOWER] = 2 * (rng.uniform(0.95, 1.15, (CURVE_DRAWS, 1)) * r - 0.5 * (ora.prob.y_lb + ora.prob.y_ub))
    ky = carla_front(ora, CarlaScenario("pool", cinit, pool, path, xo, yo, carries=dict(s_lane=slack)))[4]
    inside = excused_points(ky).any(axis=1)
    close_by = (np.abs(1.0 - ky.astype(F64)).min(axis=1) < 0.05) & ~inside
    rows = np.array(list(np.nonzero(inside)[0][:1]) + list(np.nonzero(close_by)[0][:B - 1]))
    assert len(rows) == B, "the curve search found too few candidates"
    curve = CarlaScenario("carla-curve", cinit, pool[rows], path, xo, yo, carries=dict(s_lane=slack[rows]))
    return ends, curve


def carla_scenarios():
    return list(_carla_cached())


# ------------------------------------------------------------------ j. the det projection's obstacle terms
@functools.lru_cache(maxsize=None)
def _det_cached():
    ora = carla_oracle()
    init, xo, yo, _ = _carla_tick()
    path = _carla_cached()[0].path
    rng = np.random.default_rng(41)
    pop = _pop(rng.uniform(4, 12, (B, 4)), rng.uniform(-3, 0, (B, 4)))
    base = CarlaScenario("det-base", init, pop, path, xo, yo, det_tracks=(xo.copy(), yo.copy()))
    g = probe(ora.prob, carla_state(ora, base), base.det_tracks)
    # coincide: obstacle 0 sits bit-for-bit on candidate 5's guess at t = 10 and on candidate 17's at t = 70
    xc, yc = xo.copy(), yo.copy()
    for b, t in ((5, 10), (17, 70)):
        xc[0, t], yc[0, t] = g["x"][b, t], g["y"][b, t]
    coincide = CarlaScenario("det-coincide", init, pop, path, xo, yo, det_tracks=(xc, yc))
    # nonfinite: +inf at guess points t = 63, 0 and 99, NaN at t = 64 (the shift of the flags across the register
    # boundary and at both ends)
    xn, yn = xc.copy(), yc.copy()
    xn[1, 63] = np.inf
    yn[2, 0] = np.inf
    yn[1, 99] = np.inf
    xn[2, 64] = np.nan
    nonfinite = CarlaScenario("det-nonfinite", init, pop, path, xo, yo, det_tracks=(xn, yn))
    return coincide, nonfinite


def det_scenarios():
    return list(_det_cached())


def coincidences(sc, g):
    """(candidate, obstacle, t) where an obstacle of the det tracks sits bit-for-bit on the guess."""
    xo, yo = sc.det_tracks
    hit = (g["x"][:, None, :] == xo[None]) & (g["y"][:, None, :] == yo[None])
    return np.argwhere(hit)
