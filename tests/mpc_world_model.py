"""NumPy restatement of the synthetic closed loop's world model:
one step of one episode, every operation in the precision and order the design states, for the
tests that hold mpcmmd_mpc_step_host (and through it k_mpc_step) against it bit for bit.  Scalars
are np.float32 values so NumPy's arithmetic rounds where the library's does; the transcendentals
are the fp64 ``math`` ones, rounded once; the heading of st0 is the host libm's own atan2f (what
``initial_state`` calls), reached through ctypes."""
import ctypes
import ctypes.util
import math

import numpy as np

F32 = np.float32
STREAM_NORMAL, STREAM_ACC_A, STREAM_ACC_B, STREAM_STEER_A, STREAM_STEER_B = 45, 46, 47, 48, 49   # csrc/rng.hpp
TT = np.linspace(0, 15, 100).astype(F32)

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.atan2f.restype = ctypes.c_float
_libm.atan2f.argtypes = [ctypes.c_float, ctypes.c_float]


def atan2f(y, x):
    return F32(_libm.atan2f(float(y), float(x)))


def canon(a):
    """An fp32 output a subtraction may have made a NaN of is stored as the quiet NaN 0x7FC00000."""
    return np.where(np.isnan(a), F32(np.nan), a).astype(F32)[()]


def _m(fn, *a):
    """An fp64 transcendental of ``math`` that passes NaN and infinities through as the libm does."""
    try:
        return fn(*a)
    except (ValueError, OverflowError):
        return math.nan


def draw(noise, key, seed, tick, a_c, s_c):
    """The variates of (key, seed, tick) from the oracle's restatement of the Philox streams
    (oracle/rng.py): the normals are the library's fp32 values exactly; the Beta draws are the same
    ratio evaluated in fp64 by another formula, so they equal the library's or lie next to them."""
    from oracle import rng as R
    k = (int(key) & 0xFFFFFFFF, int(seed) & 0xFFFFFFFF)
    u = R.philox_normals(k, STREAM_NORMAL, 0, 4 * (tick + 1))[4 * tick:4 * tick + 3].copy()
    if noise == "beta":
        fa, fs = abs(float(a_c)), abs(float(s_c))
        e = np.array([tick])
        u[0] = R.beta_draws([2 * fa], [5 * fa], k, STREAM_ACC_A, STREAM_ACC_B, e)[0]
        u[1] = R.beta_draws([2 * fs], [5 * fs], k, STREAM_STEER_A, STREAM_STEER_B, e)[0]
    return u


def _row(row, c):
    s = 0.0
    for k in range(11):
        s += float(row[k]) * float(c[k])
    return F32(s)


def controller(w, cx, cy):
    """(a_c, s_c, curv): compute_controls at step 0."""
    pd, pdd = w["pdot2"], w["pddot1"]
    xd0, yd0, xd1, yd1 = _row(pd[0], cx), _row(pd[0], cy), _row(pd[1], cx), _row(pd[1], cy)
    xdd0, ydd0 = _row(pdd, cx), _row(pdd, cy)
    v0, v1 = np.sqrt(xd0 * xd0 + yd0 * yd0), np.sqrt(xd1 * xd1 + yd1 * yd1)
    a_c = canon((v1 - v0) / F32(0.15))
    s2 = xd0 * xd0 + yd0 * yd0
    curv = canon((ydd0 * xd0 - yd0 * xdd0) / (s2 * np.sqrt(s2)))
    s_c = canon(F32(_m(math.atan, float(curv * F32(2.5)))))
    return a_c, s_c, curv


def perturb(w, a_c, s_c, u):
    u = [F32(x) for x in u]
    if w["noise"] == "gaussian":
        ap = (w["sigma_acc"] * np.abs(a_c)) * u[0]
        sp = (w["sigma_steer"] * np.abs(s_c)) * u[1]
    else:
        ap = w["sigma_acc"] * (F32(2.0) * u[0] - F32(1.0))
        sp = w["K_steer"] * (F32(2.0) * u[1] - F32(1.0))
    return canon((a_c + ap) + w["acc_const"] * u[2]), canon((s_c + sp) + w["steer_const"] * u[2])


def ego_step(x, y, vx, vy, psi, a, s, dt):
    v = np.sqrt(vx * vx + vy * vy)
    v = v + a * dt
    tn = F32(_m(math.tan, float(s)))
    psidot = (v * tn) / F32(2.5)
    p = canon(psi + psidot * dt)
    sn, cs = F32(_m(math.sin, float(p))), F32(_m(math.cos, float(p)))
    nvx, nvy = canon(v * cs), canon(v * sn)
    nx, ny = x + float(nvx * dt), y + float(nvy * dt)
    return nx, ny, nvx, nvy, p, canon((nvx - vx) / dt), canon((nvy - vy) / dt)


def step(w, tick, cx, cy, u, mean, pos, vel, vehicles, done_tick):
    """One step of one episode; ``w`` is the dict of ``small_model``.  Returns the dict of
    ``_native.mpc_step`` without the episode axis."""
    with np.errstate(all="ignore"):
        return _step(w, tick, cx, cy, u, mean, pos, vel, vehicles, done_tick)


def _step(w, tick, cx, cy, u, mean, pos, vel, vehicles, done_tick):
    dt = w["dt"]
    x, y = float(pos[0]), float(pos[1])
    vx, vy, psi = (F32(t) for t in vel)
    veh = np.array(vehicles, F32).reshape(-1, 4)
    a_c, s_c, curv = controller(w, cx, cy)
    a, s = perturb(w, a_c, s_c, u)
    frozen = int(done_tick) >= 0
    ax = ay = F32(0.0)
    if not frozen:
        x, y, vx, vy, psi, ax, ay = ego_step(x, y, vx, vy, psi, a, s, dt)
        veh[:, 0] = veh[:, 0] + veh[:, 2] * dt
        veh[:, 1] = veh[:, 1] + veh[:, 3] * dt
    terms = []
    for o in veh:
        dx, dy = F32(x - float(o[0])), F32(y - float(o[1]))
        lo, la = dx / w["a_obs"], dy / w["b_obs"]
        terms.append(F32(1.0) - lo * lo - la * la)
    terms = np.array(terms, F32)
    clear = F32(-np.inf) if terms.size == 0 else (F32(np.nan) if np.isnan(terms).any() else terms.max())
    lane_out = bool(y < float(w["y_lb"]) or y > float(w["y_ub"]))
    collided = not bool(clear <= 0)
    goal = bool(x >= float(w["goal_x"]))
    if not frozen and (collided or goal):
        done_tick = tick
    init = np.array([canon(F32(x)), canon(F32(y)), vx, vy, ax, ay], F32)
    h = canon(F32(init[3] + init[2])) if (np.isnan(init[2]) or np.isnan(init[3])) else atan2f(init[3], init[2])
    st0 = np.array([init[0], init[1], init[2], init[3], h, 0, 0, 0], F32)
    x_obs = (veh[:, 0:1] + veh[:, 2:3] * TT[None, :]).astype(F32)
    y_obs = (veh[:, 1:2] + veh[:, 3:4] * TT[None, :]).astype(F32)
    L, z = w["chol"], w["pop0"].astype(np.float64)
    pop = np.empty((z.shape[0], 8), F32)
    for a_ in range(8):
        sm = np.full(z.shape[0], float(F32(mean[a_])))
        for c_ in range(a_ + 1):
            sm = sm + L[a_, c_] * z[:, c_]
        pop[:, a_] = sm.astype(F32)
    pop[:, :4] = np.clip(pop[:, :4], F32(0.1), F32(30.0))
    uu = [F32(t) for t in u]
    xn = float("nan") if math.isnan(x) else x   # the canonical fp64 NaN
    yn = float("nan") if math.isnan(y) else y
    return dict(pos=np.array([xn, yn]), vel=np.array([vx, vy, psi], F32), vehicles=veh,
                done_tick=np.int32(done_tick), init_state=init, st0=st0, x_obs=x_obs, y_obs=y_obs, pop=pop,
                log_d=np.array([xn, yn]),
                log_f=np.array([vx, vy, psi, a_c, s_c, a, s, *uu, clear, curv], F32),
                log_i=np.array([lane_out, collided, goal, frozen], np.int32))


# ---- fixtures --------------------------------------------------------------------------

def small_model(native, noise="gaussian", num_obs=2, B=20, seed=0, variant="static", **over):
    """(w, model): the restatement's dict and the native MpcModel of one small configuration."""
    cfg = native.make_config(4, max(num_obs, 1), 0.2, 8, noise, 0.05, 0.02, num_batch=B, variant=variant,
                             maxiter_cem=3, seed=seed)
    rng = np.random.default_rng(99)
    cov = np.diag([20.0] * 4 + [100.0] * 4).astype(F32)
    pop0 = rng.standard_normal((B, 8)).astype(F32)
    model = native.MpcModel(cfg, cov, pop0, goal_x=over.pop("goal_x", 200.0), num_obs=num_obs, **over)
    w = dict(model.scalars)
    w.update(noise=noise, num_obs=num_obs, pdot2=model.arrays["pdot2"], pddot1=model.arrays["pddot1"],
             chol=model.arrays["chol"], pop0=pop0, seed=seed)
    return w, model


def random_inputs(rng, w, E):
    """E random states on a two-lane road with plans that roughly continue them."""
    O = w["num_obs"]
    t = np.linspace(0, 1, 11)
    v0 = rng.uniform(2.0, 15.0, E)
    x0 = rng.uniform(-50.0, 150.0, E)
    y0 = rng.uniform(-4.0, 4.0, E)
    # Bernstein coefficients of a gently curving path: increasing in x, a lateral drift in y
    cx = (x0[:, None] + v0[:, None] * 15.0 * t[None, :] * rng.uniform(0.8, 1.2, (E, 1))
          + rng.normal(0, 0.2, (E, 11))).astype(F32)
    cy = (y0[:, None] + rng.uniform(-3, 3, (E, 1)) * t[None, :] ** 2 + rng.normal(0, 0.05, (E, 11))).astype(F32)
    psi = rng.uniform(-0.3, 0.3, E)
    vel = np.stack([v0 * np.cos(psi), v0 * np.sin(psi), psi], 1).astype(F32)
    veh = np.stack([x0[:, None] + rng.uniform(-30, 60, (E, O)), rng.uniform(-4, 4, (E, O)),
                    rng.uniform(0, 8, (E, O)), rng.uniform(-0.3, 0.3, (E, O))], 2).astype(F32)
    return dict(cx=cx, cy=cy, u=rng.standard_normal((E, 3)).astype(F32) if w["noise"] == "gaussian"
                else np.concatenate([rng.uniform(0, 1, (E, 2)), rng.standard_normal((E, 1))], 1).astype(F32),
                mean=rng.normal(5, 3, (E, 8)).astype(F32), pos=np.stack([x0, y0], 1), vel=vel, vehicles=veh,
                done_tick=np.full(E, -1, np.int32))
