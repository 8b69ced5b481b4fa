"""NumPy restatement of the surrogate world, the checker
of mpcmmd_world_step_host: one step of one episode, written from the design
section and the reference's formulas, not from the library's code.  fp32
arithmetic on numpy float32 scalars in the order stated; transcendentals by the
C library's fp64 functions (``math``), rounded once; positions, distances and
the spline in fp64.

Also the fixtures the world tests share: the synthetic route with its splines,
a hairpin route with equidistant legs, and a small world."""
import math
import os
import importlib.util

import numpy as np

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CARLA = os.path.join(ROOT, "mpc-mmd_amd", "carla")


def replay():
    spec = importlib.util.spec_from_file_location("mpcmmd_carla_replay_world", os.path.join(CARLA, "replay.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def canon(a):
    """An fp32 output formed by a subtraction stores every NaN as the quiet NaN 0x7FC00000."""
    return np.where(np.isnan(a), F32(np.nan), a).astype(F32)


def clip_sym(x, m):
    return -m if x < -m else (m if x > m else x)


STREAM_NORMAL, STREAM_ACC_A, STREAM_ACC_B, STREAM_STEER_A, STREAM_STEER_B = 40, 41, 42, 43, 44   # csrc/rng.hpp


def draw(noise, key, seed, tick, a_c, s_c):
    """The variates of (key, seed, tick) from the oracle's restatement of the Philox streams
    (oracle/rng.py): the normals are the library's fp32 values exactly; the Beta draws are the same
    ratio evaluated in fp64 by another formula, so they equal the library's or lie next to them."""
    from oracle import rng as R
    k = (int(key) & 0xFFFFFFFF, int(seed) & 0xFFFFFFFF)
    u = R.philox_normals(k, STREAM_NORMAL, 0, 4 * (tick + 1))[4 * tick:].copy()
    if noise == "beta":
        fa, fs = abs(float(a_c)), abs(float(s_c))
        e = np.array([tick])
        u[0] = R.beta_draws([2 * fa], [5 * fa], k, STREAM_ACC_A, STREAM_ACC_B, e)[0]
        u[1] = R.beta_draws([2 * fs], [5 * fs], k, STREAM_STEER_A, STREAM_STEER_B, e)[0]
    return u


def controller(w, pdot4, cx, cy, steer, v):
    """(a_c, s_c): the first two values of ``control``."""
    return control(w, pdot4, cx, cy, steer, np.zeros(4, F32), v)[:2]


def control(w, pdot4, cx, cy, steer, u, v):
    vb = []
    for i in range(4):
        sx = sy = 0.0
        for k in range(11):
            sx += float(pdot4[i, k]) * float(cx[k])
            sy += float(pdot4[i, k]) * float(cy[k])
        xd, yd = F32(sx), F32(sy)
        vb.append(np.sqrt(xd * xd + yd * yd))
    four = F32(4.0)
    v_c = (((vb[0] + vb[1]) + vb[2]) + vb[3]) / four
    st = [F32(s) for s in steer[:4]]
    s_c = clip_sym((((st[0] + st[1]) + st[2]) + st[3]) / four, w["steer_max"])
    a_c = (v_c - v) / (F32(3.0) * F32(0.15))
    u = [F32(x) for x in u]
    if w["noise"] == "gaussian":
        a = (a_c + (w["sigma_acc"] * np.abs(a_c)) * u[0]) + w["acc_const"] * u[2]
        s = (s_c + (w["sigma_steer"] * np.abs(s_c)) * u[0]) + w["steer_const"] * u[3]
    else:
        a = (a_c + w["sigma_acc"] * (F32(2.0) * u[0] - F32(1.0))) + w["acc_const"] * u[2]
        s = (s_c + w["sigma_steer"] * (F32(2.0) * u[1] - F32(1.0))) + w["steer_const"] * u[3]
    return a_c, s_c, a, clip_sym(s, w["steer_max"])


def ego_step(x, y, v, psi, a, s, dt):
    vn = v + a * dt
    vn = F32(0.0) if vn < 0 else vn
    psidot = vn * F32(math.tan(float(s))) / F32(2.875)
    p = psi + psidot * dt
    sn, cs = F32(math.sin(float(p))), F32(math.cos(float(p)))
    x = x + float(vn * cs * dt)
    y = y + float(vn * sn * dt)
    return x, y, vn, F32(math.atan2(float(sn), float(cs))), psidot


def spline_values(arc, c, s):
    """scipy PPoly's term order on the piece that holds s (the last breakpoint <= s, clamped)."""
    p = np.clip(np.searchsorted(arc, s, side="right") - 1, 0, arc.size - 2)
    h = s - arc[p]
    res = 0.0 + c[3, p] * 1.0
    z = h.copy() if isinstance(h, np.ndarray) else h
    res = res + c[2, p] * z
    z = z * h
    res = res + c[1, p] * z
    z = z * h
    return res + c[0, p] * z


def spline_slope(arc, c, idx):
    p = min(idx, arc.size - 2)
    h = arc[idx] - arc[p]
    return (3.0 * c[0, p] * h + 2.0 * c[1, p]) * h + c[2, p]


def step(w, tick, cx, cy, steer, u, mean, pos, ego, vehicles, done_tick):
    """One step of one episode; ``w`` is the dict of ``small_world``.  Returns the dict of
    ``_native.world_step`` without the episode axis."""
    with np.errstate(all="ignore"):
        return _step(w, tick, cx, cy, steer, u, mean, pos, ego, vehicles, done_tick)


def _step(w, tick, cx, cy, steer, u, mean, pos, ego, vehicles, done_tick):
    dt = w["dt"]
    x, y = float(pos[0]), float(pos[1])
    v, psi, psidot = (F32(t) for t in ego)
    veh = np.array(vehicles, F32).reshape(-1, 5)
    a_c, s_c, a, s = control(w, w["pdot4"], cx, cy, steer, u, v)
    frozen = int(done_tick) >= 0
    if not frozen:
        x, y, v, psi, psidot = ego_step(x, y, v, psi, a, s, dt)
        veh[:, 0] = veh[:, 0] + veh[:, 2] * dt
        veh[:, 1] = veh[:, 1] + veh[:, 3] * dt
    terms = []
    for o in veh:
        dx, dy = F32(x - float(o[0])), F32(y - float(o[1]))
        sn, cs = F32(math.sin(float(o[4]))), F32(math.cos(float(o[4])))
        lo, la = (dx * cs + dy * sn) / w["a_obs"], (-dx * sn + dy * cs) / w["b_obs"]
        terms.append(F32(1.0) - lo * lo - la * la)
    terms = np.array(terms, F32)
    clear = F32(-np.inf) if terms.size == 0 else (F32(np.nan) if np.isnan(terms).any() else terms.max())
    rx, ry, arc = w["route_x"], w["route_y"], w["route_arc"]
    idx = int(np.argmin(np.sqrt((x - rx) ** 2 + (y - ry) ** 2)))   # waypoint_generator (cem_helper.py:264-276)
    s0 = arc[idx]
    tx, ty = spline_slope(arc, w["spline_x"], idx), spline_slope(arc, w["spline_y"], idx)
    d = canon(F32((-(x - rx[idx]) * ty + (y - ry[idx]) * tx) / math.sqrt(tx * tx + ty * ty)))[()]
    lane_out = bool(d < w["y_lb"] or d > w["y_ub"])
    collided = not bool(clear <= 0)
    g = w["goal_index"]
    goal = bool(np.sqrt((x - rx[g]) ** 2 + (y - ry[g]) ** 2) < 7.0)
    if not frozen and (collided or goal):
        done_tick = tick
    look = np.linspace(s0, s0 + 300.0, w["num_path"])
    xw = canon((spline_values(arc, w["spline_x"], look) - x).astype(F32))
    yw = canon((spline_values(arc, w["spline_y"], look) - y).astype(F32))
    # compute_obs_data (main_carla.py:74-150)
    O = w["num_obs"]
    rel = veh[:, :2].astype(np.float64) - np.array([x, y])
    h0, h1 = float(v) * math.cos(float(psi)), float(v) * math.sin(float(psi))
    dot = np.clip(rel[:, 0] * h0 + rel[:, 1] * h1, -1.0, 1.0)
    theta = np.array([math.acos(t) if not math.isnan(t) else math.nan for t in dot])
    keep = veh[theta <= 5 * np.pi / 6]
    if keep.shape[0] == 0:
        keep = np.zeros((O, 5), F32)
        keep[:, :2] = 300.0
    while keep.shape[0] < O:
        keep = np.vstack([keep, keep[-1:]])
    dist = (x - keep[:, 0].astype(np.float64)) ** 2 + (y - keep[:, 1].astype(np.float64)) ** 2
    ob = keep[np.argsort(dist, kind="stable")[:O]].astype(F32)
    ob[:, 0] = canon((ob[:, 0].astype(np.float64) - x).astype(F32))
    ob[:, 1] = canon((ob[:, 1].astype(np.float64) - y).astype(F32))
    # sampling_param (cem_helper.py:122-150) with the run's factor
    L, z = w["chol"], w["pop0"].astype(np.float64)
    pop = np.empty((z.shape[0], 8), F32)
    for a_ in range(8):
        sm = np.full(z.shape[0], float(F32(mean[a_])))
        for c_ in range(a_ + 1):
            sm = sm + L[a_, c_] * z[:, c_]
        pop[:, a_] = sm.astype(F32)
    pop[:, :4] = np.clip(pop[:, :4], F32(0.1), F32(30.0))
    uu = [F32(t) for t in u]
    return dict(pos=np.array([x, y]), ego=np.array([v, psi, psidot], F32), vehicles=veh,
                done_tick=np.int32(done_tick), init_state=np.array([0, 0, v, 0, psi, psidot], F32), x_wp=xw, y_wp=yw,
                obstacles=ob, pop=pop, log_d=np.array([x, y, s0]),
                log_f=np.array([v, psi, psidot, a_c, s_c, a, s, *uu, clear, d], F32),
                log_i=np.array([idx, lane_out, collided, goal], np.int32))


# ---- fixtures --------------------------------------------------------------------------

def route_splines(rx, ry, arc=None):
    """(route_x, route_y, route_arc, spline_x.c, spline_y.c): the drop-in's path_spline grid
    (uniform over the summed chord length) unless ``arc`` is given."""
    from scipy.interpolate import CubicSpline
    rx, ry = np.asarray(rx, np.float64), np.asarray(ry, np.float64)
    if arc is None:
        length = np.cumsum(np.sqrt(np.diff(rx) ** 2 + np.diff(ry) ** 2))[-1]
        arc = np.linspace(0.0, length, rx.size)
    return rx, ry, arc, np.ascontiguousarray(CubicSpline(arc, rx).c), np.ascontiguousarray(CubicSpline(arc, ry).c)


def synthetic_route():
    """replay.synthetic_route + extend_route: 21 k points; (splines tuple, len_path)."""
    R = replay()
    x, y = R.synthetic_route()
    ex, ey = R.extend_route(x, y)
    return route_splines(ex, ey), x.size


def hairpin_route(n_leg=60, gap=8.0, spacing=0.5):
    """130 points: a leg along +x at y = -gap / 2, a half circle of 10 points, a leg back at
    y = +gap / 2.  With the spacing a power of two, an ego at (k spacing, 0) is at bit-equal
    distance from point k of the first leg and its mirror on the second: argmin ties."""
    xs = np.arange(n_leg) * spacing
    r = gap / 2
    th = np.linspace(-np.pi / 2, np.pi / 2, 12)[1:-1]
    x = np.concatenate([xs, xs[-1] + spacing + r * np.cos(th), xs[::-1]])
    y = np.concatenate([np.full(n_leg, -r), r * np.sin(th), np.full(n_leg, r)])
    assert x.size == 130
    return route_splines(x, y), x.size


def small_world(route, goal_index, num_path=37, num_obs=2, total_obs=5, noise="gaussian", B=20, seed=0, **over):
    """The dict ``step`` takes; ``native_model`` makes the library's model from it."""
    rng = np.random.default_rng(seed)
    rx, ry, arc, sx, sy = route
    A = rng.standard_normal((8, 8))
    cov = (A @ A.T + 8 * np.eye(8)).astype(F32)
    w = dict(route_x=rx, route_y=ry, route_arc=arc, spline_x=sx, spline_y=sy, goal_index=int(goal_index),
             num_path=num_path, num_obs=num_obs, total_obs=total_obs, noise=noise, dt=F32(0.05),
             sigma_acc=F32(0.2), sigma_steer=F32(0.1), acc_const=F32(0.05), steer_const=F32(0.01),
             steer_max=F32(0.6), a_obs=F32(4.5), b_obs=F32(3.0), y_lb=F32(-2.5), y_ub=F32(6.0), cov=cov,
             chol=np.linalg.cholesky(cov.astype(np.float64)), pop0=rng.standard_normal((B, 8)).astype(F32))
    w.update(over)
    return w


def native_model(native, w, pdot4, seed=0):
    w["pdot4"] = np.asarray(pdot4, np.float64).reshape(-1)[:44].reshape(4, 11)
    return native.WorldModel(w["route_x"], w["route_y"], w["route_arc"], w["spline_x"], w["spline_y"], w["pdot4"],
                             w["cov"], w["pop0"], w["num_path"], w["num_obs"], w["goal_index"], float(w["y_lb"]),
                             float(w["y_ub"]), w["total_obs"], noise=w["noise"], dt=float(w["dt"]),
                             sigma_acc=float(w["sigma_acc"]), sigma_steer=float(w["sigma_steer"]),
                             acc_const=float(w["acc_const"]), steer_const=float(w["steer_const"]),
                             steer_max=float(w["steer_max"]), a_obs=float(w["a_obs"]), b_obs=float(w["b_obs"]), seed=seed)


def random_inputs(rng, w, E, near=None):
    """E random plans and states near route points (or near ``near`` [E, 2])."""
    rx, ry = w["route_x"], w["route_y"]
    j = rng.integers(0, min(rx.size, 1200), E)
    pos = np.stack([rx[j], ry[j]], 1) + rng.normal(0, 1.5, (E, 2)) if near is None else np.asarray(near, float)
    T = w["total_obs"]
    veh = np.zeros((E, T, 5), F32)
    veh[..., 0] = pos[:, None, 0] + rng.normal(0, 25, (E, T))
    veh[..., 1] = pos[:, None, 1] + rng.normal(0, 25, (E, T))
    veh[..., 2:4] = rng.normal(0, 2, (E, T, 2))
    veh[..., 4] = rng.uniform(-np.pi, np.pi, (E, T))
    return dict(cx=rng.normal(0, 5, (E, 11)).astype(F32), cy=rng.normal(0, 1, (E, 11)).astype(F32),
                steer=rng.normal(0, 0.3, (E, 4)).astype(F32),
                u=(rng.standard_normal((E, 4)) if w["noise"] == "gaussian" else
                   np.concatenate([rng.beta(2, 5, (E, 2)), rng.standard_normal((E, 2))], 1)).astype(F32),
                mean=rng.normal(5, 3, (E, 8)).astype(F32), pos=pos,
                ego=np.stack([rng.uniform(0, 12, E), rng.uniform(-np.pi, np.pi, E), rng.normal(0, 0.2, E)], 1).astype(F32),
                vehicles=veh, done_tick=np.full(E, -1, np.int32))
