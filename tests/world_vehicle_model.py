"""NumPy restatement of the surrogate world's routed vehicles (DESIGN.md section
24), the checker of mpcmmd_world_step_host_routed: ``leader``, ``accel``,
``advance`` and ``pose`` written from the design section, in Python floats
(fp64) in the order stated and rounded to fp32 once where the section says so;
``step`` composes them with the restatement of the rest of the world
(tests/world_model.py).  Every NaN an output holds is the quiet NaN."""
import math

import numpy as np

import world_model as wm

F32 = np.float32
SCALARS = ("acc_max", "brake", "gap0", "headway", "length", "lane_tol", "gap_min", "acc_min")
DEFAULTS = dict(acc_max=1.5, brake=2.0, gap0=5.0, headway=1.0, length=4.5, lane_tol=1.75, gap_min=0.5, acc_min=-8.0)


def scalars(**over):
    """The eight scalars as fp32 values (the library holds them in fp32)."""
    return {k: F32(over.get(k, DEFAULTS[k])) for k in SCALARS}


def leader(sc, j, s, d, v, ego):
    """(gap, v_lead) of vehicle j's leader or None.  s, d, v: every vehicle's values before the step;
    ego = (s, d, v) after its move.  Candidates in index order, the ego last; a strictly smaller gap wins."""
    best = None
    cand = [(float(s[k]), float(d[k]), F32(v[k])) for k in range(len(s)) if k != j] + \
        [(float(ego[0]), float(ego[1]), F32(ego[2]))]
    sj, dj = float(s[j]), float(d[j])
    for sk, dk, vk in cand:
        if not abs(dk - dj) < float(sc["lane_tol"]):
            continue
        if not sk > sj:
            continue
        gap = (sk - sj) - float(sc["length"])
        if best is None or gap < best[0]:
            best = (gap, vk)
    return best


def accel(sc, v, v0, lead):
    """The intelligent-driver model's acceleration, fp64, clipped and rounded once."""
    v, v0 = float(v), float(v0)
    with np.errstate(all="ignore"):
        r = float(np.float64(v) / np.float64(v0))
    free = 1.0 - (r * r) * (r * r)
    inter = 0.0
    if lead is not None:
        gap, vl = lead
        t = v * float(sc["headway"]) + v * (v - float(vl)) / (2.0 * math.sqrt(float(sc["acc_max"]) * float(sc["brake"])))
        ss = float(sc["gap0"]) + (t if t > 0.0 else 0.0)
        g = gap if gap > float(sc["gap_min"]) else float(sc["gap_min"])
        inter = (ss / g) * (ss / g)
    a = float(sc["acc_max"]) * (free - inter)
    a = float(sc["acc_min"]) if a < float(sc["acc_min"]) else a
    a = float(sc["acc_max"]) if a > float(sc["acc_max"]) else a
    return F32(a)


def advance(sc, dt, s, v, v0, lead):
    """(s', v', a) of one vehicle; not (v0 > 0): parked."""
    if not F32(v0) > 0:
        return float(s), F32(0.0), F32(0.0)
    with np.errstate(all="ignore"):
        a = accel(sc, v, v0, lead)
        vn = F32(v) + a * F32(dt)
        vn = F32(0.0) if vn < 0 else vn
        return float(s) + float(vn * F32(dt)), vn, a


def pose(w, s, d, v):
    """The row (x, y, vx, vy, psi) of a vehicle at (s, d) with speed v on w's route."""
    arc, cx, cy = w["route_arc"], w["spline_x"], w["spline_y"]
    s, v = float(s), F32(v)
    if math.isnan(s):
        return np.full(5, np.nan, F32)
    p = int(np.clip(np.searchsorted(arc, s, side="right") - 1, 0, arc.size - 2))
    h = s - float(arc[p])

    def value(c):   # scipy PPoly's term order
        res = 0.0 + float(c[3, p]) * 1.0
        z = h
        res = res + float(c[2, p]) * z
        z = z * h
        res = res + float(c[1, p]) * z
        z = z * h
        return res + float(c[0, p]) * z

    def slope(c):
        return (3.0 * float(c[0, p]) * h + 2.0 * float(c[1, p])) * h + float(c[2, p])

    with np.errstate(all="ignore"):
        X, Y, tx, ty = value(cx), value(cy), slope(cx), slope(cy)
        nrm = math.sqrt(tx * tx + ty * ty)
        ux, uy = float(np.float64(tx) / np.float64(nrm)), float(np.float64(ty) / np.float64(nrm))
        x, y = F32(X + float(F32(d)) * (-uy)), F32(Y + float(F32(d)) * ux)
        if math.isnan(ux) or math.isnan(uy):
            psi = F32(np.nan)
            sn = cs = F32(np.nan)
        else:
            psi = F32(math.atan2(float(F32(uy)), float(F32(ux))))
            sn, cs = F32(math.sin(float(psi))), F32(math.cos(float(psi)))
        return wm.canon(np.array([x, y, v * cs, v * sn, psi], F32))


def step(w, sc, tick, cx, cy, steer, u, mean, pos, ego, done_tick, veh_s, veh_v, param):
    """One routed step of one episode: the dict of ``world_model.step`` plus veh_s, veh_v and veh_log
    [total_obs, 2] = v, a.  tick < 0: the reset-mode step (no plan read, nothing moves, no log row:
    log_d, log_f, log_i and veh_log come back as zeros)."""
    reset = tick < 0
    frozen = reset or int(done_tick) >= 0
    s = np.array(veh_s, np.float64).reshape(-1)
    v = np.array(veh_v, F32).reshape(-1)
    param = np.asarray(param, F32).reshape(-1, 2)
    V = s.size
    none = np.zeros((0, 5), F32)
    if reset:
        z = lambda n: np.zeros(n, F32)
        cx, cy, steer, u = z(11), z(11), z(4), z(4)
    # the ego's move, its route point and lateral offset: the world without vehicles
    A = wm.step(w, tick, cx, cy, steer, u, mean, pos, ego, none, 0 if frozen else -1)
    acc = np.zeros(V, F32)
    if not frozen:
        e = (A["log_d"][2], A["log_f"][12], A["ego"][0])
        lead = [leader(sc, j, s, param[:, 0], v, e) for j in range(V)]
        for j in range(V):
            s[j], v[j], acc[j] = advance(sc, w["dt"], s[j], v[j], param[j, 1], lead[j])
        v, acc = wm.canon(v), wm.canon(acc)
        s = np.where(np.isnan(s), np.float64(np.nan), s)   # every NaN is stored as the quiet NaN
    rows = np.array([pose(w, s[j], param[j, 0], v[j]) for j in range(V)], F32).reshape(V, 5)
    # everything else of the step reads those rows: a frozen step of the moved ego
    B = wm.step(w, tick, cx, cy, steer, u, mean, A["pos"], A["ego"], rows, 0)
    out = dict(B)
    out["log_f"] = B["log_f"].copy()
    out["log_f"][3:7] = A["log_f"][3:7]   # the controls are those of the state before the move
    collided, goal = bool(B["log_i"][2]), bool(B["log_i"][3])
    out["done_tick"] = np.int32(tick if not frozen and (collided or goal) else done_tick)
    if reset:
        out["log_d"], out["log_f"], out["log_i"] = np.zeros(3), np.zeros(13, F32), np.zeros(4, np.int32)
    log = np.zeros((V, 2), F32) if reset else np.stack([v, acc], 1).astype(F32)
    out.update(vehicles=rows, veh_s=s, veh_v=v, veh_log=log)
    return out


# ---- fixtures the vehicle tests share ------------------------------------------------------------

def straight_route(n=400, spacing=2.0):
    """x = arc, y = 0: the spline pieces of a straight line, exact."""
    rx = np.arange(n) * spacing
    sx = np.zeros((4, n - 1))
    sx[2], sx[3] = 1.0, rx[:-1]
    return rx, np.zeros(n), rx.copy(), sx, np.zeros((4, n - 1))


def traffic(rng, w, ins, E):
    """Random routed vehicles around each episode's ego: (s [E, V] float64, v [E, V], param [E, V, 2])."""
    V = w["total_obs"]
    rx, ry, arc = w["route_x"], w["route_y"], w["route_arc"]
    s0 = np.array([arc[int(np.argmin(np.sqrt((p[0] - rx) ** 2 + (p[1] - ry) ** 2)))] for p in ins["pos"]])
    s = s0[:, None] + rng.uniform(-40.0, 60.0, (E, V))
    d = rng.choice(np.array([0.0, -3.5, 1.0, -1.0], F32), (E, V)) + (rng.random((E, V)) < 0.3) * rng.normal(0, 1, (E, V))
    v = rng.uniform(0.0, 10.0, (E, V)).astype(F32)
    v0 = rng.uniform(3.0, 10.0, (E, V)).astype(F32)
    v0[rng.random((E, V)) < 0.15] = 0.0   # some parked
    v[rng.random((E, V)) < 0.1] = 0.0     # some standing
    return s, v, np.stack([d.astype(F32), v0], -1)


def routed(s, v, param, sc):
    return dict(s=s, v=v, param=param, **{k: float(x) for k, x in sc.items()})
