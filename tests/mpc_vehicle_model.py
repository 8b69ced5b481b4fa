"""NumPy restatement of the planned vehicles of the synthetic closed loop,
for the tests that hold mpcmmd_mpc_step_host_planned (and through it the planned k_mpc_step)
against it bit for bit: ``plan``, ``track`` and ``advance`` as sequential fp64 sums over the arrays
mpcmmd_mpc_vehicle_constant returns, each sum started at 0.0, rounded once to fp32 and stored with
the quiet-NaN rule; the whole step composed with ``mpc_world_model.step``.  ``lu_tracks`` is the
independent route: the lane-tracking QP of the dynamic driver (obs_data.compute_obs_guess:
smoothness weight 100, gains k_p_v = k_p = 2, one segment over the 100 points) assembled as its
full KKT system and solved by LU with the accelerations in the boundary rows."""
import numpy as np

import mpc_world_model as mm

F32 = np.float32
SHAPES = dict(kinv_x=(14, 14), kinv_y=(15, 15), colsum_x=(11,), colsum_y=(11,), P=(100, 11), adv=(3, 11))


def constants(nat, dt=0.15):
    return {k: nat.mpc_vehicle_constant(dt, k).reshape(sh) for k, sh in SHAPES.items()}


def _seq(rows, vec):
    """sum_i rows[..., i] * vec[..., i], added in order to 0.0, in fp64 (no pairwise summation)."""
    s = np.zeros(np.broadcast(rows[..., 0], vec[..., 0]).shape)
    for i in range(rows.shape[-1]):
        s = s + rows[..., i] * vec[..., i]
    return s


def plan(K, S, target):
    """S [O, 6] = x, y, vx, vy, ax, ay; target [O, 2] = v_des, y_des -> cxf, cyf [O, 11] fp32."""
    S = np.asarray(S, F32).reshape(-1, 6).astype(np.float64)
    tg = np.asarray(target, F32).reshape(-1, 2).astype(np.float64)
    O = S.shape[0]
    with np.errstate(all="ignore"):
        rx = np.concatenate([(-2.0 * tg[:, 0:1]) * K["colsum_x"][None, :], S[:, [0, 2, 4]]], 1)
        ry = np.concatenate([(-2.0 * tg[:, 1:2]) * K["colsum_y"][None, :], S[:, [1, 3, 5]], np.zeros((O, 1))], 1)
        cx = _seq(K["kinv_x"][None, :11, :], rx[:, None, :])
        cy = _seq(K["kinv_y"][None, :11, :], ry[:, None, :])
        return mm.canon(cx.astype(F32)), mm.canon(cy.astype(F32))


def track(K, c):
    """c [O, 11] fp32 -> [O, 100] fp32."""
    with np.errstate(all="ignore"):
        return mm.canon(_seq(K["P"][None, :, :], np.asarray(c, F32).astype(np.float64)[:, None, :]).astype(F32))


def advance(K, cxf, cyf):
    """S' [O, 6] one tick along the plan."""
    with np.errstate(all="ignore"):
        ax = _seq(K["adv"][None, :, :], cxf.astype(np.float64)[:, None, :]).astype(F32)   # [O, 3]: x, vx, ax
        ay = _seq(K["adv"][None, :, :], cyf.astype(np.float64)[:, None, :]).astype(F32)
        return mm.canon(np.stack([ax[:, 0], ay[:, 0], ax[:, 1], ay[:, 1], ax[:, 2], ay[:, 2]], 1))


def step(K, w, tick, cx, cy, u, mean, pos, vel, vehicles, done_tick, acc, target):
    """One step of one episode with the policy on: the dict of ``mpc_world_model.step`` with the
    vehicles moved by advance(plan(S)), the tracks of plan(S'), and veh_acc [O, 2], veh_log [O, 6]."""
    O = w["num_obs"]
    S = np.concatenate([np.asarray(vehicles, F32).reshape(O, 4), np.asarray(acc, F32).reshape(O, 2)], 1)
    if int(done_tick) < 0 and O:
        S = advance(K, *plan(K, S, target))
    # the rest of the step sees the new positions: rows at rest stay where they are put
    at_rest = np.concatenate([S[:, :2], np.zeros((O, 2), F32)], 1)
    out = mm.step(w, tick, cx, cy, u, mean, pos, vel, at_rest, done_tick)
    cxf, cyf = plan(K, S, target) if O else (np.zeros((0, 11), F32),) * 2
    out.update(vehicles=S[:, :4].copy(), veh_acc=S[:, 4:].copy(), veh_log=S.copy(),
               x_obs=track(K, cxf).reshape(O, 100), y_obs=track(K, cyf).reshape(O, 100))
    return out


def lu_tracks(S, target):
    """The QP solved the long way for S [O, 6], target [O, 2]: x, y [O, 100] fp32."""
    from oracle.problem import bernstein_order10
    t = np.linspace(0, 15, 100)
    P, Pd, Pdd = (m.astype(F32).astype(np.float64) for m in bernstein_order10(t[0], t[-1], t))
    S = np.asarray(S, F32).astype(np.float64).reshape(-1, 6)
    tg = np.asarray(target, F32).astype(np.float64).reshape(-1, 2)
    out = []
    for axis, track_of, rows in ((0, Pd, (P[0], Pd[0], Pdd[0])), (1, P, (P[0], Pd[0], Pdd[0], Pd[-1]))):
        A = Pdd - 2.0 * track_of                       # the tracked quantity: the speed in x, the offset in y
        Q = 100.0 * Pdd.T @ Pdd + A.T @ A
        Aeq = np.vstack(rows)
        n = len(rows)
        KKT = np.block([[Q, Aeq.T], [Aeq, np.zeros((n, n))]])
        xs = np.zeros((S.shape[0], 100), F32)
        for o in range(S.shape[0]):
            b = -2.0 * tg[o, axis] * np.ones(100)
            beq = np.concatenate([S[o, axis::2], np.zeros(n - 3)])
            c = np.linalg.solve(KKT, np.concatenate([A.T @ b, beq]))[:11].astype(F32).astype(np.float64)
            xs[o] = (P @ c).astype(F32)
        out.append(xs)
    return out[0], out[1]
