"""Drop-in replacement of ``synthetic_static_obs/optimizer/cem.py`` (class CEM).

The reference drivers do::

    sys.path.insert(1, 'path/to/optimizer'); from optimizer import cem
    prob = cem.CEM(num_reduced, num_obs, noise_level, num_prime, noise,
                   acc_const_noise, steer_const_noise)            # cem.py:17-18
    prob.compute_cem_mmd_opt(idx_mpc, init_state, mean_param, cov_param,
                             x_obs_traj, y_obs_traj, v_des)          # cem.py:201-204

With ``path/to/optimizer`` pointing at ``mpc-mmd_amd`` the same code runs on
the MI355X through libmpcmmd.so (no JAX).  Constructor and methods keep the
reference's names, argument meaning and return tuples; extra keyword-only
options: ``num_batch`` (reference hard-codes 100, cem.py:137), ``variant``
("static" / "dynamic": the two constants that differ in
synthetic_dynamic_obs), ``maxiter_cem``, ``device``, ``seed``, ``max_configs`` (configurations the
handle holds: the episodes of ``run_episodes``); per call ``draws`` (explicit
standard normals, see include/mpcmmd.h) and ``trace``.  ``run_episodes`` is
this package's own: the receding-horizon loop of DESIGN.md section 21.
"""
from __future__ import annotations

import os

import numpy as np

from . import _native
from .cem_helper import Helper


def _default_device():
    return int(os.environ.get("LOCAL_RANK", "0"))


class CEM:
    def __init__(self, num_reduced, num_obs, noise_level, num_prime, noise, acc_const_noise,
                 steer_const_noise, *, num_batch=100, variant="static", maxiter_cem=20, device=None,
                 seed=0, max_configs=1):
        if noise not in _native.NOISE:
            raise ValueError("noise must be 'gaussian' or 'beta'")
        self.noise = noise
        self.acc_const_noise = acc_const_noise
        self.steer_const_noise = steer_const_noise
        # scalar attributes read by the drivers / validation (cem.py:24-171)
        self.beta_a, self.beta_b = 2, 5
        self.a_obs, self.b_obs = 4.25, 2.75
        self.wheel_base = 2.5
        self.v_max, self.v_min, self.a_max = 30.0, 0.1, 18.0
        self.num_obs = int(num_obs)
        self.steer_max = 0.6
        self.t_fin, self.num = 15, 100
        self.t = self.t_fin / self.num
        self.tot_time = np.linspace(0, self.t_fin, self.num)
        self.num_prime = int(num_prime)
        self.maxiter = 1
        self.maxiter_cem = int(maxiter_cem)
        self.num_params = 8
        self.num_batch = int(num_batch)
        self.ellite_num = 5
        self.ellite_num_projection = self.num_batch
        self.ellite_num_cost = 20
        self.num_reduced = int(num_reduced)
        self.num_mother = self.num_reduced ** 2
        self.variant = variant
        self.y_lb, self.y_ub = (-2.25, 2.25) if variant == "static" else (-2.25, -1.25)
        self.y_des_1, self.y_des_2 = -1.75, 1.75
        self.alpha_quant = self.alpha_quant_lane = 0.98
        self.weight_mmd_lane, self.weight_mmd_obs = 0.0, 1e3
        self.weight_cvar_lane, self.weight_cvar_obs = 0.0, 1e3
        self.weight_saa_lane, self.weight_saa_obs = 1e6, 1e6
        self.ker_wt = 1000.0
        self.sigma_acc = self.sigma_steer = noise_level
        self._cfg = _native.make_config(num_reduced, num_obs, noise_level, num_prime, noise,
                                        acc_const_noise, steer_const_noise, num_batch, variant,
                                        maxiter_cem, _default_device() if device is None else device, seed)
        # bases: fp64 self.P (the reference's NumPy arrays) and fp32 *_jax (cem.py:46-48)
        sh = (self.num, 11)
        self.P = _native.host_constant(self._cfg, "P64").reshape(sh)
        self.Pdot = _native.host_constant(self._cfg, "Pdot64").reshape(sh)
        self.Pddot = _native.host_constant(self._cfg, "Pddot64").reshape(sh)
        self.P_jax = self.P.astype(np.float32)
        self.Pdot_jax = self.Pdot.astype(np.float32)
        self.Pddot_jax = self.Pddot.astype(np.float32)
        self.nvar = 11
        self.cem_helper = Helper(self)
        self._h = _native.Handle(self._cfg, max_configs=int(max_configs))

    # ------------------------------------------------------------------
    def _solve(self, cost, idx_mpc, init_state, mean_param_init, cov_param_init, x_obs_traj, y_obs_traj,
               v_des, draws=None, trace=False):
        r = self._h.solve(cost, idx_mpc, init_state, mean_param_init, cov_param_init, x_obs_traj,
                          y_obs_traj, v_des, draws, trace)
        self.last_trace = r if trace else None
        if cost == "mmd_opt":
            return (r["cx"], r["cy"], r["cost_lane"], r["cost_obs"], r["beta"][:self.num_reduced].copy(),
                    r["sigma"], r["res_beta"])
        return r["cx"], r["cy"], r["cost_lane"], r["cost_obs"]

    def compute_cem_mmd_opt(self, idx_mpc, init_state, mean_param_init, cov_param_init, x_obs_traj,
                            y_obs_traj, v_des, **kw):
        """cem.py:201-333 -> (cx_best, cy_best, mmd_lane, mmd_obs, beta, sigma, res_beta)."""
        return self._solve("mmd_opt", idx_mpc, init_state, mean_param_init, cov_param_init, x_obs_traj,
                           y_obs_traj, v_des, **kw)

    def compute_cem_mmd_random(self, idx_mpc, init_state, mean_param_init, cov_param_init, x_obs_traj,
                               y_obs_traj, v_des, **kw):
        """cem.py:335-462 -> (cx_best, cy_best, mmd_lane, mmd_obs)."""
        return self._solve("mmd_random", idx_mpc, init_state, mean_param_init, cov_param_init, x_obs_traj,
                           y_obs_traj, v_des, **kw)

    def compute_cem_cvar(self, idx_mpc, init_state, mean_param_init, cov_param_init, x_obs_traj,
                         y_obs_traj, v_des, **kw):
        """cem.py:464-588 -> (cx_best, cy_best, cvar_lane, cvar_obs)."""
        return self._solve("cvar", idx_mpc, init_state, mean_param_init, cov_param_init, x_obs_traj,
                           y_obs_traj, v_des, **kw)

    def compute_cem_saa(self, idx_mpc, init_state, mean_param_init, cov_param_init, x_obs_traj,
                        y_obs_traj, v_des, **kw):
        """cem.py:590-714 -> (cx_best, cy_best, saa_lane, saa_obs)."""
        return self._solve("saa", idx_mpc, init_state, mean_param_init, cov_param_init, x_obs_traj,
                           y_obs_traj, v_des, **kw)

    # ------------------------------------------------------------------
    def run_episodes(self, cost, vehicles, starts, ticks, *, chained=True, device_step=None, u=None, key_base=0,
                     keys=None, goal_x=200.0, mean=None, cov=None, v_des=15.0, dt=0.15, validate=None, planned=None):
        """E closed-loop episodes of ``ticks`` ticks in lockstep: solve, apply
        the plan's first control under the noise model, re-solve from the new state, warm-started
        from the previous mean.  vehicles [E, num_obs, 4] = x, y, vx, vy; starts [E, 4] = x, y, vx, vy
        of the ego (a fifth column gives the heading, else atan2(vy, vx)); E <= ``max_configs``.
        u [ticks, E, 3] gives the perturbation variates, None has the step draw them from (keys[e],
        seed, tick); episode e solves tick k with idx_mpc = k + keys[e], keys = key_base + 100003 e
        unless given.

        chained=True runs everything on the GPU with one readback (``_native.Mpc``); a tuple of counts
        splits that run (``run(0, c0)``, ``run(c0, c1)``, ...); False links the ticks through the host:
        ``solve_batch``, the mean read back through ``Handle.read("mean")``, and ``mpc_step`` on the
        host (device_step None) or by the kernel on GPU ``device_step``.  All routes return the same
        bits: a dict of log_d [ticks, E, 2], log_f [ticks, E, 12], log_i [ticks, E, 4]
        (``_native.MPC_LOG_*`` name the columns), every tick's cx, cy [ticks, E, 11] and mean
        [ticks, E, 8], and done_tick [E].

        validate = dict(rollouts=R, alpha=0.98, sigma=(), overlap=True) also computes, per tick and
        episode, the Monte-Carlo risk of the plan that tick made: R fresh noisy
        rollouts of the plan from the tick's state against the tick's tracks.  The chained routes run
        it inside the loop on the GPU (``Mpc.validate``; ``overlap`` puts it on a side stream); the
        host-linked routes call ``_native.validate`` and ``_native.validate_risk`` after each tick's
        solve for the E episodes as one batch: the stage's reference and its fallback, same bits.  The
        dict gains val_counts [ticks, E, 2] (count, count_lane), val_count_pos [ticks, E, 3], val_stats
        [ticks, E, 4, 3] (var, cvar, mean, max by obs, lane_lb, lane_ub), val_mmd [ticks, E, 3, S] and
        val_est [ticks, E, 2] (the cost_lane, cost_obs the solve itself estimated).

        planned = dict(target=[E, num_obs, 2], acc=None) has every vehicle follow the dynamic
        driver's lane-tracking QP and re-plan it each tick from its own state
        instead of moving at constant velocity: target = (v_des, y_des) per vehicle, acc
        [E, num_obs, 2] the start accelerations (None: zeros).  All three routes, the same bits; the
        dict gains veh [ticks, E, num_obs, 6]: every vehicle's (x, y, vx, vy, ax, ay) after each tick."""
        h, cfg = self._h, self._cfg
        pl = None
        if planned is not None:
            if set(planned) - {"target", "acc"} or "target" not in planned:
                raise TypeError("run_episodes: planned takes target and acc")
        val = None
        if validate is not None:
            val = dict(alpha=0.98, sigma=(), overlap=True)
            val.update(validate)
            if set(val) != {"rollouts", "alpha", "sigma", "overlap"}:
                raise TypeError("run_episodes: validate takes rollouts, alpha, sigma, overlap")
            val["sigma"] = np.asarray(() if val["sigma"] is None else val["sigma"], np.float32).reshape(-1)
        ticks = int(ticks)
        starts = np.asarray(starts, np.float64)
        starts = starts.reshape(-1, starts.shape[-1])
        E = starts.shape[0]
        if E < 1 or E > h.max_configs:
            raise ValueError(f"{E} episodes: the handle holds 1..{h.max_configs} (CEM(..., max_configs=))")
        f32 = np.float32
        veh = np.ascontiguousarray(np.asarray(vehicles, f32).reshape(E, self.num_obs, 4))
        pos = np.ascontiguousarray(starts[:, :2])
        vxy = starts[:, 2:4].astype(f32)
        psi = starts[:, 4].astype(f32) if starts.shape[1] > 4 else np.arctan2(vxy[:, 1].astype(np.float64),
                                                                               vxy[:, 0].astype(np.float64)).astype(f32)
        vel = np.ascontiguousarray(np.concatenate([vxy, psi[:, None]], 1))
        mean = np.array([15.0] * 4 + [0.0] * 4, f32) if mean is None else np.asarray(mean, f32)
        mean = np.ascontiguousarray(np.broadcast_to(mean.reshape(-1, 8), (E, 8)))
        cov = np.diag([20.0] * 4 + [100.0] * 4).astype(f32) if cov is None else np.asarray(cov, f32).reshape(8, 8)
        keys = (int(key_base) + 100003 * np.arange(E)) if keys is None else np.asarray(keys, np.int64).reshape(E)
        if u is not None:
            u = np.ascontiguousarray(np.asarray(u, f32).reshape(ticks, E, 3))
        model = _native.MpcModel(cfg, cov, _native.pop0_normals(cfg), goal_x=goal_x, dt=dt, a_obs=self.a_obs,
                                 b_obs=self.b_obs)
        if planned is not None:
            acc = planned.get("acc")
            pl = dict(target=np.ascontiguousarray(np.asarray(planned["target"], f32).reshape(E, self.num_obs, 2)),
                      acc=np.zeros((E, self.num_obs, 2), f32) if acc is None else
                      np.ascontiguousarray(np.asarray(acc, f32).reshape(E, self.num_obs, 2)))
        if chained is not False:
            counts = (ticks,) if chained is True else tuple(int(c) for c in chained)
            if sum(counts) != ticks:
                raise ValueError("run_episodes: the chained counts must add up to ticks")
            ctx = _native.Mpc(h, model, max(ticks, 1))
            try:
                if val is not None:   # before the reset: the stage takes effect there
                    ctx.validate(val["rollouts"], val["alpha"], val["sigma"], val["overlap"])
                if pl is not None:    # likewise
                    ctx.plan_vehicles(pl["target"], pl["acc"])
                ctx.reset(pos, vel, veh, mean, cov, u, keys)
                k = 0
                for c in counts:
                    ctx.run(cost, k, c, cov, v_des)
                    k += c
                out = ctx.log(ticks)
                if val is not None:
                    out.update(ctx.validation_log(ticks))
                if pl is not None:
                    out["veh"] = ctx.vehicle_log(ticks)
                return out
            finally:
                ctx.close()
        out = dict(log_d=np.empty((ticks, E, 2)), log_f=np.empty((ticks, E, 12), f32),
                   log_i=np.empty((ticks, E, 4), np.int32), cx=np.empty((ticks, E, 11), f32),
                   cy=np.empty((ticks, E, 11), f32), mean=np.empty((ticks, E, 8), f32))
        if val is not None:
            S = val["sigma"].size
            out.update(val_counts=np.empty((ticks, E, 2), np.int32), val_count_pos=np.empty((ticks, E, 3), np.int32),
                       val_stats=np.empty((ticks, E, 4, 3), f32), val_mmd=np.empty((ticks, E, 3, S), f32),
                       val_est=np.empty((ticks, E, 2), f32))
            # the handle's configuration as the stage reads it: the fp32 fields widened
            plan = dict(num_prime=self.num_prime, noise=self.noise, noise_level=float(cfg.noise_level),
                        acc_const_noise=float(cfg.acc_const_noise), steer_const_noise=float(cfg.steer_const_noise),
                        num_rollouts=int(val["rollouts"]), variant=self.variant, seed=int(cfg.seed),
                        device=int(cfg.device))
        if pl is not None:
            out["veh"] = np.empty((ticks, E, self.num_obs, 6), f32)
        done = np.full(E, -1, np.int32)
        zero = np.zeros((E, 11), f32)
        # tick 0's inputs: the step of a frozen episode writes the inputs of the state it is given
        st = _native.mpc_step(model, -1, zero, zero, np.zeros((E, 3), f32), mean, pos, vel, veh, np.zeros(E, np.int32),
                              device=device_step, planned=pl)
        for k in range(ticks):
            res = h.solve_batch(cost, [int(np.int32(np.uint32((k + int(q)) & 0xFFFFFFFF))) for q in keys],
                                st["init_state"], mean, cov, st["x_obs"], st["y_obs"], v_des)
            mean = h.read("mean", shape=(E, 8)).copy()
            cx, cy = np.stack([r["cx"] for r in res]), np.stack([r["cy"] for r in res])
            if val is not None:   # the plan against the state and the tracks it was solved for
                ins = (cx, cy, st["init_state"], st["x_obs"], st["y_obs"], [(k + int(q)) & 0xFFFFFFFF for q in keys])
                cnt, lane = _native.validate(*ins, **plan)
                rk = _native.validate_risk(*ins, alpha=float(val["alpha"]), sigma=val["sigma"] if S else None, **plan)
                out["val_counts"][k] = np.stack([cnt, lane], 1)
                out["val_count_pos"][k] = rk["count_pos"]
                out["val_stats"][k] = np.stack([rk[n] for n in ("var", "cvar", "mean", "max")], 1)
                out["val_mmd"][k] = rk["mmd"]
                out["val_est"][k] = [(r["cost_lane"], r["cost_obs"]) for r in res]
            st = _native.mpc_step(model, k, cx, cy, None if u is None else u[k], mean, pos, vel, veh, done,
                                  device=device_step, keys=keys, planned=pl)
            pos, vel, veh, done = st["pos"], st["vel"], st["vehicles"], st["done_tick"]
            if pl is not None:
                pl = dict(target=pl["target"], acc=st["veh_acc"])
                out["veh"][k] = st["veh_log"]
            out["cx"][k], out["cy"][k], out["mean"][k] = cx, cy, mean
            for name in ("log_d", "log_f", "log_i"):
                out[name][k] = st[name]
        out["done_tick"] = done
        return out

    # ------------------------------------------------------------------
    def open_campaign(self, vehicles, starts, ticks_per_episode, max_lockstep_ticks, *, slots=None, v_des=15.0,
                      keys=None, key_base=0, planned=None, goal_x=200.0, mean=None, cov=None, dt=0.15):
        """The context of a campaign after its queue reset (``run_campaign`` says what the arguments
        mean): ``(ctx, cov)``, for callers that drive ``ctx.queue_run`` / ``queue_status`` themselves
        and read the result with ``campaign_result``.  Close ``ctx`` before the handle."""
        h, cfg, f32 = self._h, self._cfg, np.float32
        starts = np.asarray(starts, np.float64)
        starts = starts.reshape(-1, starts.shape[-1])
        N = starts.shape[0]
        E = h.max_configs if slots is None else int(slots)
        if N < 1:
            raise ValueError("run_campaign: at least one scene")
        if E < 1 or E > h.max_configs:
            raise ValueError(f"{E} slots: the handle holds 1..{h.max_configs} (CEM(..., max_configs=))")
        veh = np.ascontiguousarray(np.asarray(vehicles, f32).reshape(N, self.num_obs, 4))
        vxy = starts[:, 2:4].astype(f32)
        psi = starts[:, 4].astype(f32) if starts.shape[1] > 4 else np.arctan2(vxy[:, 1].astype(np.float64),
                                                                               vxy[:, 0].astype(np.float64)).astype(f32)
        vel = np.concatenate([vxy, psi[:, None]], 1)
        mean = np.array([15.0] * 4 + [0.0] * 4, f32) if mean is None else np.asarray(mean, f32)
        mean = np.broadcast_to(mean.reshape(-1, 8), (N, 8))
        cov = np.diag([20.0] * 4 + [100.0] * 4).astype(f32) if cov is None else np.asarray(cov, f32).reshape(8, 8)
        keys = (int(key_base) + 100003 * np.arange(N)) if keys is None else np.asarray(keys, np.int64).reshape(N)
        pl = None
        if planned is not None:
            if set(planned) - {"target", "acc"} or "target" not in planned:
                raise TypeError("run_campaign: planned takes target and acc")
            acc = planned.get("acc")
            pl = dict(target=np.asarray(planned["target"], f32).reshape(N, self.num_obs, 2),
                      acc=np.zeros((N, self.num_obs, 2), f32) if acc is None else
                      np.asarray(acc, f32).reshape(N, self.num_obs, 2))
        model = _native.MpcModel(cfg, cov, _native.pop0_normals(cfg), goal_x=goal_x, dt=dt, a_obs=self.a_obs,
                                 b_obs=self.b_obs)
        ctx = _native.Mpc(h, model, max(int(max_lockstep_ticks), 1))
        try:
            if pl is not None:   # turns the policy on; the queue reads its own table, not these staged rows
                ctx.plan_vehicles(pl["target"][:1], pl["acc"][:1])
            ctx.queue_reset(E, ticks_per_episode, starts[:, :2], vel, veh, mean, cov,
                            np.broadcast_to(np.asarray(v_des, f32).reshape(-1), (N,)), keys, planned=pl)
        except Exception:
            ctx.close()
            raise
        ctx.planned = pl is not None
        return ctx, cov

    @staticmethod
    def campaign_result(ctx, ticks, ticks_per_episode):
        """The per-scene arrays of a campaign whose first ``ticks`` lockstep ticks were enqueued."""
        from .campaign import cut, lockstep_ticks
        sched = ctx.queue_log()
        log = ctx.log(ticks)
        log.pop("done_tick")   # the slots' words; the scenes' come from the schedule
        if ctx.planned:
            log["veh"] = ctx.vehicle_log(ticks)
        out = cut(log, sched, ticks_per_episode)
        started, finished = ctx.queue_status()
        out.update(sched=sched, lockstep_ticks=lockstep_ticks(sched), started=started, finished=finished)
        return out

    def run_campaign(self, cost, vehicles, starts, ticks_per_episode, *, slots=None, max_lockstep_ticks=None,
                     chunk=None, **kw):
        """N closed-loop scenes through ``slots`` slots (default: ``max_configs``) of the chained loop
        (DESIGN.md section 25): a slot whose episode ends -- a collision, the goal, or
        ``ticks_per_episode`` ticks -- is refilled on the GPU with the next scene at once, so no solve
        works on a finished episode while scenes are left.  vehicles [N, num_obs, 4], starts [N, 4 or
        5], v_des a scalar or [N], keys [N] (default key_base + 100003 i), planned = dict(target=[N,
        num_obs, 2], acc=None), goal_x, mean, cov, dt as ``run_episodes`` takes them for E episodes.
        Every scene's episode equals ``run_episodes`` of that scene alone, bit for bit.

        Runs ``chunk`` lockstep ticks at a time (default: ticks_per_episode), reading the two
        counters in between, until every scene has finished or ``max_lockstep_ticks`` (default:
        (ceil(N / slots) + 1) ticks_per_episode, which always suffices) are spent.  Returns per-scene
        arrays cut from the lockstep log: log_d [ticks_per_episode, N, 2], log_f, log_i, cx, cy, mean
        (and veh with the planned policy) in ``run_episodes``' layout, the rows after a scene's end
        repeating its last row; end_tick, end_reason (``_native.QUEUE_REASONS``) and done_tick [N];
        the raw sched [N, 4]; lockstep_ticks, started and finished."""
        Tp = int(ticks_per_episode)
        N = np.asarray(starts, np.float64).reshape(-1, np.shape(starts)[-1]).shape[0]
        E = self._h.max_configs if slots is None else int(slots)
        budget = (-(-N // max(E, 1)) + 1) * Tp if max_lockstep_ticks is None else int(max_lockstep_ticks)
        chunk = Tp if chunk is None else max(int(chunk), 1)
        ctx, cov = self.open_campaign(vehicles, starts, Tp, budget, slots=slots, **kw)
        try:
            k = 0
            while k < budget:
                c = min(chunk, budget - k)
                ctx.queue_run(cost, k, c, cov)
                k += c
                if ctx.queue_status()[1] >= N:
                    break
            return self.campaign_result(ctx, k, Tp)
        finally:
            ctx.close()

    @property
    def handle(self):
        """The underlying native handle (stage access, streams, profiling)."""
        return self._h
