"""Drop-in replacement of the reference's ``carla/optimizer/cem.py`` (class
CEM of the CARLA experiments).  ``carla/main_carla.py`` does::

    sys.path.insert(1, 'path/to/optimizer'); from optimizer import cem
    prob = cem.CEM(num_reduced, 1, num_obs, noise_level, num_prime, noise, town,
                   acc_const_noise, steer_const_noise)                # main_carla.py:186-187
    cx, cy, v, steering, mean_param = prob.compute_cem_mmd(
        i, init_state_global, mean_param, cov_param, x_obs_traj, y_obs_traj, v_des,
        x_path, y_path, arc_vec, Fx_dot, Fy_dot, kappa)              # :378-382

With ``mpc-mmd_amd/carla`` on sys.path the same calls run on the MI355X
through libmpcmmd.so (mpcmmd_carla_begin / iterate / finish; no JAX).
``compute_cem_mmd``, ``compute_cem_cvar`` and ``compute_cem_det`` (the
deterministic baseline with the obstacle-constrained projection of
projection_det.py) are built, so every ``--costs`` of main_carla.py:188-194
runs.  Extra keyword-only options:
``num_batch`` (reference: 100, cem.py:138), ``maxiter_cem``, ``device``,
``seed``, ``max_configs`` (ticks the one handle solves per launch, default 1);
per call ``draws`` (explicit standard normals incl. ``init_eps``,
include/mpcmmd.h) and ``trace``.  ``compute_cem_batch`` solves up to
``max_configs`` independent ticks in one launch (mpcmmd_carla_solve_batch),
each bit-identical to its ``compute_cem_*`` call; ``compute_cem_tick_batch``
does the same from the raw tick data, with the path and Frenet preprocessing
on the GPU (mpcmmd_carla_tick_solve_batch).
"""
from __future__ import annotations

import os

import numpy as np

from ._lib import native
from .cem_helper import Helper

# cem.py:161-166 tests town == "Town10HD" only: every other name, Town10HD_Opt
# included, gets the Town05 lane bounds and desired lanes
_TOWN = {"Town10HD": "carla_town10hd"}


class CEM:
    def __init__(self, num_reduced_sqrt, num_mother, num_obs, noise_level, num_prime, noise, town,
                 acc_const_noise, steer_const_noise, *, num_batch=100, maxiter_cem=20, device=None, seed=0,
                 max_configs=1):
        N = native()
        if noise not in N.NOISE:
            raise ValueError("noise must be 'gaussian' or 'beta'")
        self.town = town
        self.noise = noise
        self.acc_const_noise = acc_const_noise
        self.steer_const_noise = steer_const_noise
        # scalars the driver reads (cem.py:25-182)
        self.beta_a, self.beta_b = 2, 5
        self.a_obs, self.b_obs = 4.5, 3
        self.wheel_base = 2.875
        self.kappa_max, self.a_centr = 0.230, 1.5
        self.v_max, self.v_min, self.a_max = 30.0, 0.1, 18.0
        self.num_obs = int(num_obs)
        self.steer_max = 0.6
        self.steer_rate_max = 0.6
        self.t_fin, self.num = 15, 100
        self.num_prime = int(num_prime)
        self.t = self.t_fin / self.num
        self.tot_time = np.linspace(0, self.t_fin, self.num)
        self.maxiter, self.maxiter_cem = 1, int(maxiter_cem)
        self.num_params = 8
        self.num_batch = int(num_batch)
        self.ellite_num, self.ellite_num_projection, self.ellite_num_cost = 5, self.num_batch, 20
        self.num_mother = num_mother                      # unused by the reference
        self.num_reduced_sqrt = int(num_reduced_sqrt)
        self.num_reduced = self.num_reduced_sqrt ** 2
        self.variant = _TOWN.get(town, "carla_town05")
        if self.variant == "carla_town10hd":
            self.y_lb, self.y_ub, self.y_des_1, self.y_des_2 = -0.3, 3.8, 0.0, 3.5
        else:
            self.y_lb, self.y_ub, self.y_des_1, self.y_des_2 = -3.8, 0.3, 0.0, -3.5
        self.alpha_quant = self.alpha_quant_lane = 0.98
        self.weight_mmd_lane_des, self.weight_mmd_lane, self.weight_mmd_obs = 0.0, 0.01, 0.1
        self.weight_cvar_lane_des, self.weight_cvar_lane, self.weight_cvar_obs = 0.0, 25, 100
        self.sigma_ker, self.ker_wt = 1e-2, 1000
        self.sigma_acc = self.sigma_steer = noise_level
        self.gamma_lane_des = 0.3
        dev = int(os.environ.get("LOCAL_RANK", "0")) if device is None else device
        self._cfg = N.make_config(num_reduced_sqrt, num_obs, noise_level, num_prime, noise, acc_const_noise,
                                  steer_const_noise, num_batch, self.variant, maxiter_cem, dev, seed)
        sh = (self.num, 11)
        self.P = N.host_constant(self._cfg, "P64").reshape(sh)
        self.Pdot = N.host_constant(self._cfg, "Pdot64").reshape(sh)
        self.Pddot = N.host_constant(self._cfg, "Pddot64").reshape(sh)
        self.P_jax, self.Pdot_jax, self.Pddot_jax = (a.astype(np.float32) for a in (self.P, self.Pdot, self.Pddot))
        self.nvar = 11
        self.cem_helper = Helper(self)
        self.max_configs = int(max_configs)
        self._h = N.Handle(self._cfg, self.max_configs)
        self._ticks = {}

    def _solve(self, cost, idx_mpc, init_state_global, mean_param_init, cov_param_init, x_obs_traj, y_obs_traj,
               v_des, x_path, y_path, arc_vec, Fx_dot, Fy_dot, kappa, draws=None, trace=False):
        path = dict(x_path=x_path, y_path=y_path, arc_vec=arc_vec, Fx_dot=Fx_dot, Fy_dot=Fy_dot, kappa=kappa)
        r = self._h.carla_solve(cost, idx_mpc, init_state_global, mean_param_init, cov_param_init, x_obs_traj,
                                y_obs_traj, v_des, path, draws, trace)
        self.last_result = r
        return r["cx"], r["cy"], r["v_best"].copy(), r["steering"].copy(), r["mean_param"]

    def compute_cem_mmd(self, idx_mpc, init_state_global, mean_param_init, cov_param_init, x_obs_traj, y_obs_traj,
                        v_des, x_path, y_path, arc_vec, Fx_dot, Fy_dot, kappa, **kw):
        """cem.py:217-441 -> (cx_best, cy_best, v_best, steering_best, mean_param)."""
        return self._solve("mmd_opt", idx_mpc, init_state_global, mean_param_init, cov_param_init, x_obs_traj,
                           y_obs_traj, v_des, x_path, y_path, arc_vec, Fx_dot, Fy_dot, kappa, **kw)

    def compute_cem_cvar(self, idx_mpc, init_state_global, mean_param_init, cov_param_init, x_obs_traj, y_obs_traj,
                         v_des, x_path, y_path, arc_vec, Fx_dot, Fy_dot, kappa, **kw):
        """cem.py:444-629 -> (cx_best, cy_best, v_best, steering_best, mean_param)."""
        return self._solve("cvar", idx_mpc, init_state_global, mean_param_init, cov_param_init, x_obs_traj,
                           y_obs_traj, v_des, x_path, y_path, arc_vec, Fx_dot, Fy_dot, kappa, **kw)

    def compute_cem_det(self, idx_mpc, init_state_global, mean_param_init, cov_param_init, x_obs_traj, y_obs_traj,
                        v_des, x_path, y_path, arc_vec, Fx_dot, Fy_dot, kappa, **kw):
        """cem.py:633-790, the deterministic baseline: one noisy initial state
        (cem_helper.py:680-696), the projection with its obstacle terms live
        (projection_det.py), no rollouts and no risk terms ->
        (cx_best, cy_best, v_best, steering_best, mean_param)."""
        return self._solve("det", idx_mpc, init_state_global, mean_param_init, cov_param_init, x_obs_traj,
                           y_obs_traj, v_des, x_path, y_path, arc_vec, Fx_dot, Fy_dot, kappa, **kw)

    def compute_cem_batch(self, cost, idx_mpc, init_states, means, cov, x_obs, y_obs, v_des, paths):
        """len(idx_mpc) <= max_configs independent ticks under one cost ("mmd",
        "cvar" or "det") in one batch: init_states [G, 6], means [G, 8] (or one
        [8]), cov one [8, 8] or [G, 8, 8], x_obs / y_obs [G, O, 100], v_des a
        scalar or [G], paths G dicts of the six path arrays.  Returns a list of
        the reference's 5-tuples (cx_best, cy_best, v_best, steering_best,
        mean_param), tick g's equal to its compute_cem_<cost> call."""
        kinds = {"mmd": "mmd_opt", "cvar": "cvar", "det": "det"}
        if cost not in kinds:
            raise ValueError("cost must be 'mmd', 'cvar' or 'det'")
        rs = self._h.carla_solve_batch(kinds[cost], idx_mpc, init_states, means, cov, x_obs, y_obs, v_des, paths)
        self.last_results = rs
        return [(r["cx"], r["cy"], r["v_best"].copy(), r["steering"].copy(), r["mean_param"]) for r in rs]

    def compute_cem_tick_batch(self, cost, idx_mpc, init_states, x_wp, y_wp, obstacles, threshold, means, cov, v_des):
        """``compute_cem_batch`` from the raw tick data (the tick route,
        mpcmmd_carla_tick_solve_batch): the preprocessing of main_carla.py:
        364-376 runs on the GPU in front of the solve.  x_wp, y_wp [G, num_path]
        the waypoints shifted to the ego, obstacles [G, num_obs, 5] = x, y
        (shifted), vx, vy, psi of the nearest obstacles, threshold that of
        custom_path_smoothing.  Returns (the list of 5-tuples ``compute_cem_batch``
        returns, the list of each tick's path dict); both equal the host
        helpers' route bit for bit."""
        kinds = {"mmd": "mmd_opt", "cvar": "cvar", "det": "det"}
        if cost not in kinds:
            raise ValueError("cost must be 'mmd', 'cvar' or 'det'")
        P = int(np.asarray(x_wp).shape[-1])
        if P not in self._ticks:   # one tick context per path length, made at its first use
            self._ticks[P] = native().Tick(self._h, P)
        tk = self._ticks[P]
        rs = tk.solve_batch(kinds[cost], idx_mpc, init_states, x_wp, y_wp, obstacles, threshold, means, cov, v_des)
        self.last_results = rs
        return ([(r["cx"], r["cy"], r["v_best"].copy(), r["steering"].copy(), r["mean_param"]) for r in rs],
                [tk.path(g) for g in range(len(rs))])

    def world_model(self, route, total_obs, goal_index=None, num_path=600, cov=None, dt=0.05, seed=0):
        """(the surrogate world's ``_native.WorldModel`` for this optimizer on
        ``route`` = (x, y) of the extended route, the tick context of
        ``num_path``): the splines are ``path_spline``'s, the noise model, lane
        bounds and ellipse the optimizer's own."""
        N = native()
        rx, ry = (np.ascontiguousarray(a, np.float64) for a in route)
        fit = getattr(self, "_route_fit", None)   # the last route's splines: a 21 k-point fit costs milliseconds
        if fit is None or not (np.array_equal(fit[0], rx) and np.array_equal(fit[1], ry)):
            fit = self._route_fit = (rx, ry, *self.cem_helper.path_spline(rx, ry))
        csx, csy, arc = fit[2], fit[3], fit[6]
        cov = np.diag([20.0] * 4 + [100.0] * 4).astype(np.float32) if cov is None else np.asarray(cov, np.float32)
        pop0 = np.random.default_rng([seed, 1]).standard_normal((self.num_batch, 8))
        pdot = N.host_constant(self._cfg, "Pdot").reshape(self.num, 11)   # plan_speed's basis
        model = N.WorldModel(rx, ry, arc, csx.c, csy.c, pdot[:4], cov, pop0, num_path, self.num_obs,
                             rx.size - 1 if goal_index is None else goal_index, self.y_lb, self.y_ub,
                             total_obs, noise=self.noise, dt=dt, sigma_acc=self.sigma_acc,
                             sigma_steer=self.sigma_steer, acc_const=self.acc_const_noise,
                             steer_const=self.steer_const_noise, steer_max=self.steer_max, a_obs=self.a_obs,
                             b_obs=self.b_obs, seed=self._cfg.seed)
        if num_path not in self._ticks:
            self._ticks[num_path] = N.Tick(self._h, num_path)
        return model, self._ticks[num_path]

    def run_episodes(self, cost, route, vehicles, starts, ticks, *, goal_index=None, num_path=600, mean=None, cov=None,
                     v_des=10.0, dt=0.05, threshold=0.1, u=None, key_base=0, key_stride=100000, seed=0,
                     device_step=True, chained=False, validate=None, routed=None):
        """E closed-loop episodes of ``ticks`` ticks on the surrogate world
        (DESIGN.md section 19): each tick all E episodes are ONE batched solve
        through the tick route (E <= max_configs), then one world step turns
        the plans into the next tick's raw inputs -- k_world_step on the GPU
        (``device_step``) or mpcmmd_world_step_host; the two give the same bits.
        There the step's arrays cross the host between solve and step.  With
        ``chained`` the whole loop is enqueued on the device (mpcmmd_world_run:
        begin, CEM and k_world_step per tick, nothing crossing the host, one
        readback of the log at the end) and gives the same bits again;
        ``chained`` may be a sequence of tick counts to split the run into.

        route (x, y) float64 of the extended route, goal_index its goal point
        (default: the last); vehicles [total_obs, 5] = x, y, vx, vy, psi;
        starts [E, 4] = x, y, v, psi.  Episode e has the key key_base +
        key_stride e: it solves tick k with idx_mpc = k + key and carries its
        own mean_param.  The perturbation's variates are drawn by the library
        from (key, the optimizer's seed, tick) after each tick's solve --
        normals, or for Beta noise Beta(2 |a_c|, 5 |a_c|) and Beta(2 |s_c|,
        5 |s_c|) of that tick's controls -- unless u [ticks, E, 4] is given.  Returns log_d [T, E, 3], log_f [T, E, 13], log_i [T, E, 4]
        (``_native.WORLD_LOG_*`` name the columns), done_tick, collided, goal
        [E] and, per tick, cx, cy [T, E, 11], steering [T, E, 4], mean_param
        [T, E, 8].

        ``validate`` = dict(rollouts=R, alpha=0.98, sigma=()) adds the
        Monte-Carlo risk of every tick's plan:
        ``validate_carla_risk`` of the tick, the plan the solve returned and R
        fresh noise rows under keys = idx_mpc, as val_counts (count, count_lane,
        count_rows), val_count_pos, val_var, val_cvar, val_mean, val_max
        [T, E, 3], val_mmd [T, E, 3, S] and val_est [T, E, 2] (the cost_lane and
        cost_obs the solve itself estimated).  On the chained route the stage
        runs inside the loop on the device (mpcmmd_world_validate); on the two
        host-linked routes each tick's obs and path are read back and the
        validator is called from the host -- the same bits, the slow way.

        ``routed`` = dict(s=, v=, d=, v0=, **scalars) replaces the constant-velocity
        vehicles by route-following traffic with car-following (DESIGN.md section
        24): s (float64 arc lengths on the route's splines), v (speeds), d (signed
        lateral offsets, left positive) and v0 (target speeds; <= 0: parked), each
        [total_obs] for every episode or [E, total_obs]; the scalars are
        ``_native.ROUTED_SCALARS``.  ``vehicles`` is then ignored (None will do):
        tick 0's rows come from (s, v, d).  The result gains veh [T, E, total_obs, 3]
        = s, v and the acceleration applied after each tick's step, the same bits
        on all three routes."""
        N = native()
        kinds = {"mmd": "mmd_opt", "cvar": "cvar", "det": "det"}
        if cost not in kinds:
            raise ValueError("cost must be 'mmd', 'cvar' or 'det'")
        val = None
        if validate is not None:
            extra = set(validate) - {"rollouts", "alpha", "sigma"}
            if extra or "rollouts" not in validate:
                raise ValueError("validate: dict(rollouts=R, alpha=..., sigma=...)")
            sg = validate.get("sigma", ())
            val = dict(rollouts=int(validate["rollouts"]), alpha=float(validate.get("alpha", 0.98)),
                       sigma=np.asarray(() if sg is None else sg, np.float32).reshape(-1))
        starts = np.asarray(starts, np.float64).reshape(-1, 4)
        E, T = starts.shape[0], int(ticks)
        if E > self.max_configs:
            raise ValueError(f"{E} episodes > max_configs {self.max_configs}")
        if T < 1:
            raise ValueError("ticks must be >= 1")
        if u is not None:
            u = np.asarray(u, np.float32).reshape(T, E, 4)
        keys = int(key_base) + int(key_stride) * np.arange(E)
        mean = np.array([v_des] * 4 + [0.0] * 4, np.float32) if mean is None else np.asarray(mean, np.float32)
        cov = np.diag([20.0] * 4 + [100.0] * 4).astype(np.float32) if cov is None else np.asarray(cov, np.float32)
        rt = None
        if routed is not None:
            if not {"s", "v", "d", "v0"} <= set(routed):
                raise ValueError("routed: dict(s=..., v=..., d=..., v0=..., **scalars)")
            V = np.asarray(routed["s"]).shape[-1] if np.ndim(routed["s"]) else 1
            per = lambda a, dt: np.ascontiguousarray(np.broadcast_to(np.asarray(a, dt).reshape(-1, V), (E, V)))
            rt = dict(s=per(routed["s"], np.float64), v=per(routed["v"], np.float32),
                      param=np.stack([per(routed["d"], np.float32), per(routed["v0"], np.float32)], -1),
                      **{k: x for k, x in routed.items() if k not in ("s", "v", "d", "v0")})
            N.routed_scalars({k: x for k, x in rt.items() if k not in ("s", "v", "param")})   # unknown names raise
            vehicles = np.zeros((V, 5), np.float32)
        vehicles = np.asarray(vehicles, np.float32).reshape(-1, 5)
        model, tk = self.world_model(route, vehicles.shape[0], goal_index, num_path, cov, dt, seed)
        if chained:
            world = N.World(tk, model, T)
            try:
                if val is not None:
                    world.validate(**val)
                if rt is not None:
                    world.route_vehicles(**rt)
                world.reset(starts[:, :2], np.stack([starts[:, 2], starts[:, 3], np.zeros(E)], 1),
                            np.tile(vehicles[None], (E, 1, 1)), np.tile(mean.reshape(1, 8), (E, 1)), cov, u, keys)
                k0 = 0
                for count in ([T] if chained is True else [int(c) for c in chained]):   # a run may be split
                    world.run(kinds[cost], k0, count, cov, v_des, threshold)
                    k0 += count
                if k0 != T:
                    raise ValueError("chained: the tick counts must add up to ticks")
                out = world.log(T)
                if rt is not None:
                    out["veh"] = world.vehicle_log(T)
                if val is not None:
                    out.update(world.validation_log(T))
            finally:
                world.close()
            done = np.where(out["done_tick"] >= 0, out["done_tick"], T - 1)
            at_end = out["log_i"][done, np.arange(E)]
            out["collided"], out["goal"] = at_end[:, 2].astype(bool), at_end[:, 3].astype(bool)
            return out
        dev = self._cfg.device if device_step else None
        st = dict(pos=starts[:, :2].copy(), ego=np.stack([starts[:, 2], starts[:, 3], np.zeros(E)], 1),
                  vehicles=np.tile(vehicles[None], (E, 1, 1)), done_tick=np.full(E, -1, np.int32))
        means = np.tile(mean.reshape(1, 8), (E, 1))
        # a frozen step leaves the state alone and writes the raw inputs of the state it is given: tick 0's
        zero = lambda n: np.zeros((E, n), np.float32)
        nxt = N.world_step(model, -1, zero(11), zero(11), zero(4), zero(4), means, st["pos"], st["ego"],
                           st["vehicles"], np.zeros(E, np.int32), device=dev, routed=rt)
        if rt is not None:   # the reset-mode step made tick 0's rows
            st["vehicles"] = nxt["vehicles"]
            out_veh = np.empty((T, E, vehicles.shape[0], 3))
        out = dict(log_d=np.empty((T, E, 3)), log_f=np.empty((T, E, 13), np.float32),
                   log_i=np.empty((T, E, 4), np.int32), cx=np.empty((T, E, 11), np.float32),
                   cy=np.empty((T, E, 11), np.float32), steering=np.empty((T, E, 4), np.float32),
                   mean_param=np.empty((T, E, 8), np.float32))
        if val is not None:
            H, O, S = self.num_prime, self.num_obs, val["sigma"].size
            out.update(val_counts=np.empty((T, E, 3), np.int32), val_count_pos=np.empty((T, E, 3), np.int32),
                       val_mmd=np.empty((T, E, 3, S), np.float32), val_est=np.empty((T, E, 2), np.float32))
            out.update({"val_" + key: np.empty((T, E, 3), np.float32) for key in ("var", "cvar", "mean", "max")})
        for k in range(T):
            idx = [k + int(key) for key in keys]
            rs = tk.solve_batch(kinds[cost], idx, nxt["init_state"], nxt["x_wp"], nxt["y_wp"], nxt["obstacles"],
                                threshold, means, cov, v_des)
            out["cx"][k] = [r["cx"] for r in rs]
            out["cy"][k] = [r["cy"] for r in rs]
            out["steering"][k] = [np.asarray(r["steering"])[:4] for r in rs]
            means = np.array([r["mean_param"] for r in rs], np.float32)
            out["mean_param"][k] = means
            if val is not None:   # the tick's plan against fresh noise rows, from what the solve left on the device
                obs = self._h.read("obs", shape=(E, 2, O, H))
                tracks = np.zeros((2, E, O, 100), np.float32)
                tracks[:, :, :, :H] = obs.transpose(1, 0, 2, 3)
                path = self._h.read("path").reshape(-1, 6, N.MAX_PATH)[:E, :, :num_path]
                c = self._cfg   # the handle's own (fp32) noise scalars
                r = N.validate_carla_risk(nxt["init_state"], [x["v_best"] for x in rs], [x["steering"] for x in rs],
                                          tracks[0], tracks[1], path, idx, H, self.noise, float(c.noise_level),
                                          float(c.acc_const_noise), float(c.steer_const_noise),
                                          num_rollouts=val["rollouts"], variant=self.variant, seed=c.seed,
                                          device=c.device, alpha=val["alpha"], sigma=val["sigma"] if S else None,
                                          counts=True)
                out["val_counts"][k] = np.stack([r["count"], r["count_lane"], r["count_rows"]], 1)
                out["val_count_pos"][k], out["val_mmd"][k] = r["count_pos"], r["mmd"]
                for key in ("var", "cvar", "mean", "max"):
                    out["val_" + key][k] = r[key]
                out["val_est"][k] = [[x["cost_lane"], x["cost_obs"]] for x in rs]
            nxt = N.world_step(model, k, out["cx"][k], out["cy"][k], out["steering"][k], None if u is None else u[k],
                               means, st["pos"], st["ego"], st["vehicles"], st["done_tick"], device=dev, keys=keys,
                               routed=rt)
            st = {key: nxt[key] for key in st}
            if rt is not None:
                rt.update(s=nxt["veh_s"], v=nxt["veh_v"])
                out_veh[k, :, :, 0], out_veh[k, :, :, 1:] = nxt["veh_s"], nxt["veh_log"]
            for key in ("log_d", "log_f", "log_i"):
                out[key][k] = nxt[key]
        if rt is not None:
            out["veh"] = out_veh
        out["done_tick"] = st["done_tick"]
        done = np.where(st["done_tick"] >= 0, st["done_tick"], T - 1)
        at_end = out["log_i"][done, np.arange(E)]
        out["collided"], out["goal"] = at_end[:, 2].astype(bool), at_end[:, 3].astype(bool)
        return out

    def close(self):
        """Free the tick contexts, then the handle."""
        for tk in self._ticks.values():
            tk.close()
        self._ticks = {}
        self._h.close()

    @property
    def handle(self):
        return self._h
