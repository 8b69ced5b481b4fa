"""ctypes binding of libmpcmmd.so (include/mpcmmd.h).

The library is built in-tree (``mpc-mmd_amd/libmpcmmd.so``, see
``__graft_entry__.build``).  There is no fallback: if the library is missing,
or no GPU is visible when a handle is created, the calls raise.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MPCMMD_LIB", os.path.join(os.path.dirname(_HERE), "libmpcmmd.so"))

COST = {"mmd_opt": 0, "mmd_random": 1, "cvar": 2, "saa": 3, "det": 4}  # det: CARLA handles (compute_cem_det)
NOISE = {"gaussian": 0, "beta": 1}
VARIANT = {"static": 0, "dynamic": 1, "carla_town05": 2, "carla_town10hd": 3}
RESULT_STRIDE_BETA_MAX = 32
ABI_VERSION = 5

SYMBOLS = (
    "mpcmmd_abi_version", "mpcmmd_last_error", "mpcmmd_device_count", "mpcmmd_create",
    "mpcmmd_destroy", "mpcmmd_set_stream", "mpcmmd_get_stream", "mpcmmd_solve", "mpcmmd_begin",
    "mpcmmd_iterate", "mpcmmd_finish", "mpcmmd_sync", "mpcmmd_profile", "mpcmmd_kernel_times",
    "mpcmmd_kernel_name", "mpcmmd_buffer_info", "mpcmmd_read", "mpcmmd_write", "mpcmmd_run_stage",
    "mpcmmd_host_constant", "mpcmmd_obs_dynamic_traj", "mpcmmd_validate", "mpcmmd_create_batch",
    "mpcmmd_max_configs", "mpcmmd_solve_batch", "mpcmmd_begin_batch", "mpcmmd_finish_batch",
    "mpcmmd_carla_begin", "mpcmmd_carla_solve", "mpcmmd_path_smoothing", "mpcmmd_path_parameters",
    "mpcmmd_global_to_frenet", "mpcmmd_set_graphs", "mpcmmd_handle_info", "mpcmmd_validate_carla",
    "mpcmmd_validate_risk", "mpcmmd_quantile_position", "mpcmmd_validate_carla_risk",
    "mpcmmd_carla_begin_batch", "mpcmmd_carla_solve_batch", "mpcmmd_tick_create", "mpcmmd_tick_destroy",
    "mpcmmd_carla_tick_begin_batch", "mpcmmd_carla_tick_solve_batch", "mpcmmd_carla_tick_host",
    "mpcmmd_world_step_host", "mpcmmd_world_step_device", "mpcmmd_world_create", "mpcmmd_world_destroy",
    "mpcmmd_world_reset", "mpcmmd_world_run", "mpcmmd_world_log", "mpcmmd_world_validate",
    "mpcmmd_world_validation_log", "mpcmmd_world_validation_inputs",
    "mpcmmd_mpc_step_host", "mpcmmd_mpc_step_device", "mpcmmd_mpc_create", "mpcmmd_mpc_destroy",
    "mpcmmd_mpc_reset", "mpcmmd_mpc_run", "mpcmmd_mpc_log", "mpcmmd_mpc_first_normals",
    "mpcmmd_mpc_validate", "mpcmmd_mpc_validation_log", "mpcmmd_mpc_validation_inputs",
    "mpcmmd_mpc_vehicle_constant", "mpcmmd_mpc_step_host_planned", "mpcmmd_mpc_step_device_planned",
    "mpcmmd_mpc_plan_vehicles", "mpcmmd_mpc_vehicle_log",
    "mpcmmd_mpc_queue_host", "mpcmmd_mpc_queue_device", "mpcmmd_mpc_queue_reset", "mpcmmd_mpc_queue_run",
    "mpcmmd_mpc_queue_status", "mpcmmd_mpc_queue_log",
    "mpcmmd_world_step_host_routed", "mpcmmd_world_step_device_routed", "mpcmmd_world_route_vehicles",
    "mpcmmd_world_vehicle_log",
)


class Config(C.Structure):
    _fields_ = [("num_reduced", C.c_int32), ("num_obs", C.c_int32), ("noise_level", C.c_float),
                ("num_prime", C.c_int32), ("noise", C.c_int32), ("acc_const_noise", C.c_float),
                ("steer_const_noise", C.c_float), ("num_batch", C.c_int32), ("variant", C.c_int32),
                ("maxiter_cem", C.c_int32), ("device", C.c_int32), ("seed", C.c_uint32)]


class Draws(C.Structure):
    _fields_ = [("pop0", C.POINTER(C.c_float)), ("roll", C.POINTER(C.c_float)),
                ("resample", C.POINTER(C.c_float)), ("beta_z0", C.POINTER(C.c_float)),
                ("beta_z", C.POINTER(C.c_float)), ("init_eps", C.POINTER(C.c_float))]


class Result(C.Structure):
    _fields_ = [("cx", C.c_float * 11), ("cy", C.c_float * 11), ("cost_lane", C.c_float),
                ("cost_obs", C.c_float), ("sigma", C.c_float), ("res_beta", C.c_float * 20),
                ("beta", C.POINTER(C.c_float)), ("elite_proj", C.POINTER(C.c_int32)),
                ("elite_obs", C.POINTER(C.c_int32)), ("elite_cem", C.POINTER(C.c_int32)),
                ("steering", C.POINTER(C.c_float)), ("v_best", C.POINTER(C.c_float)),
                ("mean_param", C.c_float * 8)]


class Path(C.Structure):
    _fields_ = [("num_path", C.c_int32), ("x_path", C.POINTER(C.c_float)), ("y_path", C.POINTER(C.c_float)),
                ("arc_vec", C.POINTER(C.c_float)), ("Fx_dot", C.POINTER(C.c_float)),
                ("Fy_dot", C.POINTER(C.c_float)), ("kappa", C.POINTER(C.c_float))]

PATH_KEYS = ("x_path", "y_path", "arc_vec", "Fx_dot", "Fy_dot", "kappa")
MAX_PATH = 2048   # kMaxPath: the stride of a path array in the handle's "path" buffer


class TickInputs(C.Structure):
    _fields_ = [("init_state", C.POINTER(C.c_float)), ("x_wp", C.POINTER(C.c_float)), ("y_wp", C.POINTER(C.c_float)),
                ("obstacles", C.POINTER(C.c_float)), ("threshold", C.c_float)]


class ValidateArgs(C.Structure):
    _fields_ = [("num_cfg", C.c_int32), ("num_obs", C.c_int32), ("num_prime", C.c_int32),
                ("num_rollouts", C.c_int32), ("noise", C.c_int32), ("variant", C.c_int32),
                ("noise_level", C.c_double), ("acc_const_noise", C.c_double), ("steer_const_noise", C.c_double),
                ("seed", C.c_uint32), ("device", C.c_int32),
                ("cx", C.POINTER(C.c_double)), ("cy", C.POINTER(C.c_double)),
                ("init_state", C.POINTER(C.c_double)), ("x_obs", C.POINTER(C.c_float)),
                ("y_obs", C.POINTER(C.c_float)), ("draws", C.POINTER(C.c_double)),
                ("keys", C.POINTER(C.c_uint32)), ("count", C.POINTER(C.c_int32)),
                ("count_lane", C.POINTER(C.c_int32))]


class ValidateCarlaArgs(C.Structure):
    _fields_ = [("num_cfg", C.c_int32), ("num_obs", C.c_int32), ("num_prime", C.c_int32),
                ("num_rollouts", C.c_int32), ("num_path", C.c_int32), ("noise", C.c_int32), ("variant", C.c_int32),
                ("noise_level", C.c_float), ("acc_const_noise", C.c_float), ("steer_const_noise", C.c_float),
                ("seed", C.c_uint32), ("device", C.c_int32),
                ("init_state", C.POINTER(C.c_float)), ("v", C.POINTER(C.c_float)), ("steer", C.POINTER(C.c_float)),
                ("x_obs", C.POINTER(C.c_float)), ("y_obs", C.POINTER(C.c_float)), ("path", C.POINTER(C.c_float)),
                ("draws", C.POINTER(C.c_float)), ("init_eps", C.POINTER(C.c_float)),
                ("keys", C.POINTER(C.c_uint32)), ("count", C.POINTER(C.c_int32)),
                ("count_lane", C.POINTER(C.c_int32)), ("count_rows", C.POINTER(C.c_int32)),
                ("count_oh", C.POINTER(C.c_int32)), ("elapsed_ms", C.POINTER(C.c_float))]


class ValidateRiskArgs(C.Structure):
    _fields_ = [("num_cfg", C.c_int32), ("num_obs", C.c_int32), ("num_prime", C.c_int32),
                ("num_rollouts", C.c_int32), ("noise", C.c_int32), ("variant", C.c_int32),
                ("noise_level", C.c_double), ("acc_const_noise", C.c_double), ("steer_const_noise", C.c_double),
                ("seed", C.c_uint32), ("device", C.c_int32),
                ("cx", C.POINTER(C.c_double)), ("cy", C.POINTER(C.c_double)),
                ("init_state", C.POINTER(C.c_double)), ("x_obs", C.POINTER(C.c_float)),
                ("y_obs", C.POINTER(C.c_float)), ("draws", C.POINTER(C.c_double)),
                ("keys", C.POINTER(C.c_uint32)), ("alpha", C.c_float), ("num_sigma", C.c_int32),
                ("sigma", C.POINTER(C.c_float)), ("costs_in", C.POINTER(C.c_float)),
                ("count_pos", C.POINTER(C.c_int32)), ("var", C.POINTER(C.c_float)), ("cvar", C.POINTER(C.c_float)),
                ("mean", C.POINTER(C.c_float)), ("max", C.POINTER(C.c_float)), ("mmd", C.POINTER(C.c_float)),
                ("costs", C.POINTER(C.c_float)), ("elapsed_ms", C.POINTER(C.c_float))]


class ValidateCarlaRiskArgs(C.Structure):
    _fields_ = ValidateCarlaArgs._fields_[:21] + [
        ("alpha", C.c_float), ("num_sigma", C.c_int32), ("sigma", C.POINTER(C.c_float)),
        ("count_pos", C.POINTER(C.c_int32)), ("var", C.POINTER(C.c_float)), ("cvar", C.POINTER(C.c_float)),
        ("mean", C.POINTER(C.c_float)), ("max", C.POINTER(C.c_float)), ("mmd", C.POINTER(C.c_float)),
        ("costs", C.POINTER(C.c_float)), ("count", C.POINTER(C.c_int32)), ("count_lane", C.POINTER(C.c_int32)),
        ("count_rows", C.POINTER(C.c_int32)), ("count_oh", C.POINTER(C.c_int32)),
        ("elapsed_ms", C.POINTER(C.c_float))]


class WorldModelStruct(C.Structure):
    _fields_ = ([(k, C.c_int32) for k in ("num_path", "num_obs", "total_obs", "num_route", "goal_index", "num_batch",
                                          "noise")] +
                [(k, C.c_float) for k in ("dt", "sigma_acc", "sigma_steer", "acc_const", "steer_const", "steer_max",
                                          "a_obs", "b_obs", "y_lb", "y_ub")] +
                [(k, C.POINTER(C.c_double)) for k in ("route_x", "route_y", "route_arc", "spline_x", "spline_y",
                                                      "pdot4", "chol")] +
                [("pop0", C.POINTER(C.c_float)), ("seed", C.c_uint32)])


class WorldStepIO(C.Structure):
    _fields_ = ([(k, C.POINTER(C.c_float)) for k in ("cx", "cy", "steer", "u", "mean")] +
                [("pos", C.POINTER(C.c_double)), ("ego", C.POINTER(C.c_float)), ("vehicles", C.POINTER(C.c_float)),
                 ("done_tick", C.POINTER(C.c_int32))] +
                [(k, C.POINTER(C.c_float)) for k in ("init_state", "x_wp", "y_wp", "obstacles", "pop")] +
                [("log_d", C.POINTER(C.c_double)), ("log_f", C.POINTER(C.c_float)), ("log_i", C.POINTER(C.c_int32)),
                 ("key", C.POINTER(C.c_uint32))])


ROUTED_SCALARS = ("acc_max", "brake", "gap0", "headway", "length", "lane_tol", "gap_min", "acc_min")
ROUTED_DEFAULTS = dict(acc_max=1.5, brake=2.0, gap0=5.0, headway=1.0, length=4.5, lane_tol=1.75, gap_min=0.5,
                       acc_min=-8.0)


class WorldRouted(C.Structure):
    _fields_ = ([("veh_s", C.POINTER(C.c_double)), ("veh_v", C.POINTER(C.c_float)),
                 ("veh_param", C.POINTER(C.c_float)), ("veh_log", C.POINTER(C.c_float))] +
                [(k, C.c_float) for k in ROUTED_SCALARS])


class WorldValidation(C.Structure):
    _fields_ = [("num_rollouts", C.c_int32), ("alpha", C.c_float), ("num_sigma", C.c_int32),
                ("sigma", C.c_float * 8)]


class MpcValidation(C.Structure):
    _fields_ = [("num_rollouts", C.c_int32), ("alpha", C.c_float), ("num_sigma", C.c_int32),
                ("sigma", C.c_float * 8), ("overlap", C.c_int32)]


class MpcModelStruct(C.Structure):
    _fields_ = ([(k, C.c_int32) for k in ("num_obs", "num_batch", "noise")] +
                [(k, C.c_float) for k in ("dt", "sigma_acc", "sigma_steer", "acc_const", "steer_const", "K_steer",
                                          "a_obs", "b_obs", "y_lb", "y_ub", "goal_x")] +
                [(k, C.POINTER(C.c_double)) for k in ("pdot2", "pddot1", "chol")] +
                [("pop0", C.POINTER(C.c_float)), ("seed", C.c_uint32)])


class MpcStepIO(C.Structure):
    _fields_ = ([(k, C.POINTER(C.c_float)) for k in ("cx", "cy", "u", "mean")] +
                [("pos", C.POINTER(C.c_double)), ("vel", C.POINTER(C.c_float)), ("vehicles", C.POINTER(C.c_float)),
                 ("done_tick", C.POINTER(C.c_int32))] +
                [(k, C.POINTER(C.c_float)) for k in ("init_state", "x_obs", "y_obs", "pop", "st0")] +
                [("log_d", C.POINTER(C.c_double)), ("log_f", C.POINTER(C.c_float)), ("log_i", C.POINTER(C.c_int32)),
                 ("key", C.POINTER(C.c_uint32))])


class MpcPlanned(C.Structure):
    _fields_ = [(k, C.POINTER(C.c_float)) for k in ("veh_acc", "veh_target", "veh_log")]


class MpcQueueIO(C.Structure):
    _fields_ = ([(k, C.c_int32) for k in ("n_slots", "n_scenes", "ticks_per_episode", "tick")] +
                [("flags", C.POINTER(C.c_int32)), ("keys", C.POINTER(C.c_int32)), ("v_des", C.POINTER(C.c_float))] +
                [(k, C.POINTER(C.c_int32)) for k in ("scene", "ltick", "done", "fresh")] +
                [("key", C.POINTER(C.c_uint32)), ("idx_mpc", C.POINTER(C.c_int32)),
                 ("slot_v_des", C.POINTER(C.c_float)), ("sched", C.POINTER(C.c_int32)),
                 ("count", C.POINTER(C.c_int32))])


class MpcScenes(C.Structure):
    _fields_ = ([("n_scenes", C.c_int32), ("pos", C.POINTER(C.c_double))] +
                [(k, C.POINTER(C.c_float)) for k in ("vel", "vehicles", "mean", "v_des")] +
                [("keys", C.POINTER(C.c_int32)), ("veh_target", C.POINTER(C.c_float)),
                 ("veh_acc", C.POINTER(C.c_float))])


QUEUE_REASONS = ("unfinished", "collision", "goal", "tick_limit")   # MPCMMD_QUEUE_*: sched[:, 3]
QUEUE_SCHED = ("slot", "first_tick", "ticks", "reason")

MPC_LOG_D = ("x", "y")
MPC_LOG_F = ("vx", "vy", "psi", "a_c", "s_c", "a", "s", "u0", "u1", "u2", "clear", "curv")
MPC_LOG_I = ("lane_out", "collided", "goal", "frozen")

WORLD_LOG_D = ("x", "y", "arc")
WORLD_LOG_F = ("v", "psi", "psidot", "a_c", "s_c", "a", "s", "u0", "u1", "u2", "u3", "clear", "d")
WORLD_LOG_I = ("idx", "lane_out", "collided", "goal")

assert ValidateCarlaRiskArgs._fields_[20][0] == "keys"   # the inputs of ValidateCarlaArgs, up to the keys

RISK_CHANNELS = ("obs", "lane_lb", "lane_ub")


class NativeError(RuntimeError):
    pass


_lib = None


def lib():
    """Load libmpcmmd.so once (raises if it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeError(f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'`"
                          " (or `make -C mpc-mmd_amd`)")
    L = C.CDLL(LIB_PATH)
    fp = C.POINTER(C.c_float)
    vp = C.c_void_p
    L.mpcmmd_abi_version.restype = C.c_int32
    L.mpcmmd_last_error.restype = C.c_char_p
    L.mpcmmd_device_count.restype = C.c_int32
    L.mpcmmd_create.argtypes = [C.POINTER(Config), C.POINTER(vp)]
    L.mpcmmd_create_batch.argtypes = [C.POINTER(Config), C.c_int32, C.POINTER(vp)]
    L.mpcmmd_max_configs.argtypes = [vp]
    L.mpcmmd_max_configs.restype = C.c_int32
    L.mpcmmd_handle_info.argtypes = [vp, C.c_char_p, C.POINTER(C.c_int64)]
    ip = C.POINTER(C.c_int32)
    bargs = [vp, C.c_int32, C.c_int32, ip, fp, fp, fp, fp, fp, fp]
    L.mpcmmd_solve_batch.argtypes = bargs + [C.POINTER(Result)]
    L.mpcmmd_begin_batch.argtypes = bargs
    L.mpcmmd_finish_batch.argtypes = [vp, C.c_int32, C.POINTER(Result)]
    L.mpcmmd_destroy.argtypes = [vp]
    L.mpcmmd_destroy.restype = None
    L.mpcmmd_set_stream.argtypes = [vp, vp]
    L.mpcmmd_get_stream.argtypes = [vp]
    L.mpcmmd_get_stream.restype = vp
    args = [vp, C.c_int32, C.c_int32, fp, fp, fp, fp, fp, C.c_float, C.POINTER(Draws)]
    L.mpcmmd_solve.argtypes = args + [C.POINTER(Result)]
    L.mpcmmd_begin.argtypes = args
    L.mpcmmd_iterate.argtypes = [vp, C.c_int32, C.c_int32]
    L.mpcmmd_finish.argtypes = [vp, C.POINTER(Result)]
    L.mpcmmd_sync.argtypes = [vp]
    L.mpcmmd_profile.argtypes = [vp, C.c_int32]
    L.mpcmmd_kernel_times.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.c_int32]
    L.mpcmmd_kernel_name.argtypes = [C.c_int32]
    L.mpcmmd_kernel_name.restype = C.c_char_p
    L.mpcmmd_buffer_info.argtypes = [vp, C.c_char_p, C.POINTER(C.c_size_t)]
    L.mpcmmd_read.argtypes = [vp, C.c_char_p, vp, C.c_size_t]
    L.mpcmmd_write.argtypes = [vp, C.c_char_p, vp, C.c_size_t]
    L.mpcmmd_run_stage.argtypes = [vp, C.c_int32, C.c_int32]
    L.mpcmmd_host_constant.argtypes = [C.POINTER(Config), C.c_char_p, C.POINTER(C.c_double), C.c_size_t]
    L.mpcmmd_validate.argtypes = [C.POINTER(ValidateArgs)]
    L.mpcmmd_validate_carla.argtypes = [C.POINTER(ValidateCarlaArgs)]
    L.mpcmmd_validate_risk.argtypes = [C.POINTER(ValidateRiskArgs)]
    if hasattr(L, "mpcmmd_validate_carla_risk"):   # an older library lacks it: validate_carla_risk raises
        L.mpcmmd_validate_carla_risk.argtypes = [C.POINTER(ValidateCarlaRiskArgs)]
    L.mpcmmd_quantile_position.argtypes = [C.c_int32, C.c_float, ip, ip, fp, fp]
    L.mpcmmd_obs_dynamic_traj.argtypes = [C.c_int32, fp, fp, fp, fp, fp, C.c_float, fp, fp]
    cargs = [vp, C.c_int32, C.c_int32, fp, fp, fp, fp, fp, C.c_float, C.POINTER(Path), C.POINTER(Draws)]
    L.mpcmmd_set_graphs.argtypes = [vp, C.c_int32]
    L.mpcmmd_carla_begin.argtypes = cargs
    L.mpcmmd_carla_solve.argtypes = cargs + [C.POINTER(Result)]
    if hasattr(L, "mpcmmd_carla_begin_batch"):   # an older library lacks them: carla_begin_batch raises
        L.mpcmmd_carla_begin_batch.argtypes = bargs + [C.POINTER(Path)]
        L.mpcmmd_carla_solve_batch.argtypes = bargs + [C.POINTER(Path), C.POINTER(Result)]
    if hasattr(L, "mpcmmd_tick_create"):   # an older library lacks the tick route: Tick raises
        targs = [vp, C.c_int32, C.c_int32, ip, C.POINTER(TickInputs), fp, fp, fp]
        L.mpcmmd_tick_create.argtypes = [vp, C.c_int32, C.POINTER(vp)]
        L.mpcmmd_tick_destroy.argtypes = [vp]
        L.mpcmmd_tick_destroy.restype = None
        L.mpcmmd_carla_tick_begin_batch.argtypes = targs
        L.mpcmmd_carla_tick_solve_batch.argtypes = targs + [C.POINTER(Result)]
        L.mpcmmd_carla_tick_host.argtypes = [C.c_int32, C.c_int32, fp, fp, fp, fp, C.c_float, fp, fp, fp]
    if hasattr(L, "mpcmmd_world_step_host"):   # an older library lacks the world: world_step raises
        L.mpcmmd_world_step_host.argtypes = [C.POINTER(WorldModelStruct), C.c_int32, C.POINTER(WorldStepIO)]
        L.mpcmmd_world_step_device.argtypes = [C.POINTER(WorldModelStruct), C.c_int32, C.c_int32, C.c_int32,
                                               C.POINTER(WorldStepIO)]
        dp = C.POINTER(C.c_double)
        L.mpcmmd_world_create.argtypes = [vp, C.POINTER(WorldModelStruct), C.c_int32, C.POINTER(vp)]
        L.mpcmmd_world_destroy.argtypes = [vp]
        L.mpcmmd_world_destroy.restype = None
        L.mpcmmd_world_reset.argtypes = [vp, C.c_int32, dp, fp, fp, fp, fp, fp, ip]
        L.mpcmmd_world_run.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, fp, fp, C.c_float]
        L.mpcmmd_world_log.argtypes = [vp, C.c_int32, dp, fp, ip, fp, ip]
    if hasattr(L, "mpcmmd_world_route_vehicles"):   # an older library lacks the routed vehicles: the callers raise
        dp = C.POINTER(C.c_double)
        L.mpcmmd_world_step_host_routed.argtypes = [C.POINTER(WorldModelStruct), C.c_int32, C.POINTER(WorldStepIO),
                                                    C.POINTER(WorldRouted)]
        L.mpcmmd_world_step_device_routed.argtypes = [C.POINTER(WorldModelStruct), C.c_int32, C.c_int32, C.c_int32,
                                                      C.POINTER(WorldStepIO), C.POINTER(WorldRouted)]
        L.mpcmmd_world_route_vehicles.argtypes = [vp, C.c_int32, dp, fp, fp, fp]
        L.mpcmmd_world_vehicle_log.argtypes = [vp, C.c_int32, dp, fp]
    if hasattr(L, "mpcmmd_world_validate"):   # an older library lacks the stage: World.validate raises
        L.mpcmmd_world_validate.argtypes = [vp, C.POINTER(WorldValidation)]
        L.mpcmmd_world_validation_log.argtypes = [vp, C.c_int32, ip, ip, fp, fp, fp]
        L.mpcmmd_world_validation_inputs.argtypes = [vp, fp, fp, fp, fp, fp, fp, C.POINTER(C.c_uint32)]
    if hasattr(L, "mpcmmd_mpc_step_host"):   # an older library lacks the synthetic loop: mpc_step raises
        dp = C.POINTER(C.c_double)
        L.mpcmmd_mpc_step_host.argtypes = [C.POINTER(MpcModelStruct), C.c_int32, C.POINTER(MpcStepIO)]
        L.mpcmmd_mpc_step_device.argtypes = [C.POINTER(MpcModelStruct), C.c_int32, C.c_int32, C.c_int32,
                                             C.POINTER(MpcStepIO)]
        L.mpcmmd_mpc_create.argtypes = [vp, C.POINTER(MpcModelStruct), C.c_int32, C.POINTER(vp)]
        L.mpcmmd_mpc_destroy.argtypes = [vp]
        L.mpcmmd_mpc_destroy.restype = None
        L.mpcmmd_mpc_reset.argtypes = [vp, C.c_int32, dp, fp, fp, fp, fp, fp, ip]
        L.mpcmmd_mpc_run.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, fp, fp]
        L.mpcmmd_mpc_log.argtypes = [vp, C.c_int32, dp, fp, ip, fp, ip]
        L.mpcmmd_mpc_first_normals.argtypes = [C.POINTER(Config), fp]
    if hasattr(L, "mpcmmd_mpc_validate"):   # an older library lacks the stage: Mpc.validate raises
        dp = C.POINTER(C.c_double)
        L.mpcmmd_mpc_validate.argtypes = [vp, C.POINTER(MpcValidation)]
        L.mpcmmd_mpc_validation_log.argtypes = [vp, C.c_int32, ip, ip, fp, fp, fp]
        L.mpcmmd_mpc_validation_inputs.argtypes = [vp, dp, dp, dp, fp, fp, C.POINTER(C.c_uint32)]
    if hasattr(L, "mpcmmd_mpc_plan_vehicles"):   # an older library lacks the planned vehicles: the callers raise
        L.mpcmmd_mpc_vehicle_constant.argtypes = [C.c_float, C.c_char_p, C.POINTER(C.c_double), C.c_size_t]
        L.mpcmmd_mpc_step_host_planned.argtypes = [C.POINTER(MpcModelStruct), C.c_int32, C.POINTER(MpcStepIO),
                                                   C.POINTER(MpcPlanned)]
        L.mpcmmd_mpc_step_device_planned.argtypes = [C.POINTER(MpcModelStruct), C.c_int32, C.c_int32, C.c_int32,
                                                     C.POINTER(MpcStepIO), C.POINTER(MpcPlanned)]
        L.mpcmmd_mpc_plan_vehicles.argtypes = [vp, C.c_int32, fp, fp]
        L.mpcmmd_mpc_vehicle_log.argtypes = [vp, C.c_int32, fp]
    if hasattr(L, "mpcmmd_mpc_queue_reset"):   # an older library lacks the scene queue: the callers raise
        L.mpcmmd_mpc_queue_host.argtypes = [C.POINTER(MpcQueueIO)]
        L.mpcmmd_mpc_queue_device.argtypes = [C.c_int32, C.POINTER(MpcQueueIO)]
        L.mpcmmd_mpc_queue_reset.argtypes = [vp, C.c_int32, C.c_int32, C.POINTER(MpcScenes), fp]
        L.mpcmmd_mpc_queue_run.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, fp]
        L.mpcmmd_mpc_queue_status.argtypes = [vp, ip, ip]
        L.mpcmmd_mpc_queue_log.argtypes = [vp, ip]
    L.mpcmmd_path_smoothing.argtypes = [C.c_int32, fp, fp, C.c_float, fp, fp]
    L.mpcmmd_path_parameters.argtypes = [C.c_int32, fp, fp, fp, fp, fp, fp, fp, fp, fp]
    L.mpcmmd_global_to_frenet.argtypes = [C.POINTER(Path), C.c_int32, fp, fp, fp, fp, fp, fp, fp]
    if L.mpcmmd_abi_version() != ABI_VERSION:
        raise NativeError("libmpcmmd ABI version mismatch")
    _lib = L
    return L


def check(rc):
    if rc < 0:
        raise NativeError(f"libmpcmmd error {rc}: {lib().mpcmmd_last_error().decode()}")
    return rc


def make_config(num_reduced, num_obs, noise_level, num_prime, noise, acc_const_noise, steer_const_noise,
                num_batch=100, variant="static", maxiter_cem=20, device=0, seed=0):
    return Config(int(num_reduced), int(num_obs), float(noise_level), int(num_prime), NOISE[noise],
                  float(acc_const_noise), float(steer_const_noise), int(num_batch), VARIANT[variant],
                  int(maxiter_cem), int(device), int(seed) & 0xFFFFFFFF)


def host_constant(cfg, name):
    L = lib()
    n = check(L.mpcmmd_host_constant(C.byref(cfg), name.encode(), None, 0))
    out = np.empty(n, np.float64)
    check(L.mpcmmd_host_constant(C.byref(cfg), name.encode(), out.ctypes.data_as(C.POINTER(C.c_double)), n))
    return out


def obs_dynamic_traj(x0, y0, vx0, vy0, v_des, y_des=-1.75):
    """mpcmmd_obs_dynamic_traj: per-obstacle QP trajectories [O][100] x 2
    (obs_data.compute_obs_guess, obs_data_generate_dynamic.py:73-109)."""
    a = [np.ascontiguousarray(np.asarray(v, np.float32).reshape(-1)) for v in (x0, y0, vx0, vy0, v_des)]
    O = a[0].size
    if any(v.size != O for v in a):
        raise ValueError("obstacle arrays differ in length")
    xt = np.empty((O, 100), np.float32)
    yt = np.empty((O, 100), np.float32)
    check(lib().mpcmmd_obs_dynamic_traj(O, *[_fptr(v) for v in a], float(y_des), _fptr(xt), _fptr(yt)))
    return xt, yt


def validate(cx, cy, init_state, x_obs, y_obs, keys, num_prime, noise, noise_level, acc_const_noise=0.0,
             steer_const_noise=0.0, num_rollouts=1000, variant="static", draws=None, seed=0, device=0):
    """mpcmmd_validate over K configurations: (count [K], count_lane [K])
    (S/validation.py compute_stats :134-171).  cx, cy [K,11]; init_state
    [K,6]; x_obs, y_obs [K,O,100] obstacle tracks; keys [K]; draws
    [K,3,R,H] fp64 or None (internal Philox)."""
    d = lambda a, *shape: np.ascontiguousarray(np.asarray(a, np.float64).reshape(*shape))
    cx = np.atleast_2d(np.asarray(cx, np.float64))
    K = cx.shape[0]
    cx, cy = d(cx, K, 11), d(cy, K, 11)
    st = d(init_state, K, 6)
    xo = np.ascontiguousarray(np.asarray(x_obs, np.float32).reshape(K, -1, 100))
    yo = np.ascontiguousarray(np.asarray(y_obs, np.float32).reshape(K, -1, 100))
    O = xo.shape[1]
    ks = np.ascontiguousarray(np.asarray(keys, np.int64).reshape(K).astype(np.uint32))
    dr = None if draws is None else d(draws, K, 3, num_rollouts, num_prime)
    cnt = np.zeros(K, np.int32)
    cl = np.zeros(K, np.int32)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    args = ValidateArgs(K, O, int(num_prime), int(num_rollouts), NOISE[noise], VARIANT[variant], float(noise_level),
                        float(acc_const_noise), float(steer_const_noise), int(seed) & 0xFFFFFFFF, int(device),
                        dp(cx), dp(cy), dp(st), _fptr(xo), _fptr(yo), None if dr is None else dp(dr),
                        ks.ctypes.data_as(C.POINTER(C.c_uint32)), cnt.ctypes.data_as(C.POINTER(C.c_int32)),
                        cl.ctypes.data_as(C.POINTER(C.c_int32)))
    check(lib().mpcmmd_validate(C.byref(args)))
    return cnt, cl


def validate_carla(init_state, v, steer, x_obs, y_obs, paths, keys, num_prime, noise, noise_level,
                   acc_const_noise=0.0, steer_const_noise=0.0, num_rollouts=1000, variant="carla_town05", draws=None,
                   init_eps=None, seed=0, device=0, count_oh=False, timing=False):
    """mpcmmd_validate_carla over K simulator ticks, one returned plan each:
    the optimizer's cvar risk model with ``num_rollouts`` fresh noise rows,
    reduced to counts (include/mpcmmd.h).  init_state [K,6]
    (init_state_global); v, steer [K,100] (v_best, steering_best); x_obs, y_obs
    [K,O,100] Frenet tracks; paths: K path dicts (PATH_KEYS) of one length, or
    an array [K,6,P]; keys [K]; draws [K,3,R,H], init_eps [K,R,4] fp32 or None
    (internal Philox streams).  Returns a dict: count, count_lane, count_rows
    [K] int32, with ``count_oh`` also count_oh [K,O,H], with ``timing`` also
    elapsed_ms (HIP events around the device work)."""
    H, R = int(num_prime), int(num_rollouts)
    K, O, P, (st, vv, ss, xo, yo, pa, dr, ie, ks) = _carla_plan_arrays(init_state, v, steer, x_obs, y_obs, paths,
                                                                     keys, H, R, draws, init_eps)
    out = {k: np.zeros(K, np.int32) for k in ("count", "count_lane", "count_rows")}
    oh = np.zeros((K, O, H), np.int32) if count_oh else None
    ms = C.c_float(0.0)
    ip = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))
    args = ValidateCarlaArgs(K, O, H, R, P, NOISE[noise], VARIANT[variant], float(noise_level),
                             float(acc_const_noise), float(steer_const_noise), int(seed) & 0xFFFFFFFF, int(device),
                             _fptr(st), _fptr(vv), _fptr(ss), _fptr(xo), _fptr(yo), _fptr(pa), _fptr(dr), _fptr(ie),
                             ks.ctypes.data_as(C.POINTER(C.c_uint32)), ip(out["count"]), ip(out["count_lane"]),
                             ip(out["count_rows"]), ip(oh), C.pointer(ms) if timing else None)
    check(lib().mpcmmd_validate_carla(C.byref(args)))
    if count_oh:
        out["count_oh"] = oh
    if timing:
        out["elapsed_ms"] = float(ms.value)
    return out


def _carla_plan_arrays(init_state, v, steer, x_obs, y_obs, paths, keys, H, R, draws, init_eps):
    """The input arrays of validate_carla / validate_carla_risk: (K, O, P, arrays in the struct's order)."""
    f = lambda a, *shape: np.ascontiguousarray(np.asarray(a, np.float32).reshape(*shape))
    K = int(np.asarray(keys).reshape(-1).shape[0])
    if K == 0:
        pa = np.zeros((0, 6, 4), np.float32)
    elif isinstance(paths, np.ndarray):
        pa = f(paths, K, 6, -1)
    else:
        if len(paths) != K:
            raise ValueError("one path per tick")
        if len({np.asarray(p[k]).size for p in paths for k in PATH_KEYS}) > 1:
            raise ValueError("path arrays differ in length (one num_path per call)")
        pa = f([[np.asarray(p[k], np.float32).reshape(-1) for k in PATH_KEYS] for p in paths], K, 6, -1)
    st, vv, ss = f(init_state, K, 6), f(v, K, 100), f(steer, K, 100)
    if K:
        xo, yo = f(x_obs, K, -1, 100), f(y_obs, K, -1, 100)
    else:  # nothing to run: the library returns before it looks at the arrays
        xo = yo = np.zeros((0, 1, 100), np.float32)
    ks = np.ascontiguousarray(np.asarray(keys, np.int64).reshape(K).astype(np.uint32))
    dr = None if draws is None else f(draws, K, 3, R, H)
    ie = None if init_eps is None else f(init_eps, K, R, 4)
    return K, xo.shape[1], pa.shape[2], (st, vv, ss, xo, yo, pa, dr, ie, ks)


def validate_carla_risk(init_state, v, steer, x_obs, y_obs, paths, keys, num_prime, noise, noise_level,
                        acc_const_noise=0.0, steer_const_noise=0.0, num_rollouts=1000, variant="carla_town05",
                        draws=None, init_eps=None, seed=0, device=0, alpha=0.98, sigma=None, return_costs=False,
                        counts=False, timing=False):
    """mpcmmd_validate_carla_risk over K simulator ticks (include/mpcmmd.h): the
    inputs of ``validate_carla``, whose rollouts it repeats point for point;
    ``sigma`` [K,S] (or [S], shared) the MMD bandwidths.  Returns the dict of
    ``validate_risk``: count_pos (int32), var, cvar, mean, max, saa [K,3]
    (channels RISK_CHANNELS), mmd [K,3,S], cvar_lane [K], mmd_lane [K,S]; with
    ``return_costs`` costs [K,3,R]; with ``counts`` also count, count_lane,
    count_rows [K] and count_oh [K,O,H] of ``validate_carla``; with ``timing``
    elapsed_ms [3] (rollouts with costs, statistics, MMD)."""
    L = lib()
    if not hasattr(L, "mpcmmd_validate_carla_risk"):
        raise NativeError(f"{LIB_PATH} has no mpcmmd_validate_carla_risk (built before the entry point existed): "
                          "rebuild it")
    H, R = int(num_prime), int(num_rollouts)
    K, O, P, arr = _carla_plan_arrays(init_state, v, steer, x_obs, y_obs, paths, keys, H, R, draws, init_eps)
    if sigma is None:
        sg = np.zeros((K, 0), np.float32)
    else:
        sg = np.asarray(sigma, np.float32)
        sg = np.ascontiguousarray(np.broadcast_to(sg, (K, sg.shape[-1])) if sg.ndim == 1 else sg.reshape(K, -1))
    S = sg.shape[1]
    out = dict(count_pos=np.zeros((K, 3), np.int32))
    out.update({k: np.zeros((K, 3), np.float32) for k in ("var", "cvar", "mean", "max")})
    out["mmd"] = np.zeros((K, 3, S), np.float32)
    costs = np.zeros((K, 3, R), np.float32) if return_costs else None
    cnt = {k: np.zeros(K, np.int32) for k in ("count", "count_lane", "count_rows")} if counts else {}
    if counts:
        cnt["count_oh"] = np.zeros((K, O, H), np.int32)
    ms = (C.c_float * 3)()
    ip = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))
    args = ValidateCarlaRiskArgs(K, O, H, R, P, NOISE[noise], VARIANT[variant], float(noise_level),
                                 float(acc_const_noise), float(steer_const_noise), int(seed) & 0xFFFFFFFF,
                                 int(device), *[_fptr(a) for a in arr[:8]],
                                 arr[8].ctypes.data_as(C.POINTER(C.c_uint32)), float(alpha), S,
                                 _fptr(sg) if S else None, ip(out["count_pos"]), _fptr(out["var"]),
                                 _fptr(out["cvar"]), _fptr(out["mean"]), _fptr(out["max"]),
                                 _fptr(out["mmd"]) if S else None, _fptr(costs), ip(cnt.get("count")),
                                 ip(cnt.get("count_lane")), ip(cnt.get("count_rows")), ip(cnt.get("count_oh")),
                                 C.cast(ms, C.POINTER(C.c_float)) if timing else None)
    check(L.mpcmmd_validate_carla_risk(C.byref(args)))
    out["saa"] = (out["count_pos"].astype(np.float32) / np.float32(R)).astype(np.float32)
    out["cvar_lane"] = (out["cvar"][:, 1] + out["cvar"][:, 2]).astype(np.float32)
    out["mmd_lane"] = (out["mmd"][:, 1] + out["mmd"][:, 2]).astype(np.float32)
    out.update(cnt)
    if return_costs:
        out["costs"] = costs
    if timing:
        out["elapsed_ms"] = np.array(list(ms), np.float32)
    return out


def quantile_position(n, alpha):
    """mpcmmd_quantile_position: (lo, hi, w_lo, w_hi) of the linear quantile of n
    ascending samples with fp32 weights (jnp.quantile).  No GPU needed."""
    lo, hi, wl, wh = C.c_int32(), C.c_int32(), C.c_float(), C.c_float()
    check(lib().mpcmmd_quantile_position(int(n), float(alpha), C.byref(lo), C.byref(hi), C.byref(wl), C.byref(wh)))
    return lo.value, hi.value, np.float32(wl.value), np.float32(wh.value)


def validate_risk(cx=None, cy=None, init_state=None, x_obs=None, y_obs=None, keys=None, num_prime=30,
                  noise="gaussian", noise_level=0.1, acc_const_noise=0.0, steer_const_noise=0.0, num_rollouts=1000,
                  variant="static", draws=None, seed=0, device=0, alpha=0.98, sigma=None, costs_in=None,
                  return_costs=False, timing=False):
    """mpcmmd_validate_risk over K configurations (include/mpcmmd.h): the plan
    inputs of ``validate``; ``sigma`` [K,S] (or [S], shared) the MMD bandwidths;
    ``costs_in`` [K,3,R] fp32 replaces the rollouts (the plan inputs may then be
    None).  Returns a dict of count_pos (int32), var, cvar, mean, max, saa
    [K,3] (channels RISK_CHANNELS), mmd [K,3,S], and the reference's lane sums
    cvar_lane [K], mmd_lane [K,S]; with ``return_costs`` costs [K,3,R], with
    ``timing`` elapsed_ms [3] (rollout, statistics, MMD stages)."""
    d = lambda a, *shape: np.ascontiguousarray(np.asarray(a, np.float64).reshape(*shape))
    f = lambda a, *shape: np.ascontiguousarray(np.asarray(a, np.float32).reshape(*shape))
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    H = int(num_prime)
    cin = ks = dr = None
    if costs_in is not None:
        cin = np.ascontiguousarray(np.asarray(costs_in, np.float32))
        if cin.ndim != 3 or cin.shape[1] != 3:
            raise ValueError("costs_in must be [K, 3, R]")
        K, _, R = cin.shape
        O = 1
        cx = cy = st = xo = yo = None
    else:
        R = int(num_rollouts)
        cx = np.atleast_2d(np.asarray(cx, np.float64))
        K = cx.shape[0]
        cx, cy, st = d(cx, K, 11), d(cy, K, 11), d(init_state, K, 6)
        xo = f(x_obs, K, -1, 100) if K else np.zeros((0, 1, 100), np.float32)
        yo = f(y_obs, K, -1, 100) if K else np.zeros((0, 1, 100), np.float32)
        O = xo.shape[1]
        ks = np.ascontiguousarray(np.asarray(keys, np.int64).reshape(K).astype(np.uint32))
        dr = None if draws is None else d(draws, K, 3, R, H)
    if sigma is None:
        sg = np.zeros((K, 0), np.float32)
    else:
        sg = np.asarray(sigma, np.float32)
        sg = np.ascontiguousarray(np.broadcast_to(sg, (K, sg.shape[-1])) if sg.ndim == 1 else sg.reshape(K, -1))
    S = sg.shape[1]
    out = dict(count_pos=np.zeros((K, 3), np.int32))
    out.update({k: np.zeros((K, 3), np.float32) for k in ("var", "cvar", "mean", "max")})
    out["mmd"] = np.zeros((K, 3, S), np.float32)
    costs = np.zeros((K, 3, R), np.float32) if return_costs else None
    ms = (C.c_float * 3)()
    args = ValidateRiskArgs(K, O, H, R, NOISE[noise], VARIANT[variant], float(noise_level), float(acc_const_noise),
                            float(steer_const_noise), int(seed) & 0xFFFFFFFF, int(device), dp(cx), dp(cy), dp(st),
                            _fptr(xo), _fptr(yo), dp(dr),
                            None if ks is None else ks.ctypes.data_as(C.POINTER(C.c_uint32)), float(alpha), S,
                            _fptr(sg) if S else None, _fptr(cin), ip(out["count_pos"]), _fptr(out["var"]),
                            _fptr(out["cvar"]), _fptr(out["mean"]), _fptr(out["max"]),
                            _fptr(out["mmd"]) if S else None, _fptr(costs),
                            C.cast(ms, C.POINTER(C.c_float)) if timing else None)
    check(lib().mpcmmd_validate_risk(C.byref(args)))
    out["saa"] = (out["count_pos"].astype(np.float32) / np.float32(R)).astype(np.float32)
    out["cvar_lane"] = (out["cvar"][:, 1] + out["cvar"][:, 2]).astype(np.float32)
    out["mmd_lane"] = (out["mmd"][:, 1] + out["mmd"][:, 2]).astype(np.float32)
    if return_costs:
        out["costs"] = costs
    if timing:
        out["elapsed_ms"] = np.array(list(ms), np.float32)
    return out


def _fptr(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))


def make_path(path):
    """mpcmmd_path from a dict of the six arrays (PATH_KEYS); returns
    (Path, keep) - keep holds the contiguous fp32 copies alive."""
    keep = {k: np.ascontiguousarray(np.asarray(path[k], np.float32).reshape(-1)) for k in PATH_KEYS}
    P = keep["x_path"].size
    if any(v.size != P for v in keep.values()):
        raise ValueError("path arrays differ in length")
    return Path(P, *(_fptr(keep[k]) for k in PATH_KEYS)), keep


def path_smoothing(x_wp, y_wp, threshold):
    """mpcmmd_path_smoothing (Helper.custom_path_smoothing, carla/optimizer/cem_helper.py:391-410)."""
    xw = np.ascontiguousarray(np.asarray(x_wp, np.float32).reshape(-1))
    yw = np.ascontiguousarray(np.asarray(y_wp, np.float32).reshape(-1))
    xo = np.empty_like(xw)
    yo = np.empty_like(yw)
    check(lib().mpcmmd_path_smoothing(xw.size, _fptr(xw), _fptr(yw), float(threshold), _fptr(xo), _fptr(yo)))
    return xo, yo


def path_parameters(x_path, y_path):
    """mpcmmd_path_parameters (Helper.compute_path_parameters, cem_helper.py:321-345):
    Fx_dot, Fy_dot, Fx_ddot, Fy_ddot, arc_vec, kappa, arc_length."""
    x = np.ascontiguousarray(np.asarray(x_path, np.float32).reshape(-1))
    y = np.ascontiguousarray(np.asarray(y_path, np.float32).reshape(-1))
    outs = [np.empty_like(x) for _ in range(6)]
    al = C.c_float()
    check(lib().mpcmmd_path_parameters(x.size, _fptr(x), _fptr(y), *[_fptr(o) for o in outs], C.byref(al)))
    return (*outs, np.float32(al.value))


def global_to_frenet(path, x, y, v, vdot, psi, psidot):
    """mpcmmd_global_to_frenet (Helper.global_to_frenet, cem_helper.py:348-388) of
    arrays of states: (x, y, vx, vy, ax, ay, psi) in the Frenet frame."""
    a = [np.ascontiguousarray(np.asarray(u, np.float32).reshape(-1)) for u in (x, y, v, vdot, psi, psidot)]
    n = a[0].size
    a = [np.ascontiguousarray(np.broadcast_to(u, (n,))) for u in a]
    out = np.empty((n, 7), np.float32)
    pth, keep = make_path(path)
    check(lib().mpcmmd_global_to_frenet(C.byref(pth), n, *[_fptr(u) for u in a], _fptr(out)))
    return tuple(out[:, k] for k in range(7))


def carla_tick_host(init_state, x_wp, y_wp, obstacles, threshold=0.1):
    """mpcmmd_carla_tick_host: the preprocessing of one simulator tick on the
    host in one call (custom_path_smoothing, compute_path_parameters,
    global_to_frenet_obs_vmap, compute_obs_trajectories).  x_wp, y_wp [P] the
    waypoints shifted to the ego; obstacles [O, 5] = x, y (shifted), vx, vy,
    psi.  Returns (path dict of PATH_KEYS, x_obs [O, 100], y_obs [O, 100])."""
    L = lib()
    if not hasattr(L, "mpcmmd_carla_tick_host"):
        raise NativeError(f"{LIB_PATH} has no mpcmmd_carla_tick_host (built before the entry point existed): rebuild it")
    f = lambda a: np.ascontiguousarray(np.asarray(a, np.float32))
    st, xw, yw = f(init_state).reshape(6), f(x_wp).reshape(-1), f(y_wp).reshape(-1)
    ob = f(obstacles).reshape(-1, 5)
    P, O = xw.size, ob.shape[0]
    if yw.size != P:
        raise ValueError("x_wp and y_wp differ in length")
    p6 = np.empty((6, P), np.float32)
    xo = np.empty((O, 100), np.float32)
    yo = np.empty((O, 100), np.float32)
    check(L.mpcmmd_carla_tick_host(P, O, _fptr(st), _fptr(xw), _fptr(yw), _fptr(ob), float(threshold), _fptr(p6),
                                   _fptr(xo), _fptr(yo)))
    return dict(zip(PATH_KEYS, p6)), xo, yo


class WorldModel:
    """mpcmmd_world_model: the constants of a surrogate world (DESIGN.md section
    19).  route_x / route_y / route_arc [R] float64 (the extended route and its
    splines' breakpoints), spline_x / spline_y the ``.c`` [4, R - 1] of scipy's
    ``CubicSpline(route_arc, route_x)``, pdot4 rows 0..3 of Pdot
    (``host_constant(cfg, "Pdot")``), cov the run's [8, 8] covariance (factored
    here as ``initial_population`` factors it), pop0 [B, 8] standard normals."""

    def __init__(self, route_x, route_y, route_arc, spline_x, spline_y, pdot4, cov, pop0, num_path, num_obs,
                 goal_index, y_lb, y_ub, total_obs, noise="gaussian", dt=0.05, sigma_acc=0.0, sigma_steer=0.0,
                 acc_const=0.0, steer_const=0.0, steer_max=0.6, a_obs=4.5, b_obs=3.0, seed=0):
        d = lambda a, *sh: np.ascontiguousarray(np.asarray(a, np.float64).reshape(*sh))
        R = np.asarray(route_x).size
        self.arrays = dict(route_x=d(route_x, R), route_y=d(route_y, R), route_arc=d(route_arc, R),
                           spline_x=d(spline_x, 4, R - 1), spline_y=d(spline_y, 4, R - 1),
                           pdot4=d(np.asarray(pdot4, np.float64).reshape(-1)[:44], 4, 11),
                           chol=np.ascontiguousarray(np.linalg.cholesky(np.asarray(cov, np.float32).astype(np.float64)
                                                                        .reshape(8, 8))))
        self.pop0 = np.ascontiguousarray(np.asarray(pop0, np.float32).reshape(-1, 8))
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        self.num_path, self.num_obs, self.total_obs = int(num_path), int(num_obs), int(total_obs)
        self.num_batch = self.pop0.shape[0]
        self.c = WorldModelStruct(self.num_path, self.num_obs, self.total_obs, R, int(goal_index), self.num_batch,
                                  NOISE[noise], dt, sigma_acc, sigma_steer, acc_const, steer_const, steer_max, a_obs,
                                  b_obs, y_lb, y_ub,
                                  *(dp(self.arrays[k]) for k in ("route_x", "route_y", "route_arc", "spline_x",
                                                                 "spline_y", "pdot4", "chol")), _fptr(self.pop0),
                                  int(seed) & 0xFFFFFFFF)


def _need_routed(L):
    if not hasattr(L, "mpcmmd_world_route_vehicles"):
        raise NativeError(f"{LIB_PATH} has no mpcmmd_world_route_vehicles (built before the routed vehicles existed): "
                          "rebuild it")


def routed_scalars(over):
    """The eight scalars of the routed vehicles in ROUTED_SCALARS' order, ROUTED_DEFAULTS overridden by ``over``."""
    extra = set(over) - set(ROUTED_SCALARS)
    if extra:
        raise ValueError(f"routed vehicles: unknown scalars {sorted(extra)}")
    return np.array([over.get(k, ROUTED_DEFAULTS[k]) for k in ROUTED_SCALARS], np.float32)


def world_step(model, tick, cx, cy, steer, u, mean, pos, ego, vehicles, done_tick, device=None, keys=None,
               routed=None):
    """One step of E episodes of the surrogate world: mpcmmd_world_step_host per
    episode (device None), or one k_world_step launch on GPU ``device``
    (mpcmmd_world_step_device).  cx, cy [E, 11], steer [E, >= 4] (the plan's
    steerings), u [E, 4] -- or None: drawn by the library from (keys [E], the
    model's seed, tick) once the controls are known -- mean [E, 8]; the state pos [E, 2] float64, ego
    [E, 3] = v, psi, psidot, vehicles [E, total_obs, 5], done_tick [E] is not
    modified.  Returns a dict: the new state under the same names, the next
    tick's init_state [E, 6], x_wp, y_wp [E, P], obstacles [E, O, 5], pop
    [E, B, 8] and the log row log_d [E, 3], log_f [E, 13], log_i [E, 4]
    (WORLD_LOG_D / _F / _I name the columns).

    routed = dict(s=[E, total_obs] float64, v=[E, total_obs], param=[E, total_obs, 2] = d, v0, plus any
    of ROUTED_SCALARS) steps the vehicles by the routed policy (DESIGN.md section 24,
    mpcmmd_world_step_host_routed / _device_routed): ``vehicles`` is then not read (None will do) and
    comes back as the rows the step made; the dict gains veh_s, veh_v (the new states) and veh_log
    [E, total_obs, 2] = v, a.  tick < 0 is then the reset-mode step (no plan read, no log row)."""
    L = lib()
    if routed is not None:
        _need_routed(L)
    if not hasattr(L, "mpcmmd_world_step_host"):
        raise NativeError(f"{LIB_PATH} has no mpcmmd_world_step_host (built before the entry point existed): rebuild it")
    E = np.asarray(pos).reshape(-1, 2).shape[0]
    m = model
    f = lambda a, *sh: np.array(np.asarray(a, np.float32).reshape(E, *sh), np.float32, order="C")
    if u is None and keys is None:
        raise ValueError("world_step: give the variates u or the episodes' keys")
    a = dict(cx=f(cx, 11), cy=f(cy, 11), steer=f(np.asarray(steer, np.float32).reshape(E, -1)[:, :4], 4),
             u=np.zeros((0, 4), np.float32) if u is None else f(u, 4),
             key=np.zeros(0, np.uint32) if keys is None else
             np.array(np.asarray(keys, np.int64).reshape(E) & 0xFFFFFFFF, np.uint32),
             mean=f(mean, 8), pos=np.array(np.asarray(pos, np.float64).reshape(E, 2), order="C"), ego=f(ego, 3),
             vehicles=np.zeros((E, m.total_obs, 5), np.float32) if routed is not None and vehicles is None
             else f(vehicles, m.total_obs, 5),
             done_tick=np.array(np.asarray(done_tick).reshape(E), np.int32, order="C"),
             init_state=np.empty((E, 6), np.float32), x_wp=np.empty((E, m.num_path), np.float32),
             y_wp=np.empty((E, m.num_path), np.float32), obstacles=np.empty((E, m.num_obs, 5), np.float32),
             pop=np.empty((E, m.num_batch, 8), np.float32), log_d=np.empty((E, 3), np.float64),
             log_f=np.empty((E, 13), np.float32), log_i=np.empty((E, 4), np.int32))
    names = [k for k, _ in WorldStepIO._fields_]

    def io_of(e):
        ptr = []
        for k in names:
            row = a[k][e:]   # the device call takes episode 0's address with every episode behind it
            ptr.append(C.cast(row.ctypes.data, dict(WorldStepIO._fields_)[k]) if row.size else None)
        return WorldStepIO(*ptr)

    if routed is not None:
        if int(tick) < 0:   # the reset-mode step writes no log row
            a["log_d"][:], a["log_f"][:], a["log_i"][:] = 0.0, 0.0, 0
        V = m.total_obs
        sc = routed_scalars({k: v for k, v in routed.items() if k not in ("s", "v", "param")})
        a["veh_s"] = np.array(np.asarray(routed["s"], np.float64).reshape(E, V), order="C")
        a["veh_v"], par = f(routed["v"], V), f(routed["param"], V, 2)
        a["veh_log"] = np.zeros((E, V, 2), np.float32)

        def rt_of(e):
            ptr = [C.cast(x[e:].ctypes.data, t) if x[e:].size else None
                   for x, (_, t) in zip((a["veh_s"], a["veh_v"], par, a["veh_log"]), WorldRouted._fields_)]
            return WorldRouted(*ptr, *[float(x) for x in sc])

        if device is None:
            for e in range(E):
                check(L.mpcmmd_world_step_host_routed(C.byref(m.c), int(tick), C.byref(io_of(e)), C.byref(rt_of(e))))
        else:
            check(L.mpcmmd_world_step_device_routed(C.byref(m.c), int(device), E, int(tick), C.byref(io_of(0)),
                                                    C.byref(rt_of(0))))
    elif device is None:
        for e in range(E):
            check(L.mpcmmd_world_step_host(C.byref(m.c), int(tick), C.byref(io_of(e))))
    else:
        check(L.mpcmmd_world_step_device(C.byref(m.c), int(device), E, int(tick), C.byref(io_of(0))))
    for k in ("cx", "cy", "steer", "u", "mean", "key"):
        del a[k]
    return a


def pad_ptr(a, ctype):
    """The address of ``a``'s data, or of a dummy word when it is empty (a NULL would be an argument error)."""
    if a.size:
        return a.ctypes.data_as(C.POINTER(ctype))
    return C.cast(C.pointer(C.c_double(0.0)), C.POINTER(ctype))


class _Episodes:
    """What World and Mpc share: they own one episode context of the library (mpcmmd_<_NAME>_*),
    registered with the object that must outlive it, and coerce the arrays of reset, run, log and
    the validation stage.  ``_U`` and ``_LOG`` are the row widths of u and of log_d, log_f, log_i
    and the plan, ``_COUNTS`` the count columns of the validation log, ``_VALIDATION`` its struct."""

    def _open(self, owner_ptr, siblings, handle, model, max_ticks):
        self._L = lib()
        if not hasattr(self._L, f"mpcmmd_{self._NAME}_create"):
            raise NativeError(f"{LIB_PATH} has no mpcmmd_{self._NAME}_create (built before the entry point existed): "
                              "rebuild it")
        self.model, self.max_ticks, self._handle, self._siblings = model, int(max_ticks), handle, siblings
        p = C.c_void_p()
        check(self._fn("create")(owner_ptr, C.byref(model.c), self.max_ticks, C.byref(p)))
        self._p = p
        self.E = 0
        siblings.append(self)   # the owner's close frees its contexts first

    def _fn(self, name):
        return getattr(self._L, f"mpcmmd_{self._NAME}_{name}")

    def close(self):
        if getattr(self, "_p", None):
            self._fn("destroy")(self._p)
            self._p = None
            if self in self._siblings:
                self._siblings.remove(self)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _reset(self, pos, state, vehicles, veh_shape, mean, cov, u, keys):
        pos = np.ascontiguousarray(np.asarray(pos, np.float64).reshape(-1, 2))
        E = self.E = pos.shape[0]
        f = lambda a, *sh: np.ascontiguousarray(np.asarray(a, np.float32).reshape(*sh))
        veh = f(vehicles, E, *veh_shape)
        kk = np.ascontiguousarray(np.asarray(keys, np.int64).reshape(E).astype(np.int32))
        check(self._fn("reset")(self._p, E, pos.ctypes.data_as(C.POINTER(C.c_double)), _fptr(f(state, E, 3)),
                                _fptr(veh) if veh.size else None, _fptr(f(mean, E, 8)), _fptr(f(cov, 64)),
                                None if u is None else _fptr(f(u, self.max_ticks, E, self._U)),
                                kk.ctypes.data_as(C.POINTER(C.c_int32))))
        self._handle._G = E

    def _run(self, cost, tick_begin, count, cov, v_des, *more):
        f = lambda a, *sh: np.ascontiguousarray(np.broadcast_to(np.asarray(a, np.float32), sh))
        check(self._fn("run")(self._p, COST[cost], int(tick_begin), int(count),
                              _fptr(np.ascontiguousarray(np.asarray(cov, np.float32).reshape(64))),
                              _fptr(f(np.asarray(v_des, np.float32).reshape(-1), self.E)), *more))

    def _log(self, ticks):
        """log_d, log_f, log_i, the plan rows and done_tick of the first ``ticks`` rows."""
        T, E, (wd, wf, wi, wp) = int(ticks), self.E, self._LOG
        ld, lf = np.empty((T, E, wd), np.float64), np.empty((T, E, wf), np.float32)
        li, pl, dn = np.empty((T, E, wi), np.int32), np.empty((T, E, wp), np.float32), np.empty(E, np.int32)
        ip = C.POINTER(C.c_int32)
        check(self._fn("log")(self._p, T, ld.ctypes.data_as(C.POINTER(C.c_double)), _fptr(lf), li.ctypes.data_as(ip),
                              _fptr(pl), dn.ctypes.data_as(ip)))
        return ld, lf, li, pl, dn

    def _validate(self, rollouts, alpha, sigma, **fields):
        if not hasattr(self._L, f"mpcmmd_{self._NAME}_validate"):
            raise NativeError(f"{LIB_PATH} has no mpcmmd_{self._NAME}_validate (built before the entry point existed): "
                              "rebuild it")
        self._val_S = 0
        if rollouts is None:
            check(self._fn("validate")(self._p, None))
            return
        sg = np.asarray(() if sigma is None else sigma, np.float32).reshape(-1)
        cfg = self._VALIDATION(int(rollouts), float(alpha), int(sg.size))
        for i, v in enumerate(sg[:8]):   # more than 8: num_sigma says so and the library refuses
            cfg.sigma[i] = float(v)
        for k, v in fields.items():
            setattr(cfg, k, v)
        check(self._fn("validate")(self._p, C.byref(cfg)))
        self._val_S = int(sg.size)

    def _validation_log(self, ticks):
        """val_counts, val_count_pos, the statistics [T, E, 4, 3], val_mmd and val_est of the first ``ticks`` rows."""
        T, E, S = int(ticks), self.E, getattr(self, "_val_S", 0)
        n = max(T, 0)
        cn, cp = np.zeros((n, E, self._COUNTS), np.int32), np.zeros((n, E, 3), np.int32)
        st, mm = np.zeros((n, E, 4, 3), np.float32), np.zeros((n, E, 3, S), np.float32)
        es = np.zeros((n, E, 2), np.float32)
        ip = C.POINTER(C.c_int32)
        check(self._fn("validation_log")(self._p, T, cn.ctypes.data_as(ip), cp.ctypes.data_as(ip), _fptr(st),
                                         _fptr(mm) if S else None, _fptr(es)))
        return dict(val_counts=cn, val_count_pos=cp, val_mmd=mm, val_est=es), st


class World(_Episodes):
    """Owns one mpcmmd_world: the chained closed loop of ``tick``'s handle on the
    surrogate world ``model`` (its num_path and num_obs must be the tick
    context's) for up to ``max_ticks`` ticks.  ``reset`` takes the episodes'
    start states, ``run(cost, tick_begin, count)`` enqueues begin, CEM and world
    step per tick with nothing crossing the host, ``log(ticks)`` performs the
    one readback.  Close it before its tick context."""
    _NAME, _U, _LOG, _COUNTS, _VALIDATION = "world", 4, (3, 13, 4, 34), 3, WorldValidation
    _w = property(lambda self: self._p)   # the raw context, for tests that call the C entry points themselves

    def __init__(self, tick, model, max_ticks):
        self.tick = tick
        self._open(tick._t, tick._worlds, tick.handle, model, max_ticks)   # Tick.close frees its worlds first

    def reset(self, pos, ego, vehicles, mean, cov, u, keys):
        """pos [E, 2] float64, ego [E, 3] = v, psi, psidot, vehicles [E, total_obs, 5], mean [E, 8],
        cov [8, 8], keys [E] (episode e solves tick k with idx_mpc = k + keys[e]), u [max_ticks, E, 4]
        or None: the kernel draws each tick's variates from (keys[e], the handle's seed, tick)."""
        none = vehicles is None and getattr(self, "_routed", False)
        self._reset(pos, ego, () if none else vehicles, (0 if none else self.model.total_obs, 5), mean, cov, u, keys)

    def run(self, cost, tick_begin, count, cov, v_des, threshold=0.1):
        self._run(cost, tick_begin, count, cov, v_des, float(threshold))

    def log(self, ticks):
        """The first ``ticks`` rows: dict of log_d, log_f, log_i, cx, cy, steering, mean_param, done_tick."""
        ld, lf, li, pl, dn = self._log(ticks)
        return dict(log_d=ld, log_f=lf, log_i=li, cx=pl[..., :11].copy(), cy=pl[..., 11:22].copy(),
                    steering=pl[..., 22:26].copy(), mean_param=pl[..., 26:].copy(), done_tick=dn)

    def route_vehicles(self, s, v=None, param=None, **scalars):
        """mpcmmd_world_route_vehicles: from the next ``reset`` on (which must be given as many episodes, and
        whose ``vehicles`` may be None), the vehicles follow the route.  s [E, total_obs]
        float64 arc lengths, v [E, total_obs] speeds, param [E, total_obs, 2] = d, v0 per vehicle; the
        scalars are ROUTED_SCALARS (defaults ROUTED_DEFAULTS).  ``s`` None turns the policy off."""
        _need_routed(self._L)
        if s is None:
            check(self._L.mpcmmd_world_route_vehicles(self._p, 0, None, None, None, None))
            self._routed = False
            return
        V = self.model.total_obs
        ss = np.ascontiguousarray(np.asarray(s, np.float64).reshape(-1, V))
        E = ss.shape[0] if V else int(np.asarray(param).shape[0])
        f = lambda a, *sh: np.ascontiguousarray(np.asarray(a, np.float32).reshape(*sh))
        vv, pp, sc = f(v, E, V), f(param, E, V, 2), routed_scalars(scalars)
        # a world without vehicles still hands over addresses: NULL arrays would turn the policy off
        pad = lambda x, dt: x if x.size else np.zeros(2, dt)
        check(self._L.mpcmmd_world_route_vehicles(self._p, E, pad(ss, np.float64).ctypes.data_as(C.POINTER(C.c_double)),
                                                  _fptr(pad(vv, np.float32)), _fptr(pad(pp, np.float32)), _fptr(sc)))
        self._routed = True

    def vehicle_log(self, ticks):
        """veh [ticks, E, total_obs, 3] float64: every routed vehicle's s, v and the acceleration applied,
        after each tick's step (v and a are the step's fp32 values, held exactly)."""
        _need_routed(self._L)
        T, E, V = int(ticks), self.E, self.model.total_obs
        vs, va = np.zeros((max(T, 0), E, V), np.float64), np.zeros((max(T, 0), E, V, 2), np.float32)
        check(self._L.mpcmmd_world_vehicle_log(self._p, T, pad_ptr(vs, C.c_double), pad_ptr(va, C.c_float)))
        return np.concatenate([vs[..., None], va.astype(np.float64)], -1)

    def validate(self, rollouts, alpha=0.98, sigma=()):
        """mpcmmd_world_validate: from the next ``reset`` on, every tick of ``run`` also computes the
        Monte-Carlo risk of the plan it made (``validate_carla_risk`` of that tick with ``rollouts``
        fresh noise rows, quantile level ``alpha`` and the MMD bandwidths ``sigma``, at most 8) into
        the validation log.  ``rollouts`` None turns the stage off."""
        self._validate(rollouts, alpha, sigma)

    def validation_log(self, ticks):
        """The first ``ticks`` rows of the validation log: val_counts [T, E, 3] (count, count_lane,
        count_rows of ``validate_carla``), val_count_pos [T, E, 3], val_var, val_cvar, val_mean,
        val_max [T, E, 3] (channels RISK_CHANNELS), val_mmd [T, E, 3, S] and val_est [T, E, 2]
        (the cost_lane and cost_obs the solve itself estimated)."""
        out, st = self._validation_log(ticks)
        return dict(out, val_var=st[:, :, 0].copy(), val_cvar=st[:, :, 1].copy(), val_mean=st[:, :, 2].copy(),
                    val_max=st[:, :, 3].copy())

    def validation_inputs(self):
        """The packed inputs of the last validated tick, as the validators read them: acc, steer [E, H],
        st0 [E, 8], path [E, 6, num_path], x_obs, y_obs [E, O, 100], keys [E] (uint32)."""
        E, h = self.E, self.tick.handle
        H, O, P = h.cfg.num_prime, h.cfg.num_obs, self.tick.num_path
        out = dict(acc=np.zeros((E, H), np.float32), steer=np.zeros((E, H), np.float32),
                   st0=np.zeros((E, 8), np.float32), path=np.zeros((E, 6, P), np.float32),
                   x_obs=np.zeros((E, O, 100), np.float32), y_obs=np.zeros((E, O, 100), np.float32),
                   keys=np.zeros(E, np.uint32))
        check(self._L.mpcmmd_world_validation_inputs(
            self._p, *[_fptr(out[k]) for k in ("acc", "steer", "st0", "path", "x_obs", "y_obs")],
            out["keys"].ctypes.data_as(C.POINTER(C.c_uint32))))
        return out


class MpcModel:
    """mpcmmd_mpc_model: the constants of the synthetic closed loop (DESIGN.md
    section 21).  ``cfg`` gives the noise kind and scalars, num_obs, num_batch,
    the seed and, through ``host_constant``, the rows of Pdot / Pddot and the
    variant's y_lb, y_ub, K_steer; keywords override.  cov the run's [8, 8]
    covariance (factored here as ``initial_population`` factors it), pop0
    [B, 8] standard normals (the host-linked routes: ``Handle.pop0``)."""

    def __init__(self, cfg, cov, pop0, goal_x, dt=0.15, a_obs=4.25, b_obs=2.75, **over):
        v = dict(zip(("y_lb", "y_ub", "K_steer"), host_constant(cfg, "mpc_scalars")))
        self.cfg = cfg
        self.num_obs, self.num_batch = int(over.pop("num_obs", cfg.num_obs)), int(cfg.num_batch)
        noise = over.pop("noise", cfg.noise)
        noise = NOISE[noise] if isinstance(noise, str) else int(noise)
        f = np.float32
        lvl = f(cfg.noise_level)
        p = dict(dt=f(dt), sigma_acc=lvl, sigma_steer=lvl, acc_const=f(cfg.acc_const_noise),
                 steer_const=f(cfg.steer_const_noise), K_steer=f(v["K_steer"] * float(lvl)), a_obs=f(a_obs),
                 b_obs=f(b_obs), y_lb=f(v["y_lb"]), y_ub=f(v["y_ub"]), goal_x=f(goal_x))
        seed = int(over.pop("seed", cfg.seed)) & 0xFFFFFFFF
        for k, val in over.items():
            if k not in p:
                raise TypeError(f"MpcModel: unknown keyword {k}")
            p[k] = f(val)
        self.scalars = p
        self.noise, self.seed = noise, seed
        pd = host_constant(cfg, "Pdot").reshape(-1, 11)
        pdd = host_constant(cfg, "Pddot").reshape(-1, 11)
        self.arrays = dict(pdot2=np.ascontiguousarray(pd[:2]), pddot1=np.ascontiguousarray(pdd[0]),
                           chol=np.ascontiguousarray(np.linalg.cholesky(
                               np.asarray(cov, np.float32).astype(np.float64).reshape(8, 8))))
        self.pop0 = np.ascontiguousarray(np.asarray(pop0, np.float32).reshape(-1, 8))
        if self.pop0.shape[0] != self.num_batch:
            raise ValueError("MpcModel: pop0 must be [num_batch, 8]")
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        self.c = MpcModelStruct(self.num_obs, self.num_batch, noise,
                                *(float(p[k]) for k in ("dt", "sigma_acc", "sigma_steer", "acc_const", "steer_const",
                                                        "K_steer", "a_obs", "b_obs", "y_lb", "y_ub", "goal_x")),
                                *(dp(self.arrays[k]) for k in ("pdot2", "pddot1", "chol")), _fptr(self.pop0), seed)


def pop0_normals(cfg):
    """mpcmmd_mpc_first_normals: the standard normals [B, 8] a handle of ``cfg`` draws for its first
    population (the pop0 of a model that steps that handle's loop on the host)."""
    out = np.empty((int(cfg.num_batch), 8), np.float32)
    check(lib().mpcmmd_mpc_first_normals(C.byref(cfg), _fptr(out)))
    return out


VEHICLE_CONSTANTS = ("kinv_x", "kinv_y", "colsum_x", "colsum_y", "P", "adv")


def _need_planned(L):
    if not hasattr(L, "mpcmmd_mpc_plan_vehicles"):
        raise NativeError(f"{LIB_PATH} has no mpcmmd_mpc_plan_vehicles (built before the planned vehicles existed): "
                          "rebuild it")


def mpc_vehicle_constant(dt, name):
    """mpcmmd_mpc_vehicle_constant: one of VEHICLE_CONSTANTS for the tick length ``dt`` (0 < dt < 15), the
    constants of the planned vehicles, as a flat float64 array.  No GPU needed."""
    L = lib()
    _need_planned(L)
    n = check(L.mpcmmd_mpc_vehicle_constant(float(np.float32(dt)), name.encode(), None, 0))
    out = np.empty(n, np.float64)
    check(L.mpcmmd_mpc_vehicle_constant(float(np.float32(dt)), name.encode(),
                                        out.ctypes.data_as(C.POINTER(C.c_double)), n))
    return out


def mpc_step(model, tick, cx, cy, u, mean, pos, vel, vehicles, done_tick, device=None, keys=None, planned=None):
    """One step of E episodes of the synthetic closed loop: mpcmmd_mpc_step_host
    per episode (device None), or one k_mpc_step launch on GPU ``device``
    (mpcmmd_mpc_step_device).  cx, cy [E, 11], u [E, 3] -- or None: drawn by the
    library from (keys [E], the model's seed, tick) once the controls are known
    -- mean [E, 8]; the state pos [E, 2] float64, vel [E, 3] = vx, vy, psi,
    vehicles [E, num_obs, 4], done_tick [E] is not modified.  Returns a dict:
    the new state under the same names, the next tick's init_state [E, 6], st0
    [E, 8], x_obs, y_obs [E, O, 100], pop [E, B, 8] and the log row log_d
    [E, 2], log_f [E, 12], log_i [E, 4] (MPC_LOG_D / _F / _I name the columns).

    planned = dict(acc=[E, O, 2], target=[E, O, 2]) steps the vehicles by their re-planned QP
    (mpcmmd_mpc_step_host_planned / _device_planned): acc the accelerations
    (ax, ay) that complete the rows of ``vehicles`` to the state S (None: zeros), target (v_des,
    y_des) per vehicle.  The dict gains veh_acc [E, O, 2] (the new accelerations) and veh_log
    [E, O, 6] (S after the step)."""
    L = lib()
    if not hasattr(L, "mpcmmd_mpc_step_host"):
        raise NativeError(f"{LIB_PATH} has no mpcmmd_mpc_step_host (built before the entry point existed): rebuild it")
    E = np.asarray(pos).reshape(-1, 2).shape[0]
    m = model
    f = lambda a, *sh: np.array(np.asarray(a, np.float32).reshape(E, *sh), np.float32, order="C")
    if u is None and keys is None:
        raise ValueError("mpc_step: give the variates u or the episodes' keys")
    O = m.num_obs
    a = dict(cx=f(cx, 11), cy=f(cy, 11), u=np.zeros((0, 3), np.float32) if u is None else f(u, 3),
             key=np.zeros(0, np.uint32) if keys is None else
             np.array(np.asarray(keys, np.int64).reshape(E) & 0xFFFFFFFF, np.uint32),
             mean=f(mean, 8), pos=np.array(np.asarray(pos, np.float64).reshape(E, 2), order="C"), vel=f(vel, 3),
             vehicles=f(vehicles, O, 4), done_tick=np.array(np.asarray(done_tick).reshape(E), np.int32, order="C"),
             init_state=np.empty((E, 6), np.float32), st0=np.empty((E, 8), np.float32),
             x_obs=np.empty((E, O, 100), np.float32), y_obs=np.empty((E, O, 100), np.float32),
             pop=np.empty((E, m.num_batch, 8), np.float32), log_d=np.empty((E, 2), np.float64),
             log_f=np.empty((E, 12), np.float32), log_i=np.empty((E, 4), np.int32))
    names = [k for k, _ in MpcStepIO._fields_]
    types = dict(MpcStepIO._fields_)

    def rows(src, k, e):
        row = src[k][e:]   # the device call takes episode 0's address with every episode behind it
        return C.cast(row.ctypes.data, C.POINTER(C.c_float)) if row.size else None

    def io_of(e):
        ptr = []
        for k in names:
            row = a[k][e:]
            ptr.append(C.cast(row.ctypes.data, types[k]) if row.size else None)
        return MpcStepIO(*ptr)

    if planned is not None:
        _need_planned(L)
        if set(planned) - {"acc", "target"} or "target" not in planned:
            raise TypeError("mpc_step: planned takes target and acc")
        acc = planned.get("acc")
        p = dict(veh_acc=np.zeros((E, O, 2), np.float32) if acc is None else f(acc, O, 2),
                 veh_target=f(planned["target"], O, 2), veh_log=np.empty((E, O, 6), np.float32))
        pl_of = lambda e: MpcPlanned(*(rows(p, k, e) for k in ("veh_acc", "veh_target", "veh_log")))
        if device is None:
            for e in range(E):
                check(L.mpcmmd_mpc_step_host_planned(C.byref(m.c), int(tick), C.byref(io_of(e)), C.byref(pl_of(e))))
        else:
            check(L.mpcmmd_mpc_step_device_planned(C.byref(m.c), int(device), E, int(tick), C.byref(io_of(0)),
                                                   C.byref(pl_of(0))))
        a.update(veh_acc=p["veh_acc"], veh_log=p["veh_log"])
    elif device is None:
        for e in range(E):
            check(L.mpcmmd_mpc_step_host(C.byref(m.c), int(tick), C.byref(io_of(e))))
    else:
        check(L.mpcmmd_mpc_step_device(C.byref(m.c), int(device), E, int(tick), C.byref(io_of(0))))
    for k in ("cx", "cy", "u", "mean", "key"):
        del a[k]
    return a


def _need_queue(L):
    if not hasattr(L, "mpcmmd_mpc_queue_reset"):
        raise NativeError(f"{LIB_PATH} has no mpcmmd_mpc_queue_reset (built before the scene queue existed): "
                          "rebuild it")


def mpc_queue(tick, ticks_per_episode, flags, keys, v_des, scene, ltick, done, key, slot_v_des, sched, count,
              device=None):
    """One lockstep tick of the scene queue's rule over E slots and N scenes:
    mpcmmd_mpc_queue_host (device None) or one k_mpc_queue launch on GPU ``device``
    (mpcmmd_mpc_queue_device).  flags [E, 4] is the step's log_i row, keys and v_des [N] the scene
    table's; scene, ltick, done, key, slot_v_des [E], sched [N, 4] and count [2] are the state before
    the tick.  Nothing given is modified; returns a dict of the state after it plus fresh and
    idx_mpc [E]."""
    L = lib()
    _need_queue(L)
    i32 = lambda a, *sh: np.ascontiguousarray(np.asarray(a, np.int64).astype(np.int32).reshape(*sh))
    fl, kt = i32(flags, -1, 4), i32(keys, -1)   # keys wrap to 32 bits
    E, N = fl.shape[0], kt.shape[0]
    vt = np.ascontiguousarray(np.asarray(v_des, np.float32).reshape(N))
    out = dict(scene=i32(scene, E).copy(), ltick=i32(ltick, E).copy(), done=i32(done, E).copy(),
               fresh=np.full(E, -7, np.int32), key=np.asarray(key, np.uint32).reshape(E).copy(),
               idx_mpc=np.full(E, -7, np.int32), slot_v_des=np.asarray(slot_v_des, np.float32).reshape(E).copy(),
               sched=i32(sched, N, 4).copy(), count=i32(count, 2).copy())
    ip = C.POINTER(C.c_int32)
    io = MpcQueueIO(E, N, int(ticks_per_episode), int(tick), fl.ctypes.data_as(ip), kt.ctypes.data_as(ip), _fptr(vt),
                    *[out[k].ctypes.data_as(ip) for k in ("scene", "ltick", "done", "fresh")],
                    out["key"].ctypes.data_as(C.POINTER(C.c_uint32)), out["idx_mpc"].ctypes.data_as(ip),
                    _fptr(out["slot_v_des"]), out["sched"].ctypes.data_as(ip), out["count"].ctypes.data_as(ip))
    if device is None:
        check(L.mpcmmd_mpc_queue_host(C.byref(io)))
    else:
        check(L.mpcmmd_mpc_queue_device(int(device), C.byref(io)))
    return out


class Mpc(_Episodes):
    """Owns one mpcmmd_mpc: the chained closed loop of a static / dynamic
    ``handle`` on ``model`` for up to ``max_ticks`` ticks.  ``reset`` takes the
    episodes' start states, ``run(cost, tick_begin, count)`` enqueues begin, CEM
    and k_mpc_step per tick with nothing crossing the host, ``log(ticks)``
    performs the one readback.  Close it before its handle."""
    _NAME, _U, _LOG, _COUNTS, _VALIDATION = "mpc", 3, (2, 12, 4, 30), 2, MpcValidation
    _c = property(lambda self: self._p)   # the raw context, for tests that call the C entry points themselves

    def __init__(self, handle, model, max_ticks):
        self.handle = handle
        self._open(handle._h, handle._ticks, handle, model, max_ticks)   # Handle.close frees its contexts first

    def reset(self, pos, vel, vehicles, mean, cov, u, keys):
        """pos [E, 2] float64, vel [E, 3] = vx, vy, psi, vehicles [E, num_obs, 4], mean [E, 8], cov
        [8, 8], keys [E] (episode e solves tick k with idx_mpc = k + keys[e]), u [max_ticks, E, 3] or
        None: the kernel draws each tick's variates from (keys[e], the handle's seed, tick)."""
        self._reset(pos, vel, vehicles, (self.model.num_obs, 4), mean, cov, u, keys)

    def run(self, cost, tick_begin, count, cov, v_des):
        self._run(cost, tick_begin, count, cov, v_des)

    def log(self, ticks):
        """The first ``ticks`` rows: dict of log_d, log_f, log_i, cx, cy, mean, done_tick."""
        ld, lf, li, pl, dn = self._log(ticks)
        return dict(log_d=ld, log_f=lf, log_i=li, cx=pl[..., :11].copy(), cy=pl[..., 11:22].copy(),
                    mean=pl[..., 22:].copy(), done_tick=dn)

    def plan_vehicles(self, target, acc=None):
        """mpcmmd_mpc_plan_vehicles: from the next ``reset`` on (which must be given as many episodes),
        the vehicles follow their re-planned QP.  target [E, O, 2] = v_des,
        y_des per vehicle, acc [E, O, 2] the start accelerations (None: zeros).  ``target`` None turns
        the policy off."""
        _need_planned(self._L)
        if target is None:
            check(self._L.mpcmmd_mpc_plan_vehicles(self._p, 0, None, None))
            return
        O = self.model.num_obs
        tg = np.ascontiguousarray(np.asarray(target, np.float32).reshape(-1, O, 2))
        ac = None if acc is None else np.ascontiguousarray(np.asarray(acc, np.float32).reshape(tg.shape))
        check(self._L.mpcmmd_mpc_plan_vehicles(self._p, tg.shape[0], _fptr(tg), None if ac is None else _fptr(ac)))

    def vehicle_log(self, ticks):
        """veh [ticks, E, O, 6]: every planned vehicle's state (x, y, vx, vy, ax, ay) after each tick's step."""
        _need_planned(self._L)
        out = np.zeros((max(int(ticks), 0), self.E, self.model.num_obs, 6), np.float32)
        check(self._L.mpcmmd_mpc_vehicle_log(self._p, int(ticks), _fptr(out)))
        return out

    def queue_reset(self, slots, ticks_per_episode, pos, vel, vehicles, mean, cov, v_des, keys, planned=None):
        """mpcmmd_mpc_queue_reset: the scene table of a campaign -- pos [N, 2]
        float64, vel [N, 3], vehicles [N, num_obs, 4], mean [N, 8], v_des [N], keys [N] and, with the
        planned policy on, planned = dict(target=[N, O, 2], acc=[N, O, 2]) -- through ``slots`` slots
        of at most ``ticks_per_episode`` ticks per scene.  Scenes 0..min(N, slots)-1 start at once."""
        _need_queue(self._L)
        pos = np.ascontiguousarray(np.asarray(pos, np.float64).reshape(-1, 2))
        N, O = pos.shape[0], self.model.num_obs
        f = lambda a, *sh: np.ascontiguousarray(np.broadcast_to(np.asarray(a, np.float32), sh))
        kk = np.ascontiguousarray(np.asarray(keys, np.int64).reshape(N).astype(np.int32))
        veh = f(np.asarray(vehicles, np.float32).reshape(N, O, 4), N, O, 4)
        arrs = [f(np.asarray(vel, np.float32).reshape(N, 3), N, 3), veh, f(np.asarray(mean, np.float32).reshape(-1, 8), N, 8),
                f(np.asarray(v_des, np.float32).reshape(-1), N)]
        pl = [None, None]
        if planned is not None:
            pl = [f(np.asarray(planned["target"], np.float32).reshape(N, O, 2), N, O, 2),
                  f(np.asarray(planned["acc"], np.float32).reshape(N, O, 2), N, O, 2)]
        sc = MpcScenes(N, pos.ctypes.data_as(C.POINTER(C.c_double)), *[_fptr(a) if a.size else None for a in arrs],
                       kk.ctypes.data_as(C.POINTER(C.c_int32)), *[None if a is None or not a.size else _fptr(a) for a in pl])
        check(self._L.mpcmmd_mpc_queue_reset(self._p, int(slots), int(ticks_per_episode), C.byref(sc),
                                             _fptr(f(np.asarray(cov, np.float32).reshape(64), 64))))
        self.E = self._handle._G = int(slots)
        self.N = N

    def queue_run(self, cost, tick_begin, count, cov):
        """mpcmmd_mpc_queue_run: ``count`` lockstep ticks from ``tick_begin``, all enqueued."""
        _need_queue(self._L)
        check(self._L.mpcmmd_mpc_queue_run(self._p, COST[cost], int(tick_begin), int(count),
                                           _fptr(np.ascontiguousarray(np.asarray(cov, np.float32).reshape(64)))))

    def queue_status(self):
        """mpcmmd_mpc_queue_status: synchronises; (started, finished) scenes."""
        _need_queue(self._L)
        a, b = C.c_int32(), C.c_int32()
        check(self._L.mpcmmd_mpc_queue_status(self._p, C.byref(a), C.byref(b)))
        return a.value, b.value

    def queue_log(self):
        """mpcmmd_mpc_queue_log: sched [N, 4] = slot, first lockstep tick, ticks run, end reason
        (``QUEUE_SCHED``, ``QUEUE_REASONS``)."""
        _need_queue(self._L)
        N = getattr(self, "N", 0)
        out = np.zeros((max(N, 1), 4), np.int32)
        check(self._L.mpcmmd_mpc_queue_log(self._p, out.ctypes.data_as(C.POINTER(C.c_int32))))
        return out[:N]

    def validate(self, rollouts, alpha=0.98, sigma=(), overlap=True):
        """mpcmmd_mpc_validate: from the next ``reset`` on, every tick of ``run`` also computes the
        Monte-Carlo risk of the plan it made (``validate`` and ``validate_risk`` of that tick with
        ``rollouts`` fresh noise rows, quantile level ``alpha`` and the MMD bandwidths ``sigma``, at
        most 8) into the validation log; ``overlap`` puts the validators' launches on the context's
        side stream, off the loop's critical path (False: in-line on the handle's stream; same bits).
        ``rollouts`` None turns the stage off."""
        self._validate(rollouts, alpha, sigma, overlap=int(overlap))

    def validation_log(self, ticks):
        """The first ``ticks`` rows of the validation log: val_counts [T, E, 2] (count, count_lane of
        ``validate``), val_count_pos [T, E, 3], val_stats [T, E, 4, 3] (var, cvar, mean, max by
        channels RISK_CHANNELS), val_mmd [T, E, 3, S] and val_est [T, E, 2] (the cost_lane and
        cost_obs the solve itself estimated)."""
        out, st = self._validation_log(ticks)
        return dict(out, val_stats=st)

    def validation_inputs(self):
        """The packed inputs of the last validated tick, as the validators read them: cx, cy [E, 11],
        init_state [E, 6] (float64), x_obs, y_obs [E, O, 100], keys [E] (uint32)."""
        E, O = self.E, self.model.num_obs
        out = dict(cx=np.zeros((E, 11)), cy=np.zeros((E, 11)), init_state=np.zeros((E, 6)),
                   x_obs=np.zeros((E, O, 100), np.float32), y_obs=np.zeros((E, O, 100), np.float32),
                   keys=np.zeros(E, np.uint32))
        dp = C.POINTER(C.c_double)
        check(self._L.mpcmmd_mpc_validation_inputs(
            self._p, *[out[k].ctypes.data_as(dp) for k in ("cx", "cy", "init_state")], _fptr(out["x_obs"]),
            _fptr(out["y_obs"]), out["keys"].ctypes.data_as(C.POINTER(C.c_uint32))))
        return out


class Tick:
    """Owns one mpcmmd_tick: the tick route of ``handle`` for paths of
    ``num_path`` points.  ``begin_batch`` / ``solve_batch`` take the raw data
    of len(idx_mpc) ticks (init_state [G, 6], x_wp / y_wp [G, num_path],
    obstacles [G, O, 5]) and do the whole per-tick setup on the handle's
    stream; afterwards the handle's own iterate / finish_batch / read apply.
    Close it before its handle."""

    def __init__(self, handle, num_path):
        self._L = lib()
        if not hasattr(self._L, "mpcmmd_tick_create"):
            raise NativeError(f"{LIB_PATH} has no mpcmmd_tick_create (built before the entry point existed): rebuild it")
        self.handle = handle
        self.num_path = int(num_path)
        t = C.c_void_p()
        check(self._L.mpcmmd_tick_create(handle._h, self.num_path, C.byref(t)))
        self._t = t
        self._keep = None
        self._worlds = []
        handle._ticks.append(self)   # Handle.close frees its tick contexts first

    def close(self):
        for w in list(getattr(self, "_worlds", [])):
            w.close()
        if getattr(self, "_t", None):
            self._L.mpcmmd_tick_destroy(self._t)
            self._t = None
            if self in self.handle._ticks:
                self.handle._ticks.remove(self)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _args(self, cost, idx_mpc, init_state, x_wp, y_wp, obstacles, threshold, mean, cov, v_des):
        h = self.handle
        G = len(idx_mpc)
        if G > h.max_configs:
            raise ValueError(f"{G} ticks > max_configs {h.max_configs}")
        f = lambda a, *sh: np.ascontiguousarray(np.broadcast_to(np.asarray(a, np.float32), sh))
        O, P = h.cfg.num_obs, self.num_path
        ins = dict(idx=np.ascontiguousarray(np.asarray(idx_mpc, np.int64).astype(np.int32)),
                   init=f(np.asarray(init_state, np.float32).reshape(G, 6), G, 6),
                   xw=f(np.asarray(x_wp, np.float32).reshape(G, P), G, P),
                   yw=f(np.asarray(y_wp, np.float32).reshape(G, P), G, P),
                   ob=f(np.asarray(obstacles, np.float32).reshape(G, O, 5), G, O, 5),
                   mean=f(mean, G, 8) if np.ndim(mean) == 2 else f(np.asarray(mean).reshape(8), G, 8),
                   cov=f(np.asarray(cov, np.float32).reshape(-1, 64), G, 64),
                   vd=f(np.asarray(v_des, np.float32).reshape(-1), G))
        ins["tin"] = TickInputs(_fptr(ins["init"]), _fptr(ins["xw"]), _fptr(ins["yw"]), _fptr(ins["ob"]),
                                float(threshold))
        self._keep = ins
        return G, (self._t, G, COST[cost], ins["idx"].ctypes.data_as(C.POINTER(C.c_int32)), C.byref(ins["tin"]),
                   _fptr(ins["mean"]), _fptr(ins["cov"]), _fptr(ins["vd"]))

    def begin_batch(self, cost, idx_mpc, init_state, x_wp, y_wp, obstacles, threshold, mean, cov, v_des):
        """mpcmmd_carla_tick_begin_batch (then the handle's iterate / finish_batch)."""
        G, args = self._args(cost, idx_mpc, init_state, x_wp, y_wp, obstacles, threshold, mean, cov, v_des)
        check(self._L.mpcmmd_carla_tick_begin_batch(*args))
        self.handle._G = G

    def solve_batch(self, cost, idx_mpc, init_state, x_wp, y_wp, obstacles, threshold, mean, cov, v_des):
        """begin_batch, iterate(0, T), finish_batch: one result dict per tick,
        bit-equal to ``Handle.carla_solve_batch`` on the host helpers' outputs."""
        self.begin_batch(cost, idx_mpc, init_state, x_wp, y_wp, obstacles, threshold, mean, cov, v_des)
        self.handle.iterate(0, self.handle.cfg.maxiter_cem)
        return self.handle.finish_batch()

    def path(self, g):
        """The device-made path of tick g of the last begin: a dict of PATH_KEYS."""
        img = self.handle.read("path").reshape(-1, 6, MAX_PATH)[g, :, :self.num_path]
        return {k: img[i].copy() for i, k in enumerate(PATH_KEYS)}


class Handle:
    """Owns one mpcmmd_handle (one device, one stream).  ``max_configs`` > 1
    sizes it for ``solve_batch`` (that many configurations per launch)."""

    def __init__(self, cfg, max_configs=1):
        self.cfg = cfg
        self.max_configs = int(max_configs)
        self._L = lib()
        if self._L.mpcmmd_device_count() < 1:
            raise NativeError("no HIP device visible: libmpcmmd needs an MI355X (gfx950)")
        h = C.c_void_p()
        check(self._L.mpcmmd_create_batch(C.byref(cfg), self.max_configs, C.byref(h)))
        self._h = h
        self._keep = []
        self._ticks = []

    def close(self):
        if getattr(self, "_h", None):
            for t in list(self._ticks):
                t.close()
            self._L.mpcmmd_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- solve ----------------------------------------------------------------
    def _inputs(self, init_state, mean, cov, x_obs, y_obs, draws):
        f = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float32))
        ins = dict(init_state=f(init_state).reshape(6), mean=f(mean).reshape(8), cov=f(cov).reshape(64),
                   x_obs=f(x_obs), y_obs=f(y_obs))
        if ins["x_obs"].shape != (self.cfg.num_obs, 100) or ins["y_obs"].shape != (self.cfg.num_obs, 100):
            raise ValueError(f"x_obs_traj / y_obs_traj must be [{self.cfg.num_obs}, 100]")
        d = None
        if draws is not None:
            keep = {}
            names = ("pop0", "roll", "resample", "beta_z0", "beta_z", "init_eps")
            for k in names:
                a = getattr(draws, k, None)
                keep[k] = None if a is None else np.ascontiguousarray(a, dtype=np.float32)
            d = Draws(*(_fptr(keep[k]) for k in names))
            ins["_draws_keep"] = keep
        ins["draws"] = d
        return ins

    def begin(self, cost, idx_mpc, init_state, mean, cov, x_obs, y_obs, v_des, draws=None):
        ins = self._inputs(init_state, mean, cov, x_obs, y_obs, draws)
        self._keep = [ins]
        d = ins["draws"]
        check(self._L.mpcmmd_begin(self._h, COST[cost], int(idx_mpc), _fptr(ins["init_state"]),
                                   _fptr(ins["mean"]), _fptr(ins["cov"]), _fptr(ins["x_obs"]),
                                   _fptr(ins["y_obs"]), float(v_des), None if d is None else C.byref(d)))

    def carla_begin(self, cost, idx_mpc, init_state, mean, cov, x_obs, y_obs, v_des, path, draws=None):
        """mpcmmd_carla_begin: compute_cem_mmd / compute_cem_cvar / compute_cem_det
        of the CARLA optimizer (carla/optimizer/cem.py:217-790; cost "mmd_opt",
        "cvar", "det"); path: dict of PATH_KEYS."""
        ins = self._inputs(init_state, mean, cov, x_obs, y_obs, draws)
        pth, keep = make_path(path)
        ins["_path"] = (pth, keep)
        self._keep = [ins]
        d = ins["draws"]
        check(self._L.mpcmmd_carla_begin(self._h, COST[cost], int(idx_mpc), _fptr(ins["init_state"]),
                                         _fptr(ins["mean"]), _fptr(ins["cov"]), _fptr(ins["x_obs"]),
                                         _fptr(ins["y_obs"]), float(v_des), C.byref(pth),
                                         None if d is None else C.byref(d)))

    def carla_solve(self, cost, idx_mpc, init_state, mean, cov, x_obs, y_obs, v_des, path, draws=None, trace=False):
        self.carla_begin(cost, idx_mpc, init_state, mean, cov, x_obs, y_obs, v_des, path, draws)
        self.iterate(0, self.cfg.maxiter_cem)
        return self.finish(trace)

    def iterate(self, t_begin, count):
        check(self._L.mpcmmd_iterate(self._h, int(t_begin), int(count)))

    def sync(self):
        check(self._L.mpcmmd_sync(self._h))

    def finish(self, trace=False):
        r = Result()
        beta = np.zeros(max(self.cfg.num_reduced, 1), np.float32)
        r.beta = _fptr(beta)
        steer = np.zeros(100, np.float32)
        vbest = np.zeros(100, np.float32)
        r.steering = _fptr(steer)
        r.v_best = _fptr(vbest)
        T, B = self.cfg.maxiter_cem, self.cfg.num_batch
        tr = None
        if trace:
            tr = dict(elite_proj=np.zeros((T, B), np.int32), elite_obs=np.zeros((T, 20), np.int32),
                      elite_cem=np.zeros((T, 5), np.int32))
            for k, v in tr.items():
                setattr(r, k, v.ctypes.data_as(C.POINTER(C.c_int32)))
        check(self._L.mpcmmd_finish(self._h, C.byref(r)))
        out = dict(cx=np.array(r.cx, np.float32), cy=np.array(r.cy, np.float32),
                   cost_lane=np.float32(r.cost_lane), cost_obs=np.float32(r.cost_obs),
                   sigma=np.float32(r.sigma), res_beta=np.array(r.res_beta, np.float32), beta=beta)
        if self.cfg.variant >= 2:
            out.update(steering=steer, v_best=vbest, mean_param=np.array(r.mean_param, np.float32))
        if tr is not None:
            out.update(tr)
        return out

    def _batch_inputs(self, idx_mpc, init_state, mean, cov, x_obs, y_obs, v_des):
        G = len(idx_mpc)
        if G > self.max_configs:
            raise ValueError(f"{G} configurations > max_configs {self.max_configs}")
        f = lambda a, *sh: np.ascontiguousarray(np.broadcast_to(np.asarray(a, np.float32), sh))
        O = self.cfg.num_obs
        ins = dict(idx=np.ascontiguousarray(np.asarray(idx_mpc, np.int64).astype(np.int32)),
                   init=f(init_state, G, 6) if np.ndim(init_state) == 2 else f(np.asarray(init_state).reshape(6), G, 6),
                   mean=f(mean, G, 8) if np.ndim(mean) == 2 else f(np.asarray(mean).reshape(8), G, 8),
                   cov=f(np.asarray(cov, np.float32).reshape(-1, 64), G, 64),
                   xo=f(np.asarray(x_obs, np.float32).reshape(G, O, 100), G, O, 100),
                   yo=f(np.asarray(y_obs, np.float32).reshape(G, O, 100), G, O, 100),
                   vd=f(np.asarray(v_des, np.float32).reshape(-1), G))
        args = (ins["idx"].ctypes.data_as(C.POINTER(C.c_int32)), _fptr(ins["init"]), _fptr(ins["mean"]),
                _fptr(ins["cov"]), _fptr(ins["xo"]), _fptr(ins["yo"]), _fptr(ins["vd"]))
        return G, ins, args

    def begin_batch(self, cost, idx_mpc, init_state, mean, cov, x_obs, y_obs, v_des):
        """mpcmmd_begin_batch (then iterate / finish_batch)."""
        G, ins, args = self._batch_inputs(idx_mpc, init_state, mean, cov, x_obs, y_obs, v_des)
        self._keep = [ins]
        check(self._L.mpcmmd_begin_batch(self._h, G, COST[cost], *args))
        self._G = G

    def carla_begin_batch(self, cost, idx_mpc, init_state, mean, cov, x_obs, y_obs, v_des, paths):
        """mpcmmd_carla_begin_batch (then iterate / finish_batch): len(idx_mpc)
        CARLA ticks in one batch, cost "mmd_opt", "cvar" or "det"; the arrays
        as ``solve_batch`` takes them; paths: one dict of PATH_KEYS per tick,
        all of one length."""
        if not hasattr(self._L, "mpcmmd_carla_begin_batch"):
            raise NativeError(f"{LIB_PATH} has no mpcmmd_carla_begin_batch (built before the entry point existed): "
                              "rebuild it")
        G, ins, args = self._batch_inputs(idx_mpc, init_state, mean, cov, x_obs, y_obs, v_des)
        if len(paths) != G:
            raise ValueError("one path per configuration")
        made = [make_path(p) for p in paths]
        pths = (Path * G)(*(m[0] for m in made))
        ins["_paths"] = (pths, made)
        self._keep = [ins]
        check(self._L.mpcmmd_carla_begin_batch(self._h, G, COST[cost], *args, pths))
        self._G = G

    def carla_solve_batch(self, cost, idx_mpc, init_state, mean, cov, x_obs, y_obs, v_des, paths):
        """mpcmmd_carla_solve_batch: one result dict per tick (the keys of
        ``carla_solve``), each bit-identical to ``carla_solve`` of that tick
        alone on a handle with the same "gen_wave"."""
        self.carla_begin_batch(cost, idx_mpc, init_state, mean, cov, x_obs, y_obs, v_des, paths)
        self.iterate(0, self.cfg.maxiter_cem)
        return self.finish_batch()

    def finish_batch(self):
        G = self._G
        rs = (Result * G)()
        betas = [np.zeros(max(self.cfg.num_reduced, 1), np.float32) for _ in range(G)]
        carla = self.cfg.variant >= 2
        steer = [np.zeros(100, np.float32) for _ in range(G)] if carla else None
        vbest = [np.zeros(100, np.float32) for _ in range(G)] if carla else None
        for g in range(G):
            rs[g].beta = _fptr(betas[g])
            if carla:
                rs[g].steering = _fptr(steer[g])
                rs[g].v_best = _fptr(vbest[g])
        check(self._L.mpcmmd_finish_batch(self._h, G, rs))
        out = [dict(cx=np.array(r.cx, np.float32), cy=np.array(r.cy, np.float32),
                    cost_lane=np.float32(r.cost_lane), cost_obs=np.float32(r.cost_obs), sigma=np.float32(r.sigma),
                    res_beta=np.array(r.res_beta, np.float32), beta=betas[g]) for g, r in enumerate(rs)]
        if carla:
            for g, r in enumerate(rs):
                out[g].update(steering=steer[g], v_best=vbest[g], mean_param=np.array(r.mean_param, np.float32))
        return out

    def solve_batch(self, cost, idx_mpc, init_state, mean, cov, x_obs, y_obs, v_des):
        """mpcmmd_solve_batch: len(idx_mpc) configurations in one batch.
        init_state / mean / cov / v_des may be shared (one value) or per
        configuration; x_obs, y_obs [G, O, 100].  Returns one result dict
        per configuration (the keys of finish())."""
        self.begin_batch(cost, idx_mpc, init_state, mean, cov, x_obs, y_obs, v_des)
        self.iterate(0, self.cfg.maxiter_cem)
        return self.finish_batch()

    def solve(self, cost, idx_mpc, init_state, mean, cov, x_obs, y_obs, v_des, draws=None, trace=False):
        self.begin(cost, idx_mpc, init_state, mean, cov, x_obs, y_obs, v_des, draws)
        self.iterate(0, self.cfg.maxiter_cem)
        return self.finish(trace)

    # -- stage access (parity tests) -------------------------------------------
    def buffer_bytes(self, name):
        n = C.c_size_t()
        check(self._L.mpcmmd_buffer_info(self._h, name.encode(), C.byref(n)))
        return n.value

    def read(self, name, dtype=np.float32, shape=None):
        nb = self.buffer_bytes(name)
        out = np.empty(nb // np.dtype(dtype).itemsize, dtype)
        check(self._L.mpcmmd_read(self._h, name.encode(), out.ctypes.data, out.nbytes))
        return out if shape is None else out[: int(np.prod(shape))].reshape(shape)

    def write(self, name, arr):
        arr = np.ascontiguousarray(arr)
        check(self._L.mpcmmd_write(self._h, name.encode(), arr.ctypes.data, arr.nbytes))

    def run_stage(self, stage, t):
        check(self._L.mpcmmd_run_stage(self._h, int(stage), int(t)))

    def info(self, name):
        """mpcmmd_handle_info: the handle's implementation choices ("gen_wave",
        "select_prep", "fused_small", "groups", "ker_path", "capacity")."""
        v = C.c_int64()
        check(self._L.mpcmmd_handle_info(self._h, name.encode(), C.byref(v)))
        return v.value

    # -- streams / profiling -----------------------------------------------------
    def set_stream(self, stream_ptr):
        check(self._L.mpcmmd_set_stream(self._h, C.c_void_p(stream_ptr)))

    def set_graphs(self, enable):
        """mpcmmd_set_graphs: replay whole solves as captured HIP graphs."""
        check(self._L.mpcmmd_set_graphs(self._h, 1 if enable else 0))

    def profile(self, enable):
        check(self._L.mpcmmd_profile(self._h, 1 if enable else 0))

    def kernel_times(self):
        n = 64
        la = (C.c_int32 * n)()
        ms = (C.c_double * n)()
        k = min(n, check(self._L.mpcmmd_kernel_times(self._h, la, ms, n)))
        return {self._L.mpcmmd_kernel_name(i).decode(): (la[i], ms[i]) for i in range(k)}
