/*
 * mpcmmd.h -- C ABI of libmpcmmd.so, the MI355X (gfx950) implementation of the
 * MMD / CVaR / SAA CEM-projection optimizer of Basant1861/MPC-MMD.
 *
 * The reference has no native code and no FFI: its optimizer is the Python
 * class `CEM` in synthetic_static_obs/optimizer/cem.py (pure JAX).  This ABI is
 * what that class's drop-in replacement (mpc-mmd_amd/optimizer/cem.py) binds
 * through ctypes; each entry point names the reference interface it replaces.
 * Plain C types only: no torch / HIP types in any signature (a stream is a
 * `void*` holding a hipStream_t).
 *
 * Threading: a handle is bound to one HIP device and one stream and is not
 * thread-safe; use one handle per thread / GPU.  Every call returns an int
 * status (0 = ok, < 0 = error; mpcmmd_last_error() has the message, thread
 * local).
 */
#ifndef MPCMMD_H
#define MPCMMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 4: MPCMMD_COST_DET (CARLA compute_cem_det), mpcmmd_handle_info
 * 5: mpcmmd_validate_carla */
#define MPCMMD_ABI_VERSION 5

/* status codes */
#define MPCMMD_OK 0
#define MPCMMD_E_INVALID (-1)     /* bad argument / shape */
#define MPCMMD_E_HIP (-2)         /* HIP runtime error (message has details) */
#define MPCMMD_E_UNSUPPORTED (-3) /* configuration outside what is built */
#define MPCMMD_E_STATE (-4)       /* call order (e.g. iterate before begin) */

/* cost variants: CEM.compute_cem_{mmd_opt,mmd_random,cvar,saa}
 * (synthetic_static_obs/optimizer/cem.py:201,335,464,590) */
#define MPCMMD_COST_MMD_OPT 0
#define MPCMMD_COST_MMD_RANDOM 1
#define MPCMMD_COST_CVAR 2
#define MPCMMD_COST_SAA 3
/* CARLA handles only: CEM.compute_cem_det of carla/optimizer/cem.py:633-790,
 * the deterministic baseline -- one noisy initial state, the projection with
 * its obstacle terms live (projection_det.py), no rollouts and no risk terms */
#define MPCMMD_COST_DET 4

/* noise models: Helper noise=="gaussian" / else beta (optimizer/cem_helper.py:405) */
#define MPCMMD_NOISE_GAUSSIAN 0
#define MPCMMD_NOISE_BETA 1

/* scenario constants: synthetic_static_obs vs synthetic_dynamic_obs
 * (y_lb,y_ub at optimizer/cem.py:155; K_steer at optimizer/cem_helper.py:24) */
#define MPCMMD_VARIANT_STATIC 0
#define MPCMMD_VARIANT_DYNAMIC 1
/* The CARLA optimizer (carla/optimizer/cem.py, CEM(num_reduced_sqrt,
 * num_mother, num_obs, noise_level, num_prime, noise, town, ...)): town
 * "Town05" / "Town10HD" select y_lb, y_ub, y_des (cem.py:161-166).  A CARLA
 * handle solves through the mpcmmd_carla_* entry points only (a path is
 * needed): mpcmmd_carla_begin / mpcmmd_carla_solve for one tick, and on a
 * handle of mpcmmd_create_batch with max_configs > 1 also
 * mpcmmd_carla_begin_batch / mpcmmd_carla_solve_batch for up to max_configs
 * independent ticks per launch. */
#define MPCMMD_VARIANT_CARLA_TOWN05 2
#define MPCMMD_VARIANT_CARLA_TOWN10HD 3

/* Replaces CEM.__init__(num_reduced, num_obs, noise_level, num_prime, noise,
 * acc_const_noise, steer_const_noise) (optimizer/cem.py:17-18).  num_batch is
 * the reference's hard-coded 100 (cem.py:137) made configurable. */
typedef struct mpcmmd_config {
  int32_t num_reduced;     /* n: samples per candidate (baseline) / reduced set (mmd_opt) */
  int32_t num_obs;         /* O */
  float noise_level;       /* sigma_acc = sigma_steer (cem.py:168-169) */
  int32_t num_prime;       /* H: rollout horizon */
  int32_t noise;           /* MPCMMD_NOISE_* */
  float acc_const_noise;
  float steer_const_noise;
  int32_t num_batch;       /* B (reference: 100) */
  int32_t variant;         /* MPCMMD_VARIANT_* */
  int32_t maxiter_cem;     /* outer CEM iterations (reference: 20, cem.py:89) */
  int32_t device;          /* HIP device ordinal */
  uint32_t seed;           /* key word 1 of the internal Philox streams */
} mpcmmd_config;

/* External draws (the parity contract): every standard normal the solve
 * consumes, host fp32 row-major.  A NULL field selects the internal Philox
 * stream for that tensor.  Shapes (T = maxiter_cem, S = num_reduced,
 * M = num_reduced^2):
 *   pop0     [B][8]             sampling_param, fixed key      (cem_helper.py:122-150)
 *   roll     [T][3][S][H]       acc / steer / const noise rows (cem_helper.py:405-441)
 *   resample [T][B-5][8]        compute_shifted_samples        (cem_helper.py:292)
 *   beta_z0  [100][M+1]         beta-CEM initial samples       (compute_beta.py:41-49)
 *   beta_z   [20][89][M+1]      beta-CEM resamples             (compute_beta.py:63)
 * Beta noise depends on the controls and is always internal. */
typedef struct mpcmmd_draws {
  const float* pop0;
  const float* roll;
  const float* resample;
  const float* beta_z0;
  const float* beta_z;
  /* CARLA: [R][4] normals of the noisy initial states, R = n^2 (mmd_opt) or
   * n (cvar) (compute_noisy_init_state(_baseline), carla/optimizer/
   * cem_helper.py:660-715) */
  const float* init_eps;
} mpcmmd_draws;

/* Return of compute_cem_* (cem.py:324-333 / 456-462): the obstacle-cost
 * elite 0 of the LAST outer iteration.  beta must point to >= n floats for
 * mmd_opt (may be NULL otherwise).  The trace pointers are optional (NULL =
 * not copied) and receive per-iteration elite index sets for parity tests:
 * elite_proj [T][B] (argsort of res_norm), elite_obs [T][20] (candidate
 * indices), elite_cem [T][5] (indices into the 20). */
typedef struct mpcmmd_result {
  float cx[11];
  float cy[11];
  float cost_lane;
  float cost_obs;
  float sigma;          /* mmd_opt */
  float res_beta[20];   /* mmd_opt */
  float* beta;          /* [n], mmd_opt */
  int32_t* elite_proj;
  int32_t* elite_obs;
  int32_t* elite_cem;
  /* CARLA return (carla/optimizer/cem.py:413-441): steering_best [100],
   * v_best [100] (optional, NULL = not written), mean_param after the last
   * iteration */
  float* steering;
  float* v_best;
  float mean_param[8];
} mpcmmd_result;

typedef struct mpcmmd_handle mpcmmd_handle;

int32_t mpcmmd_abi_version(void);
const char* mpcmmd_last_error(void);

/* Number of visible HIP devices (0 when none; never fails). */
int32_t mpcmmd_device_count(void);

/* CEM.__init__: allocates every device buffer and uploads the
 * batch-invariant matrices.  No allocation happens after this.
 * MPCMMD_E_UNSUPPORTED for num_reduced > 1024, num_obs * num_prime > 8192, or
 * (static / dynamic variants) a shape whose baseline risk stage needs more LDS
 * per workgroup than the device has (never on an MI355X: the largest accepted
 * shape needs 150 KiB of its 160). */
int mpcmmd_create(const mpcmmd_config* cfg, mpcmmd_handle** out);
void mpcmmd_destroy(mpcmmd_handle* h);

/* A handle that solves up to max_configs configurations of the same
 * CEM(...) shape in one go (mpcmmd_solve_batch): every stage is ONE launch
 * over (configuration x candidate), so the reference's num_batch = 100 sweep
 * (S/main_mpc.py:106-128, 200 independent configurations) fills the GPU.
 * Buffers are sized for max_configs * num_batch candidates (<= 65535).
 * mpcmmd_create(cfg, out) == mpcmmd_create_batch(cfg, 1, out). */
int mpcmmd_create_batch(const mpcmmd_config* cfg, int32_t max_configs, mpcmmd_handle** out);
int32_t mpcmmd_max_configs(mpcmmd_handle* h);

/* Implementation choices of a handle, fixed at create (no reference
 * counterpart: the reference has one JAX program).  name:
 *   "gen_wave"     1: the beta-CEM generators by one wave per 16-position block
 *                  (k_bgen_wave, fp64 MFMA), 0: a quad per block (k_bgen).  The
 *                  two sum in different orders, so their bits differ (both
 *                  within the parity tolerances).  Default: 1 when the handle's
 *                  capacity max_configs * num_batch <= 512 and num_reduced <= 24
 *                  -- the SAME problem can therefore give different bits on a
 *                  handle of 512 and one of 1024 candidates, or with another
 *                  max_configs.  Pin it with the environment variable
 *                  MPCMMD_GENWAVE=0/1 (read at create) to compare batch sizes.
 *                  CARLA batches alike: a tick's mmd_opt bits on a batch handle
 *                  of more than 512 candidates (say 6 x 100) differ from its
 *                  bits on the default 100-candidate handle unless pinned.
 *   "select_prep"  1: for cvar / saa / mmd_random the risk launch (stage 2) also
 *                  sorts the residuals and forms compute_cost's norms, so stage 3
 *                  needs stage 2 of the same iteration (MPCMMD_SELECT_PREP=0: in
 *                  stages 1 and 3; same bits either way)
 *   "fused_small"  1: small batches run the 20 beta-iterations as one launch
 *                  (k_bcem_small; same bits as the per-iteration kernels)
 *   "groups"       beta-CEM candidate groups on their own streams (same bits)
 *   "ker_path"     MPCMMD_KER_PATH as read at create: how k_bkernel forms K_red
 *                  (0 table or gather by union size, 1 union image, 2 gather; same bits)
 *   "capacity"     max_configs * num_batch
 * Writes *value; MPCMMD_E_INVALID for an unknown name. */
int mpcmmd_handle_info(mpcmmd_handle* h, const char* name, int64_t* value);

/* Run on a caller-owned hipStream_t instead of the handle's own stream. */
int mpcmmd_set_stream(mpcmmd_handle* h, void* hip_stream);
void* mpcmmd_get_stream(mpcmmd_handle* h);

/* CEM.compute_cem_{mmd_opt,mmd_random,cvar,saa}(idx_mpc, init_state,
 * mean_param_init, cov_param_init, x_obs_traj, y_obs_traj, v_des)
 * (cem.py:201-204 etc.).  x_obs / y_obs are [O][100] row-major.  draws may
 * be NULL (internal RNG).  Synchronous. */
int mpcmmd_solve(mpcmmd_handle* h, int32_t cost_kind, int32_t idx_mpc, const float init_state[6],
                 const float mean[8], const float cov[64], const float* x_obs, const float* y_obs,
                 float v_des, const mpcmmd_draws* draws, mpcmmd_result* out);

/* The same solve in three steps (what mpcmmd_solve does), for callers that
 * time or interleave work: begin uploads inputs and builds the initial carry
 * (sampling_param, compute_boundary_vec; cem.py:206-219); iterate enqueues
 * outer iterations [t_begin, t_begin+count) (the lax_cem body, cem.py:221-315)
 * asynchronously on the handle's stream; finish synchronises and downloads
 * the result of the last enqueued iteration. */
int mpcmmd_begin(mpcmmd_handle* h, int32_t cost_kind, int32_t idx_mpc, const float init_state[6],
                 const float mean[8], const float cov[64], const float* x_obs, const float* y_obs,
                 float v_des, const mpcmmd_draws* draws);
int mpcmmd_iterate(mpcmmd_handle* h, int32_t t_begin, int32_t count);
int mpcmmd_finish(mpcmmd_handle* h, mpcmmd_result* out);
int mpcmmd_sync(mpcmmd_handle* h);

/* n_cfg <= max_configs independent solves of the loop of S/main_mpc.py:106-128
 * (compute_cem_* per configuration) in one batch.  Arrays carry a leading
 * configuration axis: idx_mpc [n], init_state [n][6], mean [n][8], cov
 * [n][64], x_obs / y_obs [n][O][100], v_des [n]; out [n].  Configuration g
 * uses the internal RNG streams keyed by idx_mpc[g], so its result is
 * bit-identical to mpcmmd_solve of that configuration alone (external draws
 * are a single-configuration feature).  Synchronous. */
int mpcmmd_solve_batch(mpcmmd_handle* h, int32_t n_cfg, int32_t cost_kind, const int32_t* idx_mpc,
                       const float* init_state, const float* mean, const float* cov, const float* x_obs,
                       const float* y_obs, const float* v_des, mpcmmd_result* out);
/* The batch split like begin / iterate / finish (iterate is shared). */
int mpcmmd_begin_batch(mpcmmd_handle* h, int32_t n_cfg, int32_t cost_kind, const int32_t* idx_mpc,
                       const float* init_state, const float* mean, const float* cov, const float* x_obs,
                       const float* y_obs, const float* v_des);
int mpcmmd_finish_batch(mpcmmd_handle* h, int32_t n_cfg, mpcmmd_result* out);

/* ---- CARLA variant ---------------------------------------------------------
 * The path arguments of compute_cem_mmd / compute_cem_cvar
 * (carla/optimizer/cem.py:217-220, 444-448; main_carla.py:366-382), num_path
 * points each (reference: 600), fp32. */
typedef struct mpcmmd_path {
  int32_t num_path;
  const float* x_path;
  const float* y_path;
  const float* arc_vec;
  const float* Fx_dot;
  const float* Fy_dot;
  const float* kappa;
} mpcmmd_path;

/* CEM.compute_cem_mmd (cost_kind MPCMMD_COST_MMD_OPT) / compute_cem_cvar
 * (MPCMMD_COST_CVAR) / compute_cem_det (MPCMMD_COST_DET, num_obs <= 32) of
 * the CARLA optimizer (carla/optimizer/cem.py:217-790):
 * init_state = init_state_global (x, y, v, vdot, psi, psidot), x_obs / y_obs
 * the Frenet obstacle tracks [O][100], path as above.  begin then
 * mpcmmd_iterate / mpcmmd_finish, or solve in one call.  out->steering,
 * out->v_best, out->mean_param carry the reference's return
 * (cx, cy, v_best, steering_best, mean_param). */
int mpcmmd_carla_begin(mpcmmd_handle* h, int32_t cost_kind, int32_t idx_mpc, const float init_state[6],
                       const float mean[8], const float cov[64], const float* x_obs, const float* y_obs, float v_des,
                       const mpcmmd_path* path, const mpcmmd_draws* draws);
int mpcmmd_carla_solve(mpcmmd_handle* h, int32_t cost_kind, int32_t idx_mpc, const float init_state[6],
                       const float mean[8], const float cov[64], const float* x_obs, const float* y_obs, float v_des,
                       const mpcmmd_path* path, const mpcmmd_draws* draws, mpcmmd_result* out);
/* Both work on a handle of any max_configs, as n_cfg = 1 of the batch below.
 *
 * n_cfg <= max_configs independent CARLA solves (ticks) in one batch.  Arrays carry a
 * leading configuration axis as in mpcmmd_begin_batch; paths [n_cfg], every path with
 * the same num_path.  One cost_kind (mmd_opt, cvar or det) per batch.  Configuration g
 * uses the internal streams keyed by idx_mpc[g] (init_eps included), so its result is
 * bit-identical to mpcmmd_carla_solve of that tick alone on a handle with the same
 * "gen_wave" (mpcmmd_handle_info).  External draws: n_cfg == 1 only (use
 * mpcmmd_carla_begin).  Then mpcmmd_iterate / mpcmmd_finish_batch, which fills steering,
 * v_best and mean_param of every out[g].  Before any HIP call or upload:
 * MPCMMD_E_INVALID for a handle that is no CARLA variant's, n_cfg outside
 * 1..max_configs, a NULL array (inside a path too), num_path outside 4..2048 or not the
 * same for every configuration; MPCMMD_E_UNSUPPORTED for det with num_obs > 32.  The ABI
 * version is unchanged: callers detect the two entry points by their symbols. */
int mpcmmd_carla_begin_batch(mpcmmd_handle* h, int32_t n_cfg, int32_t cost_kind, const int32_t* idx_mpc,
                             const float* init_state, const float* mean, const float* cov,
                             const float* x_obs, const float* y_obs, const float* v_des,
                             const mpcmmd_path* paths);
int mpcmmd_carla_solve_batch(mpcmmd_handle* h, int32_t n_cfg, int32_t cost_kind, const int32_t* idx_mpc,
                             const float* init_state, const float* mean, const float* cov,
                             const float* x_obs, const float* y_obs, const float* v_des,
                             const mpcmmd_path* paths, mpcmmd_result* out);

/* ---- CARLA tick route -------------------------------------------------------
 * The per-tick preprocessing of main_carla.py:345-376 (custom_path_smoothing,
 * compute_path_parameters, global_to_frenet_obs_vmap, compute_obs_trajectories)
 * and the per-tick host arithmetic of mpcmmd_carla_begin_batch (the noisy
 * initial rows, their Frenet states and mean, the boundary vectors, the KKT
 * columns) on the handle's stream, from the raw data of n_cfg ticks: two
 * kernels (k_tick.hip) between one upload and the first CEM iteration, with no
 * device-to-host copy and no stream synchronisation beyond the wait for the
 * previous begin's staging copies.  Afterwards the handle is in exactly the
 * state mpcmmd_carla_begin_batch leaves it in when given the host helpers'
 * outputs for the same ticks: every buffer and every result is bit-equal
 * (tests/test_gpu_carla_tick.py), because every sum the host forms
 * sequentially is formed in the same order on the device.
 *
 * A tick context belongs to one handle and one num_path (4..2048).  It owns
 * its device memory (the (num_path+1)^2 fp64 smoothing inverse, uploaded once;
 * the KKT coefficient columns; the tick inputs; the rows' Frenet scratch) and
 * its pinned staging with its own event; none of it is in the handle's buffer
 * list.  Dynamic LDS of either kernel: 24 num_path + 16 bytes (49168 at 2048);
 * mpcmmd_tick_create returns MPCMMD_E_UNSUPPORTED if the device's workgroup
 * limit is below that.  Destroy the context before its handle.  Threading and
 * device binding are the handle's.  ABI version unchanged: detect the entry
 * points by their symbols. */
typedef struct mpcmmd_tick mpcmmd_tick;
int mpcmmd_tick_create(mpcmmd_handle* h, int32_t num_path, mpcmmd_tick** out);
void mpcmmd_tick_destroy(mpcmmd_tick* t);

typedef struct mpcmmd_tick_inputs { /* leading axis n_cfg */
  const float* init_state; /* [n][6] init_state_global (main_carla.py:352) */
  const float* x_wp;       /* [n][num_path] waypoints shifted to the ego: custom_path_smoothing's input */
  const float* y_wp;
  /* [n][num_obs][5]: x, y (shifted to the ego), vx, vy, psi of the num_obs nearest obstacles, in order.
   * psi is needed: global_to_frenet_obs scales the speed by cos / sin of (psi - path heading), so it
   * reaches vx and vy of every moving obstacle. */
  const float* obstacles;
  float threshold; /* custom_path_smoothing's (driver: 0.1) */
} mpcmmd_tick_inputs;

/* begin of n_cfg ticks through the tick route, then mpcmmd_iterate /
 * mpcmmd_finish_batch / mpcmmd_set_graphs / mpcmmd_read of the context's
 * handle; the device-made path of tick g is slice g of mpcmmd_read(h, "path")
 * ([6][2048]: x, y, arc_vec, Fx_dot, Fy_dot, kappa, zero beyond num_path).
 * Internal RNG streams only (init_eps keyed by idx_mpc[g], as in the batch
 * begin).  Before any HIP call: MPCMMD_E_INVALID for a NULL argument or array,
 * a handle of no CARLA variant, n_cfg outside 1..max_configs, a threshold that
 * is not finite, a cost other than mmd_opt, cvar or det; MPCMMD_E_UNSUPPORTED
 * for det with num_obs > 32 and for mmd_opt on a handle without it.  A failure
 * after the first enqueue drains the stream before the staging is reused. */
int mpcmmd_carla_tick_begin_batch(mpcmmd_tick* t, int32_t n_cfg, int32_t cost_kind, const int32_t* idx_mpc,
                                  const mpcmmd_tick_inputs* in, const float* mean, const float* cov,
                                  const float* v_des);
/* begin, mpcmmd_iterate(0, T), mpcmmd_finish_batch */
int mpcmmd_carla_tick_solve_batch(mpcmmd_tick* t, int32_t n_cfg, int32_t cost_kind, const int32_t* idx_mpc,
                                  const mpcmmd_tick_inputs* in, const float* mean, const float* cov,
                                  const float* v_des, mpcmmd_result* out);

/* The host route of the same tick in one call (no GPU needed): path_smoothing,
 * path_parameters, global_to_frenet of the obstacles (v = sqrtf(vx^2 + vy^2),
 * vdot = psidot = 0) and their tracks x[o][k] = x_o + vx_o tt[k] in fp32 on
 * tt = np.linspace(0, 15, 100).astype(float32).  obstacles [num_obs][5] as in
 * mpcmmd_tick_inputs; path6 [6][num_path]: x, y, arc_vec, Fx_dot, Fy_dot,
 * kappa; x_obs, y_obs [num_obs][100].  init_state is not used by the
 * preprocessing (it is the solve's) and must not be NULL. */
int mpcmmd_carla_tick_host(int32_t num_path, int32_t num_obs, const float init_state[6], const float* x_wp,
                           const float* y_wp, const float* obstacles, float threshold, float* path6, float* x_obs,
                           float* y_obs);

/* Helper.custom_path_smoothing(x_waypoints, y_waypoints, threshold)
 * (carla/optimizer/cem_helper.py:279-318, 391-410): 10 ADMM iterations of the
 * jerk-smoothing QP; the (num_path+1)^2 KKT inverse is built once per
 * num_path (fp64).  Host; no GPU needed. */
int mpcmmd_path_smoothing(int32_t num_path, const float* x_wp, const float* y_wp, float threshold, float* x_path,
                          float* y_path);
/* Helper.compute_path_parameters(x_path, y_path) (cem_helper.py:321-345).
 * Host; arc_length may be NULL. */
int mpcmmd_path_parameters(int32_t num_path, const float* x_path, const float* y_path, float* Fx_dot, float* Fy_dot,
                           float* Fx_ddot, float* Fy_ddot, float* arc_vec, float* kappa, float* arc_length);
/* Helper.global_to_frenet (cem_helper.py:348-388) of count states; out
 * [count][7] = (x, y, vx, vy, ax, ay, psi) in the Frenet frame
 * (global_to_frenet_obs, :171-200, is this with vdot = psidot = 0 and
 * v = |(vx, vy)|).  Host. */
int mpcmmd_global_to_frenet(const mpcmmd_path* path, int32_t count, const float* x, const float* y, const float* v,
                            const float* vdot, const float* psi, const float* psidot, float* out);

/* Whole-solve HIP graphs: with enable != 0, mpcmmd_iterate(h, 0, T) captures
 * the solve's launch sequence once per (cost, path length, external draws,
 * configurations) and replays it with one hipGraphLaunch (handles whose
 * launches use one stream, i.e. fewer than 1024 candidates).  Results are
 * identical to the launched sequence.  Default off (environment MPCMMD_GRAPH=1
 * turns it on at create). */
int mpcmmd_set_graphs(mpcmmd_handle* h, int32_t enable);

/* Per-kernel HIP-event timing (on the handle's stream).  When enabled, every
 * launch of every kernel is bracketed by events; mpcmmd_kernel_times returns,
 * per kernel id, the number of launches and the total milliseconds since the
 * last reset.  Kernel ids: see mpcmmd_kernel_name. */
int mpcmmd_profile(mpcmmd_handle* h, int32_t enable);
int mpcmmd_kernel_times(mpcmmd_handle* h, int32_t* launches, double* total_ms, int32_t max_kernels);
const char* mpcmmd_kernel_name(int32_t id);

/* Named device buffers, for stage-level parity tests (read / overwrite the
 * scan carry and intermediates between stages).  Names and sizes: see
 * mpcmmd_buffer_info; the name "*" gives the total bytes of every buffer of
 * the handle.  Tests can cap a handle's device memory with the environment
 * variable MPCMMD_MAX_HANDLE_BYTES (read at create): buffers past the cap fail
 * with the runtime's own out-of-memory error. */
int mpcmmd_buffer_info(mpcmmd_handle* h, const char* name, size_t* bytes);
int mpcmmd_read(mpcmmd_handle* h, const char* name, void* dst, size_t bytes);
int mpcmmd_write(mpcmmd_handle* h, const char* name, const void* src, size_t bytes);

/* Stage entry points: run one kernel of iteration t on the current device
 * state (the stages mpcmmd_iterate chains):
 *   0 noise      (internal RNG draws of iteration t)
 *   1 front      compute_x_guess + compute_projection + compute_controls
 *                (cem_helper.py:169-230, projection.py:276-323, cem_helper.py:540-551)
 *   2 risk       noisy rollouts + collision residual + risk reducer per candidate
 *                (cem_helper.py:402-538, costs.py:50-234, compute_beta.py:93-157)
 *   3 select     argsorts, compute_cost, elites, compute_shifted_samples
 *                (cem.py:233-315, cem_helper.py:232-314).  With the select
 *                preparation on (mpcmmd_handle_info "select_prep": cvar / saa /
 *                mmd_random) stage 2 sorts the residuals and forms the cost
 *                norms, so stage 3 needs stage 2 of the same iteration after
 *                stage 1 (else MPCMMD_E_INVALID)
 * cost = mmd_opt splits stage 2 into sub-stages (t = outer iteration for 4, 8;
 * t = beta-CEM iteration 0..19 for 5-7):
 *   4 mother     noisy rows, n^2 mother rollouts, Bernstein fit (cem_helper.py:469-564)
 *   5 bsample    beta-CEM samples + top-n |beta| rows     (compute_beta.py:41-68, 117-118)
 *   6 bkernel    kernel row sums, reduced QP, QP cost     (compute_beta.py:70-91, 120-129)
 *   7 belite     elites, mean, next generators             (compute_beta.py:51-68, 133-157)
 *   8 mmdfinal   reduced rollouts, MMD obs / lane          (costs.py:121-135, 173-186)
 * Buffer "beta_z" holds the device layout [20][P][96], P = M+1 rounded up to
 * 16, zero padded (transposed on upload in mpcmmd_begin; mpcmmd_write writes
 * it raw). */
int mpcmmd_run_stage(mpcmmd_handle* h, int32_t stage, int32_t t);

/* Host-side batch-invariant constants (no GPU needed): fills dst with the
 * fp64 values of `name` ("P","Pdot","Pddot" [100][11] (fp32-rounded),
 * "P_prime" [H][11], "guess_kinv_x" [14][14], "guess_kinv_y" [15][15],
 * "proj_kinv_x", "proj_kinv_y", "fit" [11][H], "det_kinv_x", "det_kinv_y"
 * (the CARLA det projection's, for cfg->num_obs obstacles), "mpc_scalars" [3] = the
 * variant's y_lb, y_ub, K_steer (mpcmmd_mpc_model)).  Returns element count, or
 * < 0 on error / when count is too small. */
int mpcmmd_host_constant(const mpcmmd_config* cfg, const char* name, double* dst, size_t count);

/* Dynamic-obstacle trajectories of the synthetic_dynamic_obs driver:
 * obs_data.compute_boundary_vec + obs_data.compute_obs_guess
 * (synthetic_dynamic_obs/obs_data_generate_dynamic.py:56-109, called per
 * obstacle at synthetic_dynamic_obs/main_mpc.py:116-126).  Obstacle i starts
 * at (x0[i], y0[i]) with speed (vx0[i], vy0[i]) and zero acceleration and
 * tracks speed v_des[i] (obs_data.sampling_param, :111-133) and lane y_des
 * (the driver passes -1.75).  Writes x_traj, y_traj [num_obs][100].  Host
 * fp64 KKT (inverted once), fp32 output; no GPU needed. */
int mpcmmd_obs_dynamic_traj(int32_t num_obs, const float* x0, const float* y0, const float* vx0, const float* vy0,
                            const float* v_des, float y_des, float* x_traj, float* y_traj);

/* Monte-Carlo validation of saved optima on the GPU: synthetic_static_obs/
 * validation.py compute_stats (:134-171) for num_cfg configurations at
 * once.  Per configuration k: controls of the saved trajectory (cx, cy)
 * (compute_controls :122-132), num_rollouts noisy fp64 rollouts from
 * init_state (compute_rollout_complete :42-101), then
 *   count[k]      = max over (obstacle, step) of #rollouts inside the ellipse
 *   count_lane[k] = max_step #(y < y_lb) + max_step #(y > y_ub)
 * (:153-169).  x_obs / y_obs: [num_cfg][num_obs][100] obstacle tracks
 * (compute_obs_trajectories).  draws: [num_cfg][3][num_rollouts][num_prime]
 * fp64 -- gaussian: the standard normals of acc, steer, const noise; beta:
 * the Beta(2|acc|, 5|acc|) and Beta(2|steer|+1e-5, 5|steer|+1e-5) draws and
 * the const normals -- or NULL for the library's Philox streams keyed by
 * (keys[k], seed).  Synchronous; allocates its own device buffers. */
typedef struct mpcmmd_validate_args {
  int32_t num_cfg, num_obs, num_prime, num_rollouts;
  int32_t noise;          /* MPCMMD_NOISE_* */
  int32_t variant;        /* MPCMMD_VARIANT_* (y_lb, y_ub, K_steer) */
  double noise_level, acc_const_noise, steer_const_noise;
  uint32_t seed;
  int32_t device;
  const double* cx;       /* [num_cfg][11] */
  const double* cy;
  const double* init_state; /* [num_cfg][6] */
  const float* x_obs;
  const float* y_obs;
  const double* draws;
  const uint32_t* keys;   /* [num_cfg] (validation.py seeds np.random with the config key) */
  int32_t* count;         /* [num_cfg] out */
  int32_t* count_lane;    /* [num_cfg] out */
} mpcmmd_validate_args;
int mpcmmd_validate(const mpcmmd_validate_args* args);

/* Monte-Carlo validation of CARLA plans on the GPU.  The reference measures
 * CARLA safety with the live simulator's collision sensor only; this call
 * evaluates the optimizer's own risk model instead -- the cvar risk stage of
 * carla/optimizer/cem.py (noisy initial states, noisy rollouts in the global
 * frame, closest-point Frenet transform, collision / lane bars) -- with
 * num_rollouts fresh noise rows, reduced as validation.py:153-169 reduces
 * (counts, not CVaR).  One configuration k is one simulator tick with one
 * returned plan; num_cfg ticks run in one launch.  fp32 arithmetic with the
 * fp64-evaluated transcendentals of the optimizer's CARLA rollouts.
 *
 * Per tick k (R = num_rollouts, H = num_prime, O = num_obs, P = num_path):
 *   controls  acc[h] = (v[h+1] - v[h]) / 0.15f with v[100] = v[99], steer[h] as
 *             given (the solve's v_best, steering_best); only h < H - 1 is used
 *   rows      (x0 + (eps[r][0] sx + mx), y0 + (eps[r][1] sy + my), vx, vy,
 *             atan2(vy, vx)) from init_state = init_state_global (x, y, v,
 *             vdot, psi, psidot): the noisy initial rows of mpcmmd_carla_begin
 *   noise     gaussian  acc + (sigma |acc|) n_a + acc_const n_c
 *             beta      acc + sigma (2 b_a - 1) + acc_const n_c
 *             steer likewise (beta: K_steer sigma), per (row, step)
 *   rollout   the point recorded at h is the state before step h
 *   counts    hit[o][r][h]  = !(f_bar(s, d, x_obs[o][h], y_obs[o][h]) <= 0) on
 *                             the point's Frenet (s, d) against the tick's path
 *             count_oh[o][h] = sum_r hit
 *             count[k]       = max_{o,h} count_oh
 *             count_rows[k]  = #{r : any hit}   (collision probability x R)
 *             count_lane[k]  = max_h #(-d + y_lb > 0) + max_h #(d - y_ub > 0)
 *
 * draws [num_cfg][3][R][H] fp32 -- gaussian: the standard normals of acc,
 * steer, const; beta: the two Beta variates and the const normals -- and
 * init_eps [num_cfg][R][4] fp32 (columns 0, 1 used; mpcmmd_draws.init_eps'
 * layout).  Either may be NULL: then the library's Philox streams keyed
 * (keys[k], seed) are used, streams 32..34 (normals of acc, steer, const), 35..38
 * (the gammas of Beta(2|acc|, 5|acc|) and Beta(2|steer|, 5|steer|): acc a, acc b,
 * steer a, steer b; fp64 combine as the CARLA optimizer) and 39 (init_eps), element
 * r H + h of the [R][H] tensors and r 4 + c of init_eps.
 *
 * Limits: 1 <= num_obs <= 32, 2 <= num_prime <= 100, 4 <= num_path <= 2048,
 * num_rollouts >= 1 (num_rollouts * num_prime < 2^31), num_cfg <= 65535;
 * variant one of the two MPCMMD_VARIANT_CARLA_*.  Anything else is
 * MPCMMD_E_INVALID before any HIP call; num_cfg == 0 returns MPCMMD_OK without
 * touching a device.  A shape whose workgroup does not fit the device's LDS
 * is MPCMMD_E_UNSUPPORTED (never on an MI355X: the largest shape needs 130 KiB).
 * Synchronous, needs no handle, allocates its own device buffers. */
typedef struct mpcmmd_validate_carla_args {
  int32_t num_cfg, num_obs, num_prime, num_rollouts, num_path;
  int32_t noise;            /* MPCMMD_NOISE_* */
  int32_t variant;          /* MPCMMD_VARIANT_CARLA_* (y_lb, y_ub) */
  float noise_level, acc_const_noise, steer_const_noise;
  uint32_t seed;
  int32_t device;
  const float* init_state;  /* [num_cfg][6] init_state_global */
  const float* v;           /* [num_cfg][100] v_best */
  const float* steer;       /* [num_cfg][100] steering_best */
  const float* x_obs;       /* [num_cfg][num_obs][100] Frenet tracks */
  const float* y_obs;
  const float* path;        /* [num_cfg][6][num_path]: x_path, y_path, arc_vec, Fx_dot, Fy_dot, kappa */
  const float* draws;       /* [num_cfg][3][R][H] or NULL */
  const float* init_eps;    /* [num_cfg][R][4] or NULL */
  const uint32_t* keys;     /* [num_cfg] */
  int32_t* count;           /* [num_cfg] out */
  int32_t* count_lane;      /* [num_cfg] out */
  int32_t* count_rows;      /* [num_cfg] out */
  int32_t* count_oh;        /* [num_cfg][num_obs][num_prime] out, or NULL (not copied) */
  float* elapsed_ms;        /* out, or NULL: HIP-event time of the device work (counter reset + the two kernels) */
} mpcmmd_validate_carla_args;
int mpcmmd_validate_carla(const mpcmmd_validate_carla_args* args);

/* Monte-Carlo risk statistics of saved optima on the GPU: the optimizer's own
 * cost terms (costs.py:121-234, kernel_computation.py:67-87) evaluated on the
 * num_rollouts noisy rollouts of mpcmmd_validate instead of the solve's n
 * samples.  The plan inputs, the draws layout and -- with draws == NULL -- the
 * Philox streams and element indices are mpcmmd_validate's: the same (keys,
 * seed) rolls the same points in both calls.  ABI version unchanged; detect
 * the entry point by its symbol.
 *
 * Per configuration k (R = num_rollouts, H = num_prime, O = num_obs, S =
 * num_sigma) three channels c of per-rollout costs, from the fp64 rollout
 * whose point at step h is the state before step h (h < H):
 *   obs[r]     = max over (o, h) of max(0, f_bar), f_bar = -(x - x_obs)^2 / 4.25^2
 *                - (y - y_obs)^2 / 2.75^2 + 1 in fp64
 *   lane_lb[r] = max over h of max(0, -y + y_lb)
 *   lane_ub[r] = max over h of max(0,  y - y_ub)
 * each rounded once to fp32, the optimizer's dtype.  With costs_in
 * [num_cfg][3][R] the rollouts are skipped (the plan pointers may be NULL) and
 * the statistics are taken of the given samples.
 *
 * Outputs per (k, c), all fp32 unless noted:
 *   count_pos  int32 #{r : !(c[r] <= 0)} (a NaN counts)
 *   var        the linear quantile at alpha with fp32 weights (jnp.quantile):
 *              pos = fp32(alpha) fp32(R - 1), lo = floor, hi = ceil, hw = pos -
 *              lo, lw = 1 - hw, var = v[lo] lw + v[hi] hw in fp32 without
 *              contraction on the ascending order with -0 == +0 and NaN last
 *              (mpcmmd_quantile_position gives lo, hi, lw, hw).  At R = n this
 *              is bit for bit the cvar reducer's VaR.
 *   cvar       mean of the samples >= var that are not NaN (fp64 sum / their
 *              count), 0 if there are none.  When fewer than (1 - alpha) R
 *              samples are positive, var = 0 and this is the mean of all
 *              samples, as in the reference.
 *   mean, max  fp64 sum / R; the largest value in the total order (NaN if any)
 *   mmd [S]    1000 ((1/R^2) sum_ij e(|c_i - c_j| / sigma) - (2/R) sum_i
 *              e(|c_i| / sigma)), e(x) = exp(-x) evaluated as exp2(d (-log2 e /
 *              sigma)) in fp32 and summed in fp64: compute_mmd with beta = 1/R
 *              against the Dirac at 0, at each bandwidth sigma[k][s]
 *   costs      [num_cfg][3][R] the per-rollout costs, or NULL (not copied)
 *   elapsed_ms [3] HIP-event times of the rollout, statistics and MMD stages,
 *              or NULL
 * Nothing accumulates through floating-point atomics: a call repeated returns
 * the same bits, and a configuration's results do not depend on the batch.
 *
 * Limits: 1 <= num_obs <= 32, 2 <= num_prime <= 100, 1 <= num_rollouts <= 2^20,
 * num_cfg <= 65535, 0 <= alpha <= 1, 0 <= num_sigma <= 8, every sigma finite
 * and > 0: anything else is MPCMMD_E_INVALID before any HIP call.  A CARLA
 * variant is MPCMMD_E_UNSUPPORTED; num_cfg == 0 returns MPCMMD_OK without
 * touching a device.  Synchronous, needs no handle, allocates its own device
 * buffers. */
typedef struct mpcmmd_validate_risk_args {
  int32_t num_cfg, num_obs, num_prime, num_rollouts;
  int32_t noise;            /* MPCMMD_NOISE_* */
  int32_t variant;          /* MPCMMD_VARIANT_STATIC / _DYNAMIC */
  double noise_level, acc_const_noise, steer_const_noise;
  uint32_t seed;
  int32_t device;
  const double* cx;         /* [num_cfg][11] */
  const double* cy;
  const double* init_state; /* [num_cfg][6] */
  const float* x_obs;       /* [num_cfg][num_obs][100] */
  const float* y_obs;
  const double* draws;      /* [num_cfg][3][R][H] or NULL */
  const uint32_t* keys;     /* [num_cfg] */
  float alpha;              /* quantile level (the optimizer's alpha_quant = 0.98) */
  int32_t num_sigma;
  const float* sigma;       /* [num_cfg][num_sigma] */
  const float* costs_in;    /* [num_cfg][3][R] or NULL */
  int32_t* count_pos;       /* [num_cfg][3] out */
  float* var;               /* [num_cfg][3] out */
  float* cvar;              /* [num_cfg][3] out */
  float* mean;              /* [num_cfg][3] out */
  float* max;               /* [num_cfg][3] out */
  float* mmd;               /* [num_cfg][3][num_sigma] out */
  float* costs;             /* [num_cfg][3][R] out, or NULL */
  float* elapsed_ms;        /* [3] out, or NULL */
} mpcmmd_validate_risk_args;
int mpcmmd_validate_risk(const mpcmmd_validate_risk_args* args);

/* Monte-Carlo risk statistics of CARLA plans on the GPU: the statistics of
 * mpcmmd_validate_risk on the rollouts of mpcmmd_validate_carla.  ABI version
 * unchanged; detect the entry point by its symbol.
 *
 * The rollouts are mpcmmd_validate_carla's, unchanged: the plan controls, the
 * noisy initial rows, the noise model, the Philox streams 32..39 with the same
 * element indices, the recorded point at h (the state before step h) and the
 * closest-point Frenet transform.  The same (inputs, keys, seed, draws,
 * init_eps) roll the same points in both calls, and one pass over them forms
 * the counts and the costs.
 *
 * Per tick k and rollout r three fp32 channels over the H recorded points
 * (carla/optimizer/costs.py:48-68, 117-211), (s, d) the point's Frenet
 * coordinates:
 *   obs[r]     = max over (o, h) of max(0, f), f = f_bar(s, d, x_obs[o][h],
 *                y_obs[o][h]) with a^2, b^2: the value whose sign the counts of
 *                mpcmmd_validate_carla test
 *   lane_lb[r] = max over h of max(0, -d + y_lb)
 *   lane_ub[r] = max over h of max(0,  d - y_ub)
 * One term t contributes t if t > 0, +0 if t <= 0 and NaN if t is NaN; a row's
 * cost is NaN if any of its terms is (jnp.maximum and jnp.max propagate NaN),
 * stored as the one quiet NaN 0x7fc00000.  Hence !(cost <= 0) <=> some term
 * !(t <= 0), and count_pos[k][0] == count_rows[k] exactly.
 *
 * The statistics are mpcmmd_validate_risk's, definition for definition
 * (count_pos, var, cvar, mean, max [num_cfg][3], mmd [num_cfg][3][num_sigma];
 * the same kernels on the device cost buffer, mpcmmd_quantile_position's
 * ranks).  costs [num_cfg][3][R] and the counts of mpcmmd_validate_carla
 * (count, count_lane, count_rows [num_cfg], count_oh [num_cfg][O][H]) are
 * optional outputs: NULL is not copied.  elapsed_ms [3], or NULL: HIP-event
 * times of the rollouts with costs and counts, the statistics and the MMD.
 * Nothing accumulates through floating-point atomics (the row maxima are
 * integer maxima of ordered keys): a value depends on (k, r) only, a call
 * repeated returns the same bits, and a tick returns in a batch the bits it
 * returns alone.
 *
 * Out of scope: the desired-lane term (compute_lane_des_*), a single Frobenius
 * norm over the whole sample set and not a per-rollout cost.
 *
 * Limits: those of mpcmmd_validate_carla, and num_rollouts <= 2^20, 0 <= alpha
 * <= 1, 0 <= num_sigma <= 8, every sigma finite and > 0.  Anything else, a
 * NULL required argument or a static / dynamic variant (mpcmmd_validate_risk's)
 * is MPCMMD_E_INVALID before any HIP call; num_cfg == 0 returns MPCMMD_OK
 * without touching a device.  A shape whose workgroup does not fit the
 * device's LDS is MPCMMD_E_UNSUPPORTED (never on an MI355X: the largest shape
 * needs 768 B more than mpcmmd_validate_carla's, under 131 KiB).  Synchronous,
 * needs no handle, allocates its own device buffers. */
typedef struct mpcmmd_validate_carla_risk_args {
  int32_t num_cfg, num_obs, num_prime, num_rollouts, num_path;
  int32_t noise;            /* MPCMMD_NOISE_* */
  int32_t variant;          /* MPCMMD_VARIANT_CARLA_* (y_lb, y_ub) */
  float noise_level, acc_const_noise, steer_const_noise;
  uint32_t seed;
  int32_t device;
  const float* init_state;  /* [num_cfg][6] init_state_global */
  const float* v;           /* [num_cfg][100] v_best */
  const float* steer;       /* [num_cfg][100] steering_best */
  const float* x_obs;       /* [num_cfg][num_obs][100] Frenet tracks */
  const float* y_obs;
  const float* path;        /* [num_cfg][6][num_path] */
  const float* draws;       /* [num_cfg][3][R][H] or NULL */
  const float* init_eps;    /* [num_cfg][R][4] or NULL */
  const uint32_t* keys;     /* [num_cfg] */
  float alpha;              /* quantile level (the optimizer's alpha_quant = 0.98) */
  int32_t num_sigma;
  const float* sigma;       /* [num_cfg][num_sigma] */
  int32_t* count_pos;       /* [num_cfg][3] out */
  float* var;               /* [num_cfg][3] out */
  float* cvar;              /* [num_cfg][3] out */
  float* mean;              /* [num_cfg][3] out */
  float* max;               /* [num_cfg][3] out */
  float* mmd;               /* [num_cfg][3][num_sigma] out */
  float* costs;             /* [num_cfg][3][R] out, or NULL */
  int32_t* count;           /* [num_cfg] out, or NULL */
  int32_t* count_lane;      /* [num_cfg] out, or NULL */
  int32_t* count_rows;      /* [num_cfg] out, or NULL */
  int32_t* count_oh;        /* [num_cfg][num_obs][num_prime] out, or NULL */
  float* elapsed_ms;        /* [3] out, or NULL */
} mpcmmd_validate_carla_risk_args;
int mpcmmd_validate_carla_risk(const mpcmmd_validate_carla_risk_args* args);

/* The linear quantile's position among n >= 1 ascending samples, 0 <= alpha <=
 * 1 (else MPCMMD_E_INVALID): indices lo, hi and fp32 weights w_lo, w_hi of
 * quantile = v[lo] w_lo + v[hi] w_hi.  Host only, no GPU needed. */
int mpcmmd_quantile_position(int32_t n, float alpha, int32_t* lo, int32_t* hi, float* w_lo, float* w_hi);

/* ---- Surrogate world of a closed CARLA loop ----------------------------------
 * One step of the world model of DESIGN.md section 19 (a model of this
 * library's, not CARLA physics): from the plan of tick k (cx, cy and the first
 * four steerings of a CARLA result) to the raw inputs of tick k + 1 as
 * mpcmmd_tick_inputs carries them, plus the first population of that tick's
 * CEM and one log row.  Controller (main_carla.py:408-413), perturbation
 * (:415-436) from four given variates, bicycle step (compute_rollout_one_step
 * with the world's dt), constant-velocity vehicles, the flags, the waypoints
 * (waypoint_generator) and the nearest obstacles (compute_obs_data).  fp32 in
 * the order DESIGN.md states, transcendentals evaluated in fp64 and rounded
 * once, positions, distances and the spline in fp64.
 *
 * The variates u[4] are given, or drawn where the controls are known (u NULL):
 * Philox streams keyed (episode key, seed) at stream ids 40..44 (csrc/rng.hpp),
 * element = tick.  gaussian: u0, u2, u3 = normals 0, 2, 3 of block `tick` of
 * stream 40.  beta: u0 ~ Beta(2|a_c|, 5|a_c|) (streams 41, 42), u1 ~
 * Beta(2|s_c|, 5|s_c|) (43, 44) by the validators' fp64 sampler, with its
 * |control| = 0 limit rule (DESIGN.md Numerics), rounded once; u2, u3 as above.
 * The log row holds the variates used.
 *
 * mpcmmd_world_step_host steps one episode on the host (no GPU needed).
 * mpcmmd_world_step_device steps n_episodes independent episodes with one
 * launch of k_world_step (one workgroup per episode, k_world.hip) on device
 * `device`, every array with a leading episode axis; each episode's outputs
 * are bit-equal to the host step's (tests/test_gpu_world.py).  It uploads and
 * reads back every array, so it is the kernel's reference harness, not a fast
 * path: that is the world context below.  ABI version unchanged: detect the
 * entry points by their symbols.
 *
 * Before any HIP call: MPCMMD_E_INVALID for a NULL argument or array,
 * num_path outside 2..2048, num_obs outside 1..64, total_obs outside 0..64,
 * num_route < 2, goal_index outside 0..num_route-1, num_batch < 1, a noise
 * other than 0 / 1, n_episodes < 1. */
typedef struct mpcmmd_world_model {
  int32_t num_path;   /* waypoints per tick */
  int32_t num_obs;    /* obstacles the optimizer sees */
  int32_t total_obs;  /* vehicles in the world, 0..64 */
  int32_t num_route;  /* points of the (extended) route */
  int32_t goal_index; /* route point whose 7 m neighbourhood is the goal (len_path - 1, main_carla.py:329) */
  int32_t num_batch;  /* rows of the first population */
  int32_t noise;      /* 0 gaussian, 1 beta (u[0], u[1] are then Beta variates) */
  float dt;           /* tick length (replay: 0.05) */
  float sigma_acc, sigma_steer, acc_const, steer_const; /* the driver's noise model */
  float steer_max;    /* 0.6 */
  float a_obs, b_obs; /* half axes of the keep-out ellipse (4.5, 3) */
  float y_lb, y_ub;   /* lane bounds of the signed lateral offset */
  const double* route_x;   /* [num_route] */
  const double* route_y;
  const double* route_arc; /* [num_route] the splines' breakpoints, strictly increasing */
  const double* spline_x;  /* [4][num_route-1]: scipy CubicSpline(route_arc, route_x).c */
  const double* spline_y;
  const double* pdot4;     /* [4][11]: rows 0..3 of Pdot (mpcmmd_host_constant) */
  const double* chol;      /* [8][8] lower Cholesky factor of the run's covariance, row-major */
  const float* pop0;       /* [num_batch][8] standard normals of the first population */
  uint32_t seed;           /* key word 1 of the drawn variates' Philox streams (the world context: the handle's) */
} mpcmmd_world_model;

#define MPCMMD_WORLD_LOG_D 3  /* x, y (global, after the step), arc of the closest route point */
#define MPCMMD_WORLD_LOG_F 13 /* v, psi, psidot, a_c, s_c, a, s, u[4], clear, d */
#define MPCMMD_WORLD_LOG_I 4  /* idx, lane_out, collided, goal */

typedef struct mpcmmd_world_step_io { /* leading axis n_episodes for the device step */
  /* the plan and the variates of this tick */
  const float* cx;    /* [11] */
  const float* cy;    /* [11] */
  const float* steer; /* [4] the plan's first four steerings */
  const float* u;     /* [4] the variates, or NULL: drawn from (key, seed, tick) once a_c and s_c are known */
  const float* mean;  /* [8] mean_param as the solve left it */
  /* the episode's state, updated in place unless it is frozen */
  double* pos;        /* [2] global x, y */
  float* ego;         /* [3] v, psi, psidot */
  float* vehicles;    /* [total_obs][5] x, y, vx, vy, psi */
  int32_t* done_tick; /* [1] -1 while the episode runs; the tick that set collided or goal */
  /* the next tick */
  float* init_state;  /* [6] */
  float* x_wp;        /* [num_path] */
  float* y_wp;
  float* obstacles;   /* [num_obs][5] */
  float* pop;         /* [num_batch][8] */
  /* the log row */
  double* log_d;      /* [MPCMMD_WORLD_LOG_D] */
  float* log_f;       /* [MPCMMD_WORLD_LOG_F] */
  int32_t* log_i;     /* [MPCMMD_WORLD_LOG_I] */
  const uint32_t* key; /* [1] the episode's key; needed when u is NULL */
} mpcmmd_world_step_io;

int mpcmmd_world_step_host(const mpcmmd_world_model* m, int32_t tick, const mpcmmd_world_step_io* io);
int mpcmmd_world_step_device(const mpcmmd_world_model* m, int32_t device, int32_t n_episodes, int32_t tick,
                             const mpcmmd_world_step_io* io);

/* Routed vehicles (csrc/world_vehicle.hpp): instead of
 * moving at constant velocity, vehicle j follows the route's splines at a
 * constant signed lateral offset d (left positive, the sign of log_f's d) with
 * the state s (fp64 arc length) and v (fp32 speed >= 0), and accelerates by the
 * intelligent-driver car-following model towards its target speed v0 behind its
 * leader: the nearest of the other vehicles and the ego (after its move: arc of
 * its closest route point, its lateral offset, its new speed) with |d_k - d_j|
 * < lane_tol and s_k > s_j, gap = (s_k - s_j) - length; equal gaps: the lowest
 * vehicle index, the ego last.  Every s read is the value before the step.
 *   a  = clip(acc_max (1 - (v/v0)^4 - (ss / max(gap, gap_min))^2), acc_min, acc_max),
 *   ss = gap0 + max(0, v headway + v (v - v_lead) / (2 sqrt(acc_max brake)))
 * (no leader: the last term is 0), v' = max(v + a dt, 0), s' = s + v' dt.  A
 * vehicle with !(v0 > 0) is parked (v' = 0, s' = s).  A live episode's step
 * advances (s, v); every step, frozen ones included, writes the vehicles' rows
 * (x, y, vx, vy, psi) from (s, d, v) into io->vehicles -- whose contents on
 * entry are not read -- and the rest of the step reads those rows as before.
 * All in fp64 in this order, rounded once; every NaN is stored as the quiet NaN.
 * A model of this library's, not CARLA's traffic manager.
 *
 * mpcmmd_world_step_host_routed / _device_routed are mpcmmd_world_step_host /
 * _device with that policy; the kernel is the routed instantiation of
 * k_world_step and equals the host step in every word
 * (tests/test_gpu_world_vehicles.py).  tick < 0 is the reset-mode step of the
 * chained route: no plan is read (cx, cy, steer, u may hold anything), nothing
 * moves, done_tick and the log rows are not written; it makes tick 0's inputs
 * and the vehicles' rows from the start states.
 *
 * Before any HIP call, beyond the plain step's errors: MPCMMD_E_INVALID for a
 * NULL rt, a NULL veh_s, veh_v or veh_param when total_obs > 0, or scalars
 * that break acc_max > 0, brake > 0, gap_min > 0, acc_min < 0, lane_tol >= 0. */
typedef struct mpcmmd_world_routed { /* leading axis n_episodes for the device step */
  double* veh_s;          /* [total_obs] updated in place unless frozen */
  float* veh_v;           /* [total_obs] likewise */
  const float* veh_param; /* [total_obs][2] d, v0 */
  float* veh_log;         /* [total_obs][2] v after this step and the acceleration applied (0: parked, frozen), or
                             NULL; s after the step is veh_s itself, in fp64; not written when tick < 0 */
  float acc_max, brake, gap0, headway, length, lane_tol, gap_min, acc_min;
} mpcmmd_world_routed;
int mpcmmd_world_step_host_routed(const mpcmmd_world_model* m, int32_t tick, const mpcmmd_world_step_io* io,
                                  const mpcmmd_world_routed* rt);
int mpcmmd_world_step_device_routed(const mpcmmd_world_model* m, int32_t device, int32_t n_episodes, int32_t tick,
                                    const mpcmmd_world_step_io* io, const mpcmmd_world_routed* rt);

/* The chained route: E <= max_configs closed-loop episodes on a tick context's
 * handle with nothing crossing the host between two solves.  A world context
 * belongs to one tick context (its num_path and its handle's num_obs must be
 * the model's; num_batch, chol and pop0 of the model are not read: the
 * population is the handle's, from its own pop0 normals and the Cholesky
 * factor of the covariance given at reset).  It owns its device memory (route,
 * spline pieces, the episodes' state, the variates, the log); none of it is in
 * the handle's buffer list.  Destroy it before its tick context.
 *
 * mpcmmd_world_reset uploads the episodes' start states (pos [E][2], ego
 * [E][3] = v, psi, psidot, vehicles [E][total_obs][5]), their means [E][8]
 * (into the handle's mean), the run's covariance [64] (factored on the host as
 * initial_population factors it), the episodes' keys [E] and the variates u
 * [max_ticks][E][4] -- or u NULL: k_world_step then draws each tick's variates
 * itself from (keys[e], the handle's seed, tick), after that tick's solve, which
 * is what Beta noise needs (its parameters are the controls) -- and
 * enqueues one k_world_step in reset mode, which writes tick 0's raw inputs
 * into the tick context's input image, the handle's st0 and iteration 0's
 * population from the start states.  Episode e solves tick k with idx_mpc =
 * k + keys[e].
 *
 * mpcmmd_world_run enqueues, for each tick of [tick_begin, tick_begin +
 * count): the chained begin (begin_impl through the tick route with the raw
 * inputs, st0, the population and the mean already on the device: idx_mpc,
 * v_des [E], cov and the init_eps normals are still staged), the T CEM
 * iterations, and k_world_step, which reads the plan from the handle's result
 * buffers (results, res_steer, mean) and writes the next tick's inputs where
 * the next begin finds them.  No device-to-host copy and no stream
 * synchronisation inside the loop beyond the staging-event waits every begin
 * makes; begin k + 1 waits for begin k's staging event, which lies behind tick
 * k - 1's solve and step in the stream, so the host runs at most about one
 * tick ahead of the device.  Ticks run in order; a run may be split (run(0, 3) then run(3, 3)).
 * After a run the handle holds the last tick's solve (mpcmmd_finish_batch,
 * mpcmmd_read(h, "path")).
 *
 * mpcmmd_world_log synchronises and reads back the first `ticks` rows: log_d
 * [ticks][E][3], log_f [ticks][E][13], log_i [ticks][E][4], plan
 * [ticks][E][34] (cx, cy, the first four steerings and mean_param of the solve
 * the step consumed) and done_tick [E].  Every row equals the host-stepped
 * loop's (mpcmmd_carla_tick_solve_batch + mpcmmd_world_step_host) bit for bit
 * (tests/test_gpu_closed_loop.py).
 *
 * Before any HIP call: MPCMMD_E_INVALID for NULL arguments, a model out of
 * range or not matching the tick context, n_episodes outside 1..max_configs,
 * a covariance that is not positive definite, a tick range outside
 * [0, max_ticks]; MPCMMD_E_STATE for a run before a reset; then the tick
 * begin's own errors. */
typedef struct mpcmmd_world mpcmmd_world;
int mpcmmd_world_create(mpcmmd_tick* t, const mpcmmd_world_model* m, int32_t max_ticks, mpcmmd_world** out);
void mpcmmd_world_destroy(mpcmmd_world* w);
int mpcmmd_world_reset(mpcmmd_world* w, int32_t n_episodes, const double* pos, const float* ego,
                       const float* vehicles, const float* mean, const float* cov, const float* u,
                       const int32_t* keys);
int mpcmmd_world_run(mpcmmd_world* w, int32_t cost_kind, int32_t tick_begin, int32_t count, const float* cov,
                     const float* v_des, float threshold);
int mpcmmd_world_log(mpcmmd_world* w, int32_t ticks, double* log_d, float* log_f, int32_t* log_i, float* plan,
                     int32_t* done_tick);

/* Routed vehicles on the chained route (the policy of mpcmmd_world_routed
 * above; no ABI version change: detect the entry points by their symbols).
 *
 * mpcmmd_world_route_vehicles stages the start states veh_s, veh_v
 * [n_episodes][total_obs], the parameters veh_param [n_episodes][total_obs][2]
 * = d, v0 and the eight scalars (acc_max, brake, gap0, headway, length,
 * lane_tol, gap_min, acc_min, in this order) in the world context, allocates
 * the states and a vehicle log [max_ticks][max_configs][total_obs] there (none
 * of it in the handle's buffer list) and synchronises.  It takes effect at the
 * next mpcmmd_world_reset, which must be given the same n_episodes
 * (MPCMMD_E_INVALID otherwise) and whose `vehicles` argument is then ignored
 * and may be NULL: the reset-mode step makes tick 0's rows from (s, v, d).
 * Every reset starts from the staged states again.  A run before that reset is
 * MPCMMD_E_STATE.  NULL arrays (all three) turn the policy off and free its
 * memory.  With the policy on the reset-mode step and every tick's step are
 * the routed kernel; the loop gains no readback, synchronisation or
 * allocation, and the validation stage reads whatever rows the step wrote.
 *
 * mpcmmd_world_vehicle_log synchronises and reads back the first `ticks` rows:
 * veh_s [ticks][E][total_obs] (fp64) and veh_va [ticks][E][total_obs][2] = v
 * and the acceleration applied, every vehicle's state after each tick's step;
 * MPCMMD_E_STATE with the policy off.  Every word equals the host-stepped
 * loop's (tests/test_gpu_closed_loop_vehicles.py).
 *
 * Before any HIP call: MPCMMD_E_INVALID for a NULL w, some but not all arrays
 * NULL, NULL scalars with arrays given, n_episodes outside 1..max_configs, the
 * scalars' rules of mpcmmd_world_routed, a tick range outside [0, max_ticks]. */
int mpcmmd_world_route_vehicles(mpcmmd_world* w, int32_t n_episodes, const double* veh_s, const float* veh_v,
                                const float* veh_param, const float* scalars);
int mpcmmd_world_vehicle_log(mpcmmd_world* w, int32_t ticks, double* veh_s, float* veh_va);

/* The validation stage of the chained route: the Monte-Carlo risk of every
 * tick's plan, computed inside the loop from the device buffers the solve just
 * used.  (No ABI version change: callers detect these entry points by their
 * symbols.)
 *
 * mpcmmd_world_validate configures the stage (cfg NULL: turns it off) and
 * allocates everything it needs -- the costs [E][3][R], the MMD scratch, the
 * counters, the packed inputs and the logs [max_ticks][E]... -- so a run
 * allocates nothing.  It synchronises the handle's stream, and it takes effect
 * at the next mpcmmd_world_reset: a run before that reset is MPCMMD_E_STATE.
 *
 * With the stage on, mpcmmd_world_run enqueues per tick, in this order: the
 * chained begin, the T CEM iterations, the validation stage, k_world_step (the
 * step overwrites the tick's init_state and st0, so the stage comes first).
 * The stage is k_world_validate_prep, which packs the validators' inputs on
 * the device, two hipMemsetAsync of the integer accumulators, and then the
 * launches of mpcmmd_validate_carla_risk unchanged, with their results pointed
 * at the tick's log row.  No device-to-host copy, no synchronisation and no
 * allocation is added to the loop, and the solve and the world's log are what
 * they are without the stage.
 *
 * The log row of (tick k, episode e) is, bit for bit, what
 * mpcmmd_validate_carla_risk returns for num_cfg = 1 with: init_state the
 * tick's raw init_state; v, steer the solve's v_best and steering as
 * mpcmmd_finish_batch returns them; x_obs, y_obs the handle's obs buffer
 * (columns >= num_prime zero: the validator reads h < num_prime only); path the
 * first num_path columns of the handle's path; noise, noise_level,
 * acc_const_noise, steer_const_noise, variant, seed, num_prime, num_obs the
 * handle's configuration; num_path the tick context's; keys[0] = uint32(k +
 * keys[e]), the tick's idx_mpc; draws, init_eps NULL; alpha, sigma from cfg.
 * The validators' Philox streams are their own, so the rows are independent
 * of the solve's draws under the same key.  Frozen episodes are validated like
 * the others (their frozen state and its plan).
 *
 * mpcmmd_world_validation_log synchronises and reads back the first `ticks`
 * rows: counts [ticks][E][3] = count, count_lane, count_rows of
 * mpcmmd_validate_carla; count_pos [ticks][E][3] per channel (obs, lane_lb,
 * lane_ub); stats [ticks][E][4][3] = var, cvar, mean, max per channel; mmd
 * [ticks][E][3][num_sigma] (may be NULL when num_sigma == 0); est
 * [ticks][E][2] = the cost_lane and cost_obs the solve itself estimated
 * (mpcmmd_result).  mpcmmd_world_validation_inputs synchronises and reads back
 * the packed inputs of the last validated tick (debugging and tests): acc,
 * steer [E][num_prime], st0 [E][8], path [E][6][num_path], x_obs, y_obs
 * [E][num_obs][100], keys [E]; a NULL array is skipped.
 *
 * Before any HIP call: MPCMMD_E_INVALID for a NULL w, num_rollouts outside
 * 1..2^20 or num_rollouts * num_prime >= 2^31, alpha outside [0, 1],
 * num_sigma outside 0..8, a sigma that is not finite and > 0, a handle with
 * num_obs > 32 (the validator's limit), a NULL required log array, a tick
 * range outside [0, max_ticks]; MPCMMD_E_STATE for a log or inputs readback
 * while the stage is off.  MPCMMD_E_UNSUPPORTED if the validator's workgroup
 * needs more LDS than the device has. */
typedef struct mpcmmd_world_validation {
  int32_t num_rollouts; /* R: fresh noise rows per (tick, episode) */
  float alpha;          /* quantile level of VaR / CVaR */
  int32_t num_sigma;    /* S, 0..8 */
  float sigma[8];       /* MMD bandwidths, the same for every episode and tick */
} mpcmmd_world_validation;
int mpcmmd_world_validate(mpcmmd_world* w, const mpcmmd_world_validation* cfg);
int mpcmmd_world_validation_log(mpcmmd_world* w, int32_t ticks, int32_t* counts, int32_t* count_pos, float* stats,
                                float* mmd, float* est);
int mpcmmd_world_validation_inputs(mpcmmd_world* w, float* acc, float* steer, float* st0, float* path, float* x_obs,
                                   float* y_obs, uint32_t* keys);

/* ---- Receding-horizon episodes of the synthetic variants -----------------------
 * The closed loop of a MPCMMD_VARIANT_STATIC / _DYNAMIC handle (DESIGN.md
 * section 21): solve, apply the plan's first control under the noise model,
 * re-solve from where the ego ended up, warm-started from the previous mean.
 * The world is the optimizer's own rollout model with one realised draw (a
 * model of this library's: the reference has no synthetic loop):
 *   controller   compute_controls at step 0: a_c = (v_1 - v_0) / 0.15, s_c =
 *                atan(2.5 curv), curv = (ydd_0 xd_0 - yd_0 xdd_0) / (s2 sqrt(s2))
 *   perturbation the optimizer's noisy_from on one draw u[3]
 *   ego          bicycle_step_cr_t's expression, wheel base 2.5, the model's dt,
 *                no speed clamp; position in fp64
 *   vehicles     num_obs rows (x, y, vx, vy), constant velocity, all seen by
 *                the optimizer; tracks x + vx tt on np.linspace(0, 15, 100)
 *   flags        clear = max_o (1 - (dx/a)^2 - (dy/b)^2) (-inf without
 *                vehicles), collided = !(clear <= 0), lane_out = y < y_lb | y >
 *                y_ub, goal = x >= goal_x; a collided or goal episode is
 *                frozen: done_tick is set, the state stops, the slot keeps
 *                being solved on the frozen state (with zero acceleration)
 * fp32 in the order DESIGN.md states, transcendentals in fp64 rounded once;
 * every NaN a subtraction may form is stored as 0x7FC00000.
 *
 * The variates u[3] are given, or drawn where the controls are known (u NULL):
 * Philox streams keyed (episode key, seed) at stream ids 45..49 (csrc/rng.hpp),
 * element = tick.  u0, u1, u2 = normals 0, 1, 2 of block `tick` of stream 45.
 * beta: u0 ~ Beta(2|a_c|, 5|a_c|) (streams 46, 47), u1 ~ Beta(2|s_c|, 5|s_c|)
 * (48, 49) by the validators' fp64 sampler with its |control| = 0 limit rule,
 * rounded once -- the optimizer's beta_pair parameters.  The log row holds the
 * variates used.
 *
 * mpcmmd_mpc_step_host steps one episode on the host (no GPU needed).
 * mpcmmd_mpc_step_device steps n_episodes (1..65535) independent episodes with
 * one launch of k_mpc_step (one workgroup per episode, k_mpc.hip) on device
 * `device`, every array with a leading episode axis; each word it writes is the
 * host step's (tests/test_gpu_mpc_step.py).  It uploads and reads back every
 * array: the kernel's reference harness, not a fast path.  ABI version
 * unchanged: detect the entry points by their symbols.
 *
 * Before any HIP call: MPCMMD_E_INVALID for a NULL argument or array, num_obs
 * outside 0..64, num_batch < 1, a noise other than 0 / 1, dt, a_obs or b_obs
 * not > 0, n_episodes out of range. */
typedef struct mpcmmd_mpc_model {
  int32_t num_obs;   /* vehicles, 0..64 (the context: the handle's num_obs) */
  int32_t num_batch; /* rows of the first population */
  int32_t noise;     /* 0 gaussian, 1 beta (u[0], u[1] are then Beta variates) */
  float dt;          /* tick length (0.15: the rollout step) */
  float sigma_acc, sigma_steer, acc_const, steer_const; /* the noise model's scalars */
  float K_steer;     /* float32(K_steer * sigma_steer), as the optimizer holds it (beta noise) */
  float a_obs, b_obs; /* half axes of the keep-out ellipse (4.25, 2.75) */
  float y_lb, y_ub;  /* lane bounds of y */
  float goal_x;      /* the episode ends at x >= goal_x */
  const double* pdot2;  /* [2][11]: rows 0, 1 of Pdot (mpcmmd_host_constant) */
  const double* pddot1; /* [11]: row 0 of Pddot */
  const double* chol;   /* [8][8] lower Cholesky factor of the run's covariance, row-major */
  const float* pop0;    /* [num_batch][8] standard normals of the first population */
  uint32_t seed;        /* key word 1 of the drawn variates' Philox streams (the context: the handle's) */
} mpcmmd_mpc_model;

#define MPCMMD_MPC_LOG_D 2  /* x, y after the step */
#define MPCMMD_MPC_LOG_F 12 /* vx, vy, psi, a_c, s_c, a, s, u[3], clear, curv */
#define MPCMMD_MPC_LOG_I 4  /* lane_out, collided, goal, frozen (the step found the episode done) */

typedef struct mpcmmd_mpc_step_io { /* leading axis n_episodes for the device step */
  /* the plan and the variates of this tick */
  const float* cx;   /* [11] */
  const float* cy;   /* [11] */
  const float* u;    /* [3] the variates, or NULL: drawn from (key, seed, tick) once a_c and s_c are known */
  const float* mean; /* [8] the CEM mean as the solve left it */
  /* the episode's state, updated in place unless it is frozen */
  double* pos;        /* [2] x, y */
  float* vel;         /* [3] vx, vy, psi */
  float* vehicles;    /* [num_obs][4] x, y, vx, vy */
  int32_t* done_tick; /* [1] -1 while the episode runs; the tick that set collided or goal */
  /* the next tick */
  float* init_state; /* [6] float(x), float(y), vx, vy, ax, ay */
  float* x_obs;      /* [num_obs][100] */
  float* y_obs;
  float* pop;        /* [num_batch][8] */
  float* st0;        /* [8] the rollouts' initial state of that init_state (the handle's st0 buffer) */
  /* the log row */
  double* log_d;  /* [MPCMMD_MPC_LOG_D] */
  float* log_f;   /* [MPCMMD_MPC_LOG_F] */
  int32_t* log_i; /* [MPCMMD_MPC_LOG_I] */
  const uint32_t* key; /* [1] the episode's key; needed when u is NULL */
} mpcmmd_mpc_step_io;

int mpcmmd_mpc_step_host(const mpcmmd_mpc_model* m, int32_t tick, const mpcmmd_mpc_step_io* io);
/* The standard normals [cfg->num_batch][8] a handle of cfg draws for its first population (fixed
 * key, cfg->seed): the pop0 of a model that steps that handle's loop on the host.  Host only. */
int mpcmmd_mpc_first_normals(const mpcmmd_config* cfg, float* out);
int mpcmmd_mpc_step_device(const mpcmmd_mpc_model* m, int32_t device, int32_t n_episodes, int32_t tick,
                           const mpcmmd_mpc_step_io* io);

/* The chained route: E <= max_configs episodes on a static / dynamic handle
 * with nothing crossing the host between two solves.  The context owns its
 * device memory (the episodes' state, the variates, the log, the KKT columns);
 * num_batch, chol, pop0 and seed of the model are not read: the population is
 * the handle's, from its own pop0 normals and the Cholesky factor of the
 * covariance given at reset, the seed the handle's.  Destroy it before its
 * handle.
 *
 * mpcmmd_mpc_reset (synchronous) uploads the start states (pos [E][2], vel
 * [E][3], vehicles [E][num_obs][4]), the means [E][8] (into the handle's
 * mean), the covariance [64] (factored on the host as initial_population
 * factors it), the keys [E] and the variates u [max_ticks][E][3] -- or u NULL:
 * k_mpc_step draws them -- and runs k_mpc_step once in reset mode (every
 * episode as if frozen, no controller, no log row), which writes tick 0's
 * st0, solve_c, obs and first population into the handle's buffers.
 *
 * mpcmmd_mpc_run enqueues, per tick of [tick_begin, tick_begin + count): the
 * chained begin (only idx_mpc, v_des [E] and cov are staged; the lam / s_lane
 * memsets), the T CEM iterations and k_mpc_step, which reads the plan from the
 * handle's results of the last iteration and writes the next solve's buffers;
 * mean stays where k_select left it: the warm start.  Episode e solves tick k
 * with idx_mpc = k + keys[e].  No device-to-host copy and no synchronisation
 * beyond the staging-event wait every begin makes.  Ticks run in order; a run
 * may be split.
 *
 * mpcmmd_mpc_log synchronises and reads back the first `ticks` rows: log_d
 * [ticks][E][2], log_f [ticks][E][12], log_i [ticks][E][4], plan
 * [ticks][E][30] (cx, cy and mean of the solve the step consumed) and
 * done_tick [E].  Every row equals the host-stepped loop's (mpcmmd_solve_batch
 * + mpcmmd_mpc_step_host) bit for bit (tests/test_gpu_mpc_loop.py).
 *
 * Before any HIP call: MPCMMD_E_INVALID for a NULL argument, a CARLA handle, a
 * model out of range or whose num_obs is not the handle's, n_episodes outside
 * 1..max_configs, a covariance that is not positive definite, a tick range
 * outside [0, max_ticks]; MPCMMD_E_STATE for a run before a reset;
 * MPCMMD_E_UNSUPPORTED for mmd_opt on a handle without it. */
typedef struct mpcmmd_mpc mpcmmd_mpc;
int mpcmmd_mpc_create(mpcmmd_handle* h, const mpcmmd_mpc_model* m, int32_t max_ticks, mpcmmd_mpc** out);
void mpcmmd_mpc_destroy(mpcmmd_mpc* c);
int mpcmmd_mpc_reset(mpcmmd_mpc* c, int32_t n_episodes, const double* pos, const float* vel, const float* vehicles,
                     const float* mean, const float* cov, const float* u, const int32_t* keys);
int mpcmmd_mpc_run(mpcmmd_mpc* c, int32_t cost_kind, int32_t tick_begin, int32_t count, const float* cov,
                   const float* v_des);
int mpcmmd_mpc_log(mpcmmd_mpc* c, int32_t ticks, double* log_d, float* log_f, int32_t* log_i, float* plan,
                   int32_t* done_tick);

/* The validation stage of the synthetic chained route:
 * the Monte-Carlo risk of every tick's plan, computed inside the loop from the
 * device buffers the solve just used.  (No ABI version change: callers detect
 * these entry points by their symbols.)
 *
 * mpcmmd_mpc_validate configures the stage (cfg NULL: turns it off) and
 * allocates everything it needs into the context -- the costs [E][3][R], the
 * MMD scratch, the packed inputs, the fp32 Pdot / Pddot images, the logs
 * [max_ticks][E]..., one side stream and two events -- so a run allocates
 * nothing.  It synchronises the handle's stream (and the side stream of a stage
 * it replaces), and it takes effect at the next mpcmmd_mpc_reset: a run before
 * that reset is MPCMMD_E_STATE.
 *
 * With the stage on, mpcmmd_mpc_run enqueues per tick, in this order: the
 * resident begin, the T CEM iterations, the stage, k_mpc_step.  The stage is
 * k_mpc_validate_prep, which packs the validators' inputs on the device (always
 * on the handle's stream and before the step: the step overwrites the state and
 * the tracks, the next solve the results), and then the launches of
 * mpcmmd_validate and mpcmmd_validate_risk unchanged (k_validate, k_vrisk_roll,
 * the statistics, the MMD) with their results pointed at the tick's log row.
 * overlap = 0 puts those launches behind the prep on the handle's stream.
 * overlap = 1 records an event behind the prep, has the context's side stream
 * wait for it and run the launches there, while the handle's stream goes
 * straight on to k_mpc_step and the next tick; the next tick's prep first waits
 * for the side stream's completion event of the previous tick (the packed
 * inputs, the costs and the scratch are single buffers).  Plain streams and
 * events: nothing is captured into a graph.  mpcmmd_mpc_validation_log,
 * mpcmmd_mpc_validation_inputs, mpcmmd_mpc_log, mpcmmd_mpc_reset,
 * mpcmmd_mpc_destroy and turning the stage off synchronise both streams.  No
 * device-to-host copy, no host synchronisation and no allocation is added to the
 * loop, and the solve and the loop's log are what they are without the stage.
 *
 * The log row of (tick k, episode e) is, bit for bit, what mpcmmd_validate and
 * mpcmmd_validate_risk return for num_cfg = 1 with: cx, cy the solve's fp32 cx,
 * cy widened to fp64; init_state the fp32 (float(x), float(y), vx, vy, ax, ay)
 * the host-stepped loop hands mpcmmd_solve_batch for that tick, widened (the
 * validators read words 0..3: the stage packs 0 into words 4, 5); x_obs, y_obs
 * the tick's tracks (columns >= num_prime zero: the validators read h <
 * num_prime only); noise, variant, seed, num_prime, num_obs the handle's
 * configuration; noise_level, acc_const_noise, steer_const_noise the handle's
 * fp32 fields widened; keys[0] = uint32(k + keys[e]), the tick's idx_mpc; draws
 * NULL; alpha, sigma from cfg.  The validators' Philox stream ids (24..30,
 * csrc/rng.hpp) are their own -- the solve draws from streams 0..7 and 16..18,
 * the step's variates from 45..49 -- so the rows are independent of the
 * solve's draws and of the step's variates under the same key.  Frozen episodes
 * are validated like the others (their frozen state and its plan).
 *
 * mpcmmd_mpc_validation_log synchronises and reads back the first `ticks` rows:
 * counts [ticks][E][2] = count, count_lane of mpcmmd_validate; count_pos
 * [ticks][E][3] per channel (obs, lane_lb, lane_ub); stats [ticks][E][4][3] =
 * var, cvar, mean, max per channel; mmd [ticks][E][3][num_sigma] (may be NULL
 * when num_sigma == 0); est [ticks][E][2] = the cost_lane and cost_obs the solve
 * itself estimated (mpcmmd_result).  mpcmmd_mpc_validation_inputs synchronises
 * and reads back the packed inputs of the last validated tick (debugging and
 * tests): cx, cy [E][11], init_state [E][6], x_obs, y_obs [E][num_obs][100],
 * keys [E]; a NULL array is skipped.
 *
 * Before any HIP call: MPCMMD_E_INVALID for a NULL c, num_rollouts outside
 * 1..2^20, alpha outside [0, 1], num_sigma outside 0..8, a sigma that is not
 * finite and > 0, an overlap other than 0 or 1, a handle whose num_obs is
 * outside the validators' 1..32 (the loop itself allows 0..64), a NULL required
 * log array, a tick range outside [0, max_ticks]; MPCMMD_E_STATE for a log or
 * inputs readback while the stage is off, and for a run between
 * mpcmmd_mpc_validate and the next reset. */
typedef struct mpcmmd_mpc_validation {
  int32_t num_rollouts; /* R: fresh noise rows per (tick, episode) */
  float alpha;          /* quantile level of VaR / CVaR */
  int32_t num_sigma;    /* S, 0..8 */
  float sigma[8];       /* MMD bandwidths, the same for every episode and tick */
  int32_t overlap;      /* 0: the stage in-line on the handle's stream; 1: its heavy part on the context's side stream */
} mpcmmd_mpc_validation;
int mpcmmd_mpc_validate(mpcmmd_mpc* c, const mpcmmd_mpc_validation* cfg);
int mpcmmd_mpc_validation_log(mpcmmd_mpc* c, int32_t ticks, int32_t* counts, int32_t* count_pos, float* stats,
                              float* mmd, float* est);
int mpcmmd_mpc_validation_inputs(mpcmmd_mpc* c, double* cx, double* cy, double* init_state, float* x_obs,
                                 float* y_obs, uint32_t* keys);

/* ---- Planned vehicles of the synthetic closed loop ------
 * With this policy a vehicle is no longer moved at constant velocity: it follows
 * the dynamic driver's lane-tracking QP (obs_data.compute_obs_guess, what
 * mpcmmd_obs_dynamic_traj solves once) and re-plans it every tick from its own
 * state.  A planned vehicle has the fp32 state S = (x, y, vx, vy, ax, ay) -- the
 * row (x, y, vx, vy) of `vehicles` and the row (ax, ay) of veh_acc -- and a
 * target (v_des, y_des), constant over the episode.  Three pure functions, each
 * element a sequential fp64 sum started at 0.0, rounded once to fp32 and stored
 * through the quiet-NaN rule (0x7FC00000), no contraction, no transcendental:
 *   plan(S, target)   rx[j] = (-2 v_des) colsum_x[j] (j < 11), rx[11..13] = x,
 *                     vx, ax; ry[j] = (-2 y_des) colsum_y[j], ry[11..14] = y, vy,
 *                     ay, 0; cxf[j] = float(sum_i kinv_x[j][i] rx[i]), cyf[j] =
 *                     float(sum_i kinv_y[j][i] ry[i]).  With ax = ay = 0 this is
 *                     mpcmmd_obs_dynamic_traj's solve bit for bit.
 *   track(c, k)       float(sum_j P[k][j] double(c[j])), k < 100
 *   advance(cxf, cyf) S' = (adv[0].cxf, adv[0].cyf, adv[1].cxf, adv[1].cyf,
 *                     adv[2].cxf, adv[2].cyf)
 * Where the step moves a vehicle by v dt, a live episode with the policy on does
 * S <- advance(plan(S, target)); a frozen or reset episode keeps S.  The clear
 * terms use the new positions, and the tracks the step writes are
 * track(plan(S, target), k) of the new S, in the same buffers and layouts.
 * Nothing else of the step changes.  A NaN in a state or a target reaches that
 * vehicle's tracks and state as the quiet NaN, and collided = !(clear <= 0)
 * applies; nothing is rejected for being NaN.
 *
 * mpcmmd_mpc_vehicle_constant returns the model's constants for the tick length
 * dt, 0 < dt < 15 (host only): "kinv_x" [14][14], "kinv_y" [15][15], "colsum_x",
 * "colsum_y" [11], "P" [100][11] (fp32-rounded), "adv" [3][11] = the rows P,
 * Pdot, Pddot of the same basis at the single time double(dt) on [0, 15], each
 * element rounded to fp32 and widened.  Return value as mpcmmd_host_constant's:
 * the element count, or MPCMMD_E_INVALID (dt out of range, an unknown name, dst
 * too small).
 *
 * mpcmmd_mpc_step_host_planned / _device_planned are mpcmmd_mpc_step_host /
 * _device with the policy on (the model's dt must be < 15); the device step gives
 * every array of pl a leading episode axis and runs the planned instantiation of
 * k_mpc_step, whose every word equals the host step's
 * (tests/test_gpu_mpc_vehicles.py).  A NULL pl, or a NULL veh_acc or veh_target
 * with num_obs > 0, is MPCMMD_E_INVALID before any HIP call.  ABI version
 * unchanged: detect the entry points by their symbols. */
int mpcmmd_mpc_vehicle_constant(float dt, const char* name, double* dst, size_t count);

typedef struct mpcmmd_mpc_planned { /* leading axis n_episodes for the device step */
  float* veh_acc;          /* [num_obs][2] ax, ay: updated in place unless the episode is frozen */
  const float* veh_target; /* [num_obs][2] v_des, y_des */
  float* veh_log;          /* [num_obs][6] S after the step, or NULL */
} mpcmmd_mpc_planned;

int mpcmmd_mpc_step_host_planned(const mpcmmd_mpc_model* m, int32_t tick, const mpcmmd_mpc_step_io* io,
                                 const mpcmmd_mpc_planned* pl);
int mpcmmd_mpc_step_device_planned(const mpcmmd_mpc_model* m, int32_t device, int32_t n_episodes, int32_t tick,
                                   const mpcmmd_mpc_step_io* io, const mpcmmd_mpc_planned* pl);

/* The policy on the chained route.  mpcmmd_mpc_plan_vehicles allocates into the
 * context what the policy needs -- the constants, the accelerations and targets
 * [max_configs][num_obs][2], the vehicle log [max_ticks][max_configs][num_obs][6]
 * -- and stages veh_target [n_episodes][num_obs][2] and veh_acc (NULL: zeros).
 * veh_target NULL turns the policy off and frees all of it.  Like
 * mpcmmd_mpc_validate it synchronises the context's streams and takes effect at
 * the next mpcmmd_mpc_reset: a run before that reset is MPCMMD_E_STATE, and a
 * reset with another n_episodes than the staged one is MPCMMD_E_INVALID.  Every
 * reset starts the accelerations from the staged ones again.  With the policy on
 * the reset's reset-mode step and every tick's step are the planned kernel; no
 * readback, no synchronisation and no allocation is added to the loop, and the
 * validation stage (which packs whatever tracks the step wrote) needs no change.
 * MPCMMD_E_INVALID for a NULL c, n_episodes outside 1..max_configs or a model
 * whose dt is not < 15.
 *
 * mpcmmd_mpc_vehicle_log synchronises like mpcmmd_mpc_log and reads back the
 * first `ticks` rows veh [ticks][E][num_obs][6]: every vehicle's S after that
 * tick's step.  MPCMMD_E_STATE with the policy off. */
int mpcmmd_mpc_plan_vehicles(mpcmmd_mpc* c, int32_t n_episodes, const float* veh_target, const float* veh_acc);
int mpcmmd_mpc_vehicle_log(mpcmmd_mpc* c, int32_t ticks, float* veh);

/* The scene queue of the synthetic chained route: N
 * scenes through E slots, a slot refilled on the device as soon as its episode
 * ends, one readback at the end.  (No ABI version change: callers detect the
 * entry points by their symbols.)
 *
 * The rule, per slot e with scene[e] (a scene index, or -1: idle) and ltick[e]
 * (its episode's local tick): after the step of a lockstep tick the episode has
 * ended if done[e] >= 0 (a collision or the goal) or ltick[e] ==
 * ticks_per_episode - 1.  Ended slots are served in ascending slot order; each
 * takes the next unstarted scene, or becomes idle (and frozen) once the table
 * is exhausted; every other live slot advances ltick[e] by one.  For every slot
 * the next solve's idx_mpc[e] = ltick[e] + key[e] (32-bit wrap).  One schedule
 * row per scene: sched [N][4] = slot, first lockstep tick, ticks run, end
 * reason (MPCMMD_QUEUE_*); a scene never started has slot and first tick -1.
 *
 * mpcmmd_mpc_queue_host applies the rule to host arrays (no GPU needed);
 * mpcmmd_mpc_queue_device is one k_mpc_queue launch on `device` over the same
 * arrays: the same words.  flags [E][4] is the step's log_i row of the tick,
 * keys and v_des [N] the scene table's; scene, ltick, done, key [E], sched and
 * count [2] = started, finished are state (in and out), fresh [E] (the scene a
 * slot took this tick, or -1), idx_mpc and slot_v_des [E] outputs (slot_v_des
 * is written for slots that take a scene only).  MPCMMD_E_INVALID for a NULL
 * array, n_slots or n_scenes < 1 (n_slots > 65535), ticks_per_episode < 1, a
 * scene word outside -1..N-1, count[0] outside 0..N. */
#define MPCMMD_QUEUE_UNFINISHED 0
#define MPCMMD_QUEUE_COLLISION 1
#define MPCMMD_QUEUE_GOAL 2
#define MPCMMD_QUEUE_TICK_LIMIT 3
typedef struct mpcmmd_mpc_queue_io {
  int32_t n_slots, n_scenes, ticks_per_episode, tick;
  const int32_t* flags;
  const int32_t* keys;
  const float* v_des;
  int32_t *scene, *ltick, *done, *fresh;
  uint32_t* key;
  int32_t* idx_mpc;
  float* slot_v_des;
  int32_t* sched;
  int32_t* count;
} mpcmmd_mpc_queue_io;
int mpcmmd_mpc_queue_host(const mpcmmd_mpc_queue_io* io);
int mpcmmd_mpc_queue_device(int32_t device, const mpcmmd_mpc_queue_io* io);

/* The queue on a context.  The scene table: pos [N][2], vel [N][3], vehicles
 * [N][num_obs][4], mean [N][8] (a scene's start mean), v_des [N], keys [N] and,
 * with the planned policy on (mpcmmd_mpc_plan_vehicles; its staged arrays are
 * not read), veh_target and veh_acc [N][num_obs][2]: both NULL without it.
 *
 * mpcmmd_mpc_queue_reset (synchronous, like mpcmmd_mpc_reset) uploads the
 * table, fills slots 0..min(N, n_slots)-1 with scenes in order -- a slot beyond
 * them is idle from the start: frozen on a copy of scene 0's start state, owned
 * by no scene -- and runs the reset-mode step.  The variates are always drawn.
 *
 * mpcmmd_mpc_queue_run enqueues, per lockstep tick of [tick_begin, tick_begin +
 * count): the chained begin (only cov is staged: idx_mpc and v_des are on the
 * device), the T CEM iterations, the step with each slot's own tick,
 * k_mpc_queue, and the reset-mode step masked to the slots that took a scene.
 * No readback, no synchronisation beyond the begin's staging-event wait, no
 * allocation.  The lockstep log is mpcmmd_mpc_log's, [tick][slot] rows
 * (done_tick holds local ticks); the schedule cuts it into per-scene episodes,
 * each bit-equal to that scene run alone (tests/test_gpu_mpc_queue.py).
 *
 * mpcmmd_mpc_queue_status synchronises and reads the two counters;
 * mpcmmd_mpc_queue_log synchronises and reads sched [N][4].
 *
 * MPCMMD_E_INVALID for a NULL argument, n_slots outside 1..max_configs,
 * n_scenes < 1, ticks_per_episode < 1, policy arrays that do not match the
 * policy's state, a tick range outside [0, max_ticks].  MPCMMD_E_STATE for any
 * queue call with the validation stage on (its validators are keyed by the
 * lockstep tick), for a queue run, status or log before a queue reset, and for
 * mpcmmd_mpc_run after a queue reset (until an ordinary reset) or a queue run
 * after an ordinary reset. */
typedef struct mpcmmd_mpc_scenes {
  int32_t n_scenes;
  const double* pos;
  const float* vel;
  const float* vehicles;
  const float* mean;
  const float* v_des;
  const int32_t* keys;
  const float* veh_target;
  const float* veh_acc;
} mpcmmd_mpc_scenes;
int mpcmmd_mpc_queue_reset(mpcmmd_mpc* c, int32_t n_slots, int32_t ticks_per_episode, const mpcmmd_mpc_scenes* scenes,
                           const float* cov);
int mpcmmd_mpc_queue_run(mpcmmd_mpc* c, int32_t cost_kind, int32_t tick_begin, int32_t count, const float* cov);
int mpcmmd_mpc_queue_status(mpcmmd_mpc* c, int32_t* started, int32_t* finished);
int mpcmmd_mpc_queue_log(mpcmmd_mpc* c, int32_t* sched);

#ifdef __cplusplus
}
#endif
#endif /* MPCMMD_H */
