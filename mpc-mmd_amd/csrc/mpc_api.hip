// libmpcmmd: the synthetic closed loop on the device (include/mpcmmd.h).
// mpcmmd_mpc_step_device holds k_mpc_step against the host twin.  The context
// (mpcmmd_mpc) is an episode context (episodes.hpp owns the buffers, the reset's
// prologue, the tick loop and the read-backs) whose tick is the resident begin
// (begin.hip), the CEM iterations and k_mpc_step on the handle's stream: the
// kernel reads the handle's result buffer and writes st0, solve_c, obs and
// iteration 0's population, so nothing crosses the host between two solves.
// With a validation stage configured (mpcmmd_mpc_validate)
// each tick also enqueues, between its CEM iterations and its step, the
// Monte-Carlo risk of the plan it just made: k_mpc_validate_prep packs the
// validators' inputs from the device buffers the solve used, then
// mpcmmd_validate's and mpcmmd_validate_risk's own launches write the tick's row
// of the validation log, on the handle's stream or on the context's side stream.
// With the vehicle policy configured (mpcmmd_mpc_plan_vehicles, DESIGN.md section
// 23) the reset's and every tick's step is k_mpc_step_planned: the constants, the
// accelerations, the targets and the vehicle log live in the context, and the
// loop gains no copy, synchronisation or allocation.
#include <cstring>

#include "episodes.hpp"
#include "mpc.hpp"
#include "mpc_draw.hpp"
#include "mpc_host.hpp"
#include "mpc_validate.hpp"
#include "rng.hpp"
#include "solve_host.hpp"

using namespace mpcmmd;

// hidden, as everything of episodes.hpp it embeds: no constructor or destructor becomes a dynamic symbol
struct __attribute__((visibility("hidden"))) mpcmmd_mpc {
  Episodes s;         // the episodes, the log and the two stages' common state (episodes.hpp)
  MpcStepParams q{};  // the model's arrays and the state, filled at create
  // the validation stage (off: none of the stream and events exists)
  bool val_overlap = false;   // the validators' launches go to the side stream
  MpcValidateParams vp{};     // the packed inputs once more, as k_mpc_validate_prep writes them
  hipStream_t side = nullptr;                       // the validators' stream of an overlapped stage
  hipEvent_t ev_prep = nullptr, ev_done = nullptr;  // the prep is done; the side stream's tick is done
  bool side_pending = false;                        // ev_done was recorded since the last synchronisation
  // the planned vehicles
  MpcVehParams pv{};             // the constants, the live accelerations, the targets
  float* veh_acc0 = nullptr;     // [Emax][O][2] the staged accelerations every reset starts from
  float* veh_log = nullptr;      // [Tmax][Emax][O][6]
};

namespace {

// guess_kinv_x/y, proj_kinv_x/y columns 11.. of rows 0..10, as solve_columns reads them: [4][11][4]
std::vector<double> kkt_columns(const ProblemConsts& pc) {
  std::vector<double> out(size_t(4) * kNvar * 4, 0.0);
  for (int k = 0; k < kNvar; ++k) {
    for (int e = 0; e < 3; ++e) out[(0 * kNvar + k) * 4 + e] = pc.guess_kinv_x[k * 14 + kNvar + e];
    for (int e = 0; e < 4; ++e) out[(1 * kNvar + k) * 4 + e] = pc.guess_kinv_y[k * 15 + kNvar + e];
    for (int e = 0; e < 3; ++e) out[(2 * kNvar + k) * 4 + e] = pc.proj_kinv_x[k * 14 + kNvar + e];
    for (int e = 0; e < 4; ++e) out[(3 * kNvar + k) * 4 + e] = pc.proj_kinv_y[k * 15 + kNvar + e];
  }
  return out;
}

// one k_mpc_step over the context's episodes, on the handle's stream: behind everything
// mpcmmd_iterate enqueued (the group streams of large handles join it before iterate returns),
// ahead of the next begin.  The plan from the handle's results of the last iteration, the next
// solve's buffers where begin_impl's resident route expects them.
void enqueue_step(mpcmmd_mpc* c, int tick, bool reset) {
  const Episodes& s = c->s;
  mpcmmd_handle* h = s.h;
  MpcStepParams q = c->q;
  q.tick = tick, q.reset = reset ? 1 : 0;
  const int T = h->T;
  float* res = h->p.results + size_t(T - 1) * kResultStride;
  q.cx = res, q.cy = res + 11, q.s_plan = T * kResultStride;
  q.mean = h->p.mean;
  q.H = h->H;
  q.obs = const_cast<float*>(h->p.obs);
  q.st0 = const_cast<float*>(h->p.st0);
  q.solve_c = const_cast<double*>(h->p.solve_c);
  q.pop = h->p.pop;
  const size_t row = size_t(reset ? 0 : tick) * s.Emax;
  q.u = s.drawn ? nullptr : s.u + row * 3;
  q.key = s.keys_dev, q.seed = h->cfg.seed;
  q.logd = s.logd + row * 2, q.logf = s.logf + row * 12, q.logi = s.logi + row * 4;
  q.plan = s.plan + row * 30;
  q.chol = s.chol;
  if (s.veh_on) {
    MpcVehParams pv = c->pv;
    pv.log = c->veh_log + row * size_t(q.w.O) * 6;
    launch_mpc_step_planned(q, pv, s.E, h->stream);
  } else {
    launch_mpc_step(q, s.E, h->stream);
  }
  HIPC(hipGetLastError());
}

// the validation stage of tick `tick`, behind its CEM iterations and before its step (the step
// overwrites pos, vel and obs, the next solve the results): the packed inputs on the handle's
// stream, then mpcmmd_validate's and mpcmmd_validate_risk's launches with K = E and the results
// pointed at the tick's log row -- behind the prep, or on the side stream between two events
void enqueue_validation(mpcmmd_mpc* c, int tick) {
  const Episodes& s = c->s;
  mpcmmd_handle* h = s.h;
  const int T = h->T, E = s.E;
  const size_t row = size_t(tick) * s.Emax;
  if (c->side_pending) {  // the previous tick's validators still own the packed inputs, the costs and the scratch
    HIPC(hipStreamWaitEvent(h->stream, c->ev_done, 0));
    c->side_pending = false;
  }
  MpcValidateParams p = c->vp;
  p.tick = tick;
  p.res = h->p.results + size_t(T - 1) * kResultStride, p.s_res = T * kResultStride;
  p.pos = c->q.pos, p.vel = c->q.vel;
  p.obs = h->p.obs;
  p.key = s.keys_dev;
  p.est = s.vl.est + row * 2;
  launch_mpc_validate_prep(p, E, h->stream);
  HIPC(hipGetLastError());
  hipStream_t st = h->stream;
  if (c->val_overlap) {
    HIPC(hipEventRecord(c->ev_prep, h->stream));
    HIPC(hipStreamWaitEvent(c->side, c->ev_prep, 0));
    st = c->side;
  }
  ValidateRiskParams q = s.vq;
  q.K = q.roll.K = E;
  ValidateParams v = q.roll;
  v.count = s.vl.count[0] + row, v.count_lane = s.vl.count[1] + row;
  launch_validate(v, st);
  HIPC(hipGetLastError());
  s.vl.point(q, row);
  launch_vrisk_roll(q, st);
  HIPC(hipGetLastError());
  launch_vrisk_stats(q, st);
  HIPC(hipGetLastError());
  launch_vrisk_mmd(q, st);
  HIPC(hipGetLastError());
  if (c->val_overlap) {
    HIPC(hipEventRecord(c->ev_done, c->side));
    c->side_pending = true;
  }
}

// the handle's stream and the side stream idle
void sync_streams(mpcmmd_mpc* c) {
  HIPC(hipStreamSynchronize(c->s.h->stream));
  if (c->side) HIPC(hipStreamSynchronize(c->side));
  c->side_pending = false;
}

// frees the validation stage's buffers, its stream and events
void drop_validation(mpcmmd_mpc* c) {
  c->s.val.release();
  if (c->ev_prep) (void)hipEventDestroy(c->ev_prep);
  if (c->ev_done) (void)hipEventDestroy(c->ev_done);
  if (c->side) (void)hipStreamDestroy(c->side);
  c->ev_prep = c->ev_done = nullptr, c->side = nullptr;
  c->side_pending = false;
  c->s.val_on = false;
}

void drop_vehicles(mpcmmd_mpc* c) {
  c->s.veh.release();
  c->pv = MpcVehParams{};
  c->veh_acc0 = c->veh_log = nullptr;
  c->s.veh_on = false, c->s.veh_E = 0;
}

// the constants of t in device memory, allocated by `up(src, doubles)`
template <class F>
MpcVehConsts upload_vehicle_consts(const MpcVehTables& t, F&& up) {
  MpcVehConsts k;
  k.kinv_x = up(t.qp->kinv_x.data(), t.qp->kinv_x.size());
  k.kinv_y = up(t.qp->kinv_y.data(), t.qp->kinv_y.size());
  k.colsum_x = up(t.qp->colsum_x.data(), t.qp->colsum_x.size());
  k.colsum_y = up(t.qp->colsum_y.data(), t.qp->colsum_y.size());
  k.P = up(t.qp->P.data(), t.qp->P.size());
  k.adv = up(t.adv.data(), t.adv.size());
  return k;
}

int step_device(const mpcmmd_mpc_model* m, int32_t device, int32_t n_episodes, int32_t tick,
                const mpcmmd_mpc_step_io* io, const mpcmmd_mpc_planned* pl) {
  return guarded([&] {
    StepHarness hs;
    if (int rc = hs.open("mpc", device, n_episodes)) return rc;
    const size_t E = size_t(n_episodes), O = size_t(m->num_obs), B = size_t(m->num_batch);
    MpcStepParams q{};
    q.w = mpc_scalars(*m);
    q.tick = tick;
    q.s_plan = 11, q.H = 0;
    q.pdot2 = hs.in(m->pdot2, 22), q.pddot1 = hs.in(m->pddot1, 11), q.chol = hs.in(m->chol, 64);
    q.pop0 = hs.in(m->pop0, B * 8);
    q.cx = hs.in(io->cx, E * 11), q.cy = hs.in(io->cy, E * 11);
    q.u = io->u ? hs.in(io->u, E * 3) : nullptr;
    q.key = io->key ? hs.in(io->key, E) : nullptr;
    q.seed = m->seed;
    q.mean = hs.in(io->mean, E * 8);
    // state: in and out; a world without vehicles still gets a pointer
    q.pos = hs.io(io->pos, E * 2, true), q.vel = hs.io(io->vel, E * 3, true);
    q.veh = hs.io(io->vehicles, E * O * 4, true), q.done = hs.io(io->done_tick, E, true);
    q.init = hs.io(io->init_state, E * 6, false), q.st0 = hs.io(io->st0, E * 8, false);
    q.x_obs = hs.io(io->x_obs, E * O * kMpcTrack, false), q.y_obs = hs.io(io->y_obs, E * O * kMpcTrack, false);
    q.pop = hs.io(io->pop, E * B * 8, false);
    q.logd = hs.io(io->log_d, E * MPCMMD_MPC_LOG_D, false), q.logf = hs.io(io->log_f, E * MPCMMD_MPC_LOG_F, false);
    q.logi = hs.io(io->log_i, E * MPCMMD_MPC_LOG_I, false);
    if (pl) {
      const MpcVehTables t = mpc_vehicle_tables(m->dt);
      MpcVehParams pv{};
      pv.k = upload_vehicle_consts(t, [&](const double* src, size_t n) { return hs.in(src, n); });
      pv.target = hs.in(pl->veh_target, E * O * 2);
      pv.acc = hs.io(pl->veh_acc, E * O * 2, true);
      pv.log = pl->veh_log ? hs.io(pl->veh_log, E * O * 6, false) : nullptr;
      launch_mpc_step_planned(q, pv, n_episodes, nullptr);
    } else {
      launch_mpc_step(q, n_episodes, nullptr);
    }
    hs.finish();
    return MPCMMD_OK;
  });
}

}  // namespace

extern "C" {

int mpcmmd_mpc_step_host(const mpcmmd_mpc_model* m, int32_t tick, const mpcmmd_mpc_step_io* io) {
  if (int rc = check_mpc(m, io)) return rc;
  mpc_step_host(*m, tick, *io, mpc_draw);
  return MPCMMD_OK;
}

int mpcmmd_mpc_first_normals(const mpcmmd_config* cfg, float* out) {
  if (!cfg || !out) return fail(MPCMMD_E_INVALID, "null argument");
  if (cfg->num_batch < 1) return fail(MPCMMD_E_INVALID, "mpc: num_batch >= 1");
  const std::vector<float> z = host_normals(kFixedKey0, cfg->seed, kStreamPop0, 0, size_t(cfg->num_batch) * 8);
  std::memcpy(out, z.data(), z.size() * 4);
  return MPCMMD_OK;
}

int mpcmmd_mpc_step_host_planned(const mpcmmd_mpc_model* m, int32_t tick, const mpcmmd_mpc_step_io* io,
                                 const mpcmmd_mpc_planned* pl) {
  if (int rc = check_mpc(m, io)) return rc;
  if (int rc = check_mpc_planned(m, pl)) return rc;
  try {
    const MpcVehTables t = mpc_vehicle_tables(m->dt);
    const MpcVehConsts vc = t.view();
    mpc_step_host(*m, tick, *io, mpc_draw, pl, &vc);
    return MPCMMD_OK;
  } catch (const std::exception& e) {
    return fail(MPCMMD_E_INVALID, e.what());
  }
}

int mpcmmd_mpc_step_device(const mpcmmd_mpc_model* m, int32_t device, int32_t n_episodes, int32_t tick,
                           const mpcmmd_mpc_step_io* io) {
  if (int rc = check_mpc(m, io)) return rc;
  return step_device(m, device, n_episodes, tick, io, nullptr);
}

int mpcmmd_mpc_step_device_planned(const mpcmmd_mpc_model* m, int32_t device, int32_t n_episodes, int32_t tick,
                                   const mpcmmd_mpc_step_io* io, const mpcmmd_mpc_planned* pl) {
  if (int rc = check_mpc(m, io)) return rc;
  if (int rc = check_mpc_planned(m, pl)) return rc;
  return step_device(m, device, n_episodes, tick, io, pl);
}

int mpcmmd_mpc_create(mpcmmd_handle* h, const mpcmmd_mpc_model* m, int32_t max_ticks, mpcmmd_mpc** out) {
  if (!h || !m || !out) return fail(MPCMMD_E_INVALID, "null argument");
  *out = nullptr;
  if (h->carla) return fail(MPCMMD_E_INVALID, "mpc: a handle of a static or dynamic variant is needed (CARLA: mpcmmd_world)");
  mpcmmd_mpc_model mm = *m;
  mm.num_batch = h->B;  // the handle's population and its own pop0 normals
  const double unit[64] = {};
  const float none[8] = {};
  if (!mm.chol) mm.chol = unit;  // chol, pop0: not read by the context
  if (!mm.pop0) mm.pop0 = none;
  if (int rc = check_mpc_model(&mm)) return rc;
  if (m->num_obs != h->O) return fail(MPCMMD_E_INVALID, "mpc: num_obs is not the handle's");
  if (max_ticks < 1 || max_ticks > (1 << 20)) return fail(MPCMMD_E_INVALID, "mpc: 1 <= max_ticks <= 2^20");
  auto* c = new mpcmmd_mpc();
  Episodes& s = c->s;
  s.h = h;
  s.Tmax = max_ticks, s.Emax = h->Gmax;
  int rc = guarded([&] {
    check_device(h);
    const size_t E = size_t(s.Emax), O = size_t(m->num_obs);
    if (h->pop0_normals.empty())
      h->pop0_normals = host_normals(kFixedKey0, h->cfg.seed, kStreamPop0, 0, size_t(h->B) * 8);
    const std::vector<double> kc = kkt_columns(h->pc);
    MpcStepParams& q = c->q;
    Arena& a = s.base;
    q.w = mpc_scalars(mm);
    q.pdot2 = a.alloc<double>(22, m->pdot2), q.pddot1 = a.alloc<double>(11, m->pddot1);
    q.kcol = a.alloc<double>(kc.size(), kc.data());
    q.pop0 = a.alloc<float>(h->pop0_normals.size(), h->pop0_normals.data());
    s.chol = a.alloc<double>(64);
    q.pos = s.pos = a.alloc<double>(E * 2), q.vel = a.alloc<float>(E * 3);
    q.veh = a.alloc<float>(E * O * 4), q.done = s.done = a.alloc<int32_t>(E);
    s.alloc_rows(3, MPCMMD_MPC_LOG_D, MPCMMD_MPC_LOG_F, MPCMMD_MPC_LOG_I, 30);
    return MPCMMD_OK;
  });
  if (rc != MPCMMD_OK) {
    mpcmmd_mpc_destroy(c);
    (void)hipGetLastError();
    return rc;
  }
  *out = c;
  return MPCMMD_OK;
}

void mpcmmd_mpc_destroy(mpcmmd_mpc* c) {
  if (!c) return;
  (void)hipSetDevice(c->s.h->device);
  if (c->s.h->stream) (void)hipStreamSynchronize(c->s.h->stream);  // the steps in flight
  if (c->side) (void)hipStreamSynchronize(c->side);                // and the validators
  drop_validation(c);  // its stream and events
  delete c;            // the three arenas free their buffers
}

int mpcmmd_mpc_reset(mpcmmd_mpc* c, int32_t n_episodes, const double* pos, const float* vel, const float* vehicles,
                     const float* mean, const float* cov, const float* u, const int32_t* keys) {
  if (!c || !pos || !vel || !mean || !cov || !keys || (c->q.w.O > 0 && !vehicles))
    return fail(MPCMMD_E_INVALID, "null argument");
  if (n_episodes < 1 || n_episodes > c->s.Emax)
    return fail(MPCMMD_E_INVALID, "mpc: n_episodes must be 1..max_configs of the handle");
  if (c->s.veh_on && n_episodes != c->s.veh_E)
    return fail(MPCMMD_E_INVALID, "mpc: n_episodes is not the one mpcmmd_mpc_plan_vehicles staged");
  auto upload = [&](size_t E) {
    const size_t O = size_t(c->q.w.O);
    HIPC(hipMemcpy(c->q.vel, vel, E * 3 * 4, hipMemcpyHostToDevice));
    if (O) HIPC(hipMemcpy(c->q.veh, vehicles, E * O * 4 * 4, hipMemcpyHostToDevice));
    if (c->s.veh_on && O) HIPC(hipMemcpy(c->pv.acc, c->veh_acc0, E * O * 2 * 4, hipMemcpyDeviceToDevice));
  };
  return reset_common(c->s, n_episodes, pos, mean, cov, u, keys, [&] { sync_streams(c); }, upload, [&] {
    enqueue_step(c, -1, true);  // tick 0's st0, solve_c, obs and population from the start states
    HIPC(hipStreamSynchronize(c->s.h->stream));
  });
}

int mpcmmd_mpc_run(mpcmmd_mpc* c, int32_t cost_kind, int32_t tick_begin, int32_t count, const float* cov,
                   const float* v_des) {
  if (!c || !cov || !v_des) return fail(MPCMMD_E_INVALID, "null argument");
  if (!c->s.reset_done) return fail(MPCMMD_E_STATE, "mpcmmd_mpc_run before mpcmmd_mpc_reset");
  if (tick_begin < 0 || count < 0 || tick_begin + count > c->s.Tmax) return fail(MPCMMD_E_INVALID, "mpc: tick range");
  return run_ticks(
      c->s, tick_begin, count, cov,
      [&](const int32_t* idx, const float* covs) {
        return begin_impl(c->s.h, c->s.E, cost_kind, idx, nullptr, nullptr, covs, nullptr, nullptr, v_des, nullptr,
                          nullptr, nullptr, true);
      },
      [&](int k) {
        if (c->s.val_on) enqueue_validation(c, k);
        enqueue_step(c, k, false);
      });
}

int mpcmmd_mpc_log(mpcmmd_mpc* c, int32_t ticks, double* log_d, float* log_f, int32_t* log_i, float* plan,
                   int32_t* done_tick) {
  if (!c || !log_d || !log_f || !log_i || !plan || !done_tick) return fail(MPCMMD_E_INVALID, "null argument");
  if (ticks < 0 || ticks > c->s.Tmax) return fail(MPCMMD_E_INVALID, "mpc: tick range");
  return guarded([&] {
    check_device(c->s.h);
    sync_streams(c);
    const size_t E = size_t(c->s.E);
    if (ticks > 0 && E > 0) log_rows_back(c->s, ticks, log_d, log_f, log_i, plan);
    if (E > 0) HIPC(hipMemcpy(done_tick, c->s.done, E * 4, hipMemcpyDeviceToHost));
    return MPCMMD_OK;
  });
}

int mpcmmd_mpc_validate(mpcmmd_mpc* c, const mpcmmd_mpc_validation* cfg) {
  if (!c) return fail(MPCMMD_E_INVALID, "null argument");
  Episodes& s = c->s;
  mpcmmd_handle* h = s.h;
  const int O = h->O, H = h->H;
  ValidateRiskParams q{};
  if (cfg) {
    q.R = q.roll.R = cfg->num_rollouts, q.S = cfg->num_sigma;
    if (int rc = check_risk_config("mpc", q.R, cfg->alpha, q.S, cfg->sigma, &q.lo, &q.hi, &q.w_lo, &q.w_hi)) return rc;
    if (cfg->overlap != 0 && cfg->overlap != 1) return fail(MPCMMD_E_INVALID, "mpc validation: overlap must be 0 or 1");
    if (!validate_shape_ok(O, H))
      return fail(MPCMMD_E_INVALID, "mpc validation: the validators take 1 <= num_obs <= 32 and 2 <= num_prime <= 100");
  }
  return remake_stage(s, cfg != nullptr, [&] { sync_streams(c); }, [&] { drop_validation(c); }, [&] {
    s.val_on = true;
    c->val_overlap = cfg->overlap == 1;
    HIPC(hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking));
    HIPC(hipEventCreateWithFlags(&c->ev_prep, hipEventDisableTiming));
    HIPC(hipEventCreateWithFlags(&c->ev_done, hipEventDisableTiming));
    Arena& a = s.val;
    const size_t Em = size_t(s.Emax);
    const ProblemConsts& pc = h->pc;
    const mpcmmd_config& hc = h->cfg;
    ValidateParams& v = q.roll;  // as plan_params (validate_api.hip)
    v.O = O, v.H = H, v.noise = hc.noise;
    v.noise_level = hc.noise_level, v.acc_const = hc.acc_const_noise, v.steer_const = hc.steer_const_noise;
    v.K_steer = pc.K_steer, v.y_lb = pc.y_lb, v.y_ub = pc.y_ub, v.seed = hc.seed;
    const std::vector<float> basis = pack_basis(pc);  // P, Pdot, Pddot
    v.Pdot = a.alloc<float>(size_t(kNum) * kNvar, basis.data() + kNum * kNvar);
    v.Pddot = a.alloc<float>(size_t(kNum) * kNvar, basis.data() + 2 * kNum * kNvar);
    MpcValidateParams& p = c->vp;
    p = MpcValidateParams{};
    p.H = H, p.O = O;
    v.cx = p.cx = a.alloc<double>(Em * kNvar), v.cy = p.cy = a.alloc<double>(Em * kNvar);
    v.init_state = p.init = a.alloc<double>(Em * 6);
    v.x_obs = p.x_obs = a.alloc<float>(Em * O * kMpcTrack);
    v.y_obs = p.y_obs = a.alloc<float>(Em * O * kMpcTrack);
    v.keys = p.keys = a.alloc<uint32_t>(Em);
    v.draws = nullptr;
    alloc_risk_scratch(a, q, Em, cfg->sigma);  // the costs: every element is stored by its rollout's thread
    s.vq = q;
    s.vl.alloc(a, size_t(s.Tmax) * Em, size_t(q.S), 2);
    return MPCMMD_OK;
  });
}

int mpcmmd_mpc_validation_log(mpcmmd_mpc* c, int32_t ticks, int32_t* counts, int32_t* count_pos, float* stats,
                              float* mmd, float* est) {
  if (!c) return fail(MPCMMD_E_INVALID, "null argument");
  return validation_log_back(c->s, "mpc", "mpcmmd_mpc_validation_log", ticks, counts, count_pos, stats, mmd, est,
                             [&] { sync_streams(c); });
}

int mpcmmd_mpc_validation_inputs(mpcmmd_mpc* c, double* cx, double* cy, double* init_state, float* x_obs,
                                 float* y_obs, uint32_t* keys) {
  if (!c) return fail(MPCMMD_E_INVALID, "null argument");
  if (!c->s.val_on) return fail(MPCMMD_E_STATE, "mpcmmd_mpc_validation_inputs without a validation stage");
  return guarded([&] {
    check_device(c->s.h);
    sync_streams(c);
    const size_t E = size_t(c->s.E), O = size_t(c->vp.O);
    back_if(cx, c->vp.cx, E * kNvar * 8), back_if(cy, c->vp.cy, E * kNvar * 8);
    back_if(init_state, c->vp.init, E * 6 * 8), back_if(keys, c->vp.keys, E * 4);
    back_if(x_obs, c->vp.x_obs, E * O * kMpcTrack * 4), back_if(y_obs, c->vp.y_obs, E * O * kMpcTrack * 4);
    return MPCMMD_OK;
  });
}

int mpcmmd_mpc_plan_vehicles(mpcmmd_mpc* c, int32_t n_episodes, const float* veh_target, const float* veh_acc) {
  if (!c) return fail(MPCMMD_E_INVALID, "null argument");
  MpcVehTables t{};
  if (veh_target) {
    if (n_episodes < 1 || n_episodes > c->s.Emax)
      return fail(MPCMMD_E_INVALID, "mpc: n_episodes must be 1..max_configs of the handle");
    if (!(c->q.w.dt < 15.0f)) return fail(MPCMMD_E_INVALID, "mpc vehicles: 0 < dt < 15");
    try {
      t = mpc_vehicle_tables(c->q.w.dt);
    } catch (const std::exception& e) {
      return fail(MPCMMD_E_INVALID, e.what());
    }
  }
  return remake_stage(c->s, veh_target != nullptr, [&] { sync_streams(c); }, [&] { drop_vehicles(c); }, [&] {
    Episodes& s = c->s;
    Arena& a = s.veh;
    const size_t Em = size_t(s.Emax), Tm = size_t(s.Tmax), O = size_t(c->q.w.O), n = size_t(n_episodes) * O * 2;
    c->pv.k = upload_vehicle_consts(t, [&](const double* src, size_t cnt) { return a.alloc<double>(cnt, src); });
    c->pv.target = a.alloc<float>(Em * O * 2, nullptr);
    c->pv.acc = a.alloc<float>(Em * O * 2);
    c->veh_acc0 = a.alloc<float>(Em * O * 2);
    c->veh_log = a.alloc<float>(Tm * Em * O * 6);
    if (n) {
      HIPC(hipMemcpy(const_cast<float*>(c->pv.target), veh_target, n * 4, hipMemcpyHostToDevice));
      if (veh_acc) HIPC(hipMemcpy(c->veh_acc0, veh_acc, n * 4, hipMemcpyHostToDevice));
      else HIPC(hipMemset(c->veh_acc0, 0, n * 4));
    }
    s.veh_E = n_episodes;
    s.veh_on = true;
    return MPCMMD_OK;
  });
}

int mpcmmd_mpc_vehicle_log(mpcmmd_mpc* c, int32_t ticks, float* veh) {
  if (!c || !veh) return fail(MPCMMD_E_INVALID, "null argument");
  if (ticks < 0 || ticks > c->s.Tmax) return fail(MPCMMD_E_INVALID, "mpc: tick range");
  if (!c->s.veh_on) return fail(MPCMMD_E_STATE, "mpcmmd_mpc_vehicle_log without the vehicle policy");
  return guarded([&] {
    check_device(c->s.h);
    sync_streams(c);
    const size_t row = size_t(c->q.w.O) * 6 * 4, E = size_t(c->s.E);
    if (ticks > 0 && E > 0 && row > 0) rows_back(veh, c->veh_log, row, ticks, E, size_t(c->s.Emax));
    return MPCMMD_OK;
  });
}

}  // extern "C"
