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
// The scene queue (mpcmmd_mpc_queue_*) runs N scenes
// through the context's slots: per tick the begin stages only cov, the step takes
// each slot's own tick, k_mpc_queue (k_mpc_queue.hip) refills the slots whose
// episode ended and a reset-mode step masked to them writes their next solve's
// buffers.
#include <algorithm>
#include <cstring>
#include <type_traits>

#include "episodes.hpp"
#include "mpc.hpp"
#include "mpc_draw.hpp"
#include "mpc_host.hpp"
#include "mpc_queue_host.hpp"
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
  // the scene queue
  Arena queue;               // the scene table, the slots' words and the schedule of the last queue reset
  MpcQueueParams qp{};       // k_mpc_queue's arguments but the tick and its log_i row
  bool queue_on = false;     // the steps are the queue's instantiations (set by either reset)
  bool queue_ready = false;  // a queue reset succeeded and nothing replaced it since
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
// With the queue on the step is the queue's instantiation: each slot's own tick, and with `masked`
// (the reset-mode step behind k_mpc_queue) only the slots that took a scene.
void enqueue_step(mpcmmd_mpc* c, int tick, bool reset, bool masked = false) {
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
  if (c->queue_on) q.ltick = c->qp.st.ltick, q.fresh = masked ? c->qp.st.fresh : nullptr;
  if (s.veh_on) {
    MpcVehParams pv = c->pv;
    pv.log = masked ? nullptr : c->veh_log + row * size_t(q.w.O) * 6;  // a refill logs no row
    if (c->queue_on) launch_mpc_step_planned_queue(q, pv, s.E, h->stream);
    else launch_mpc_step_planned(q, pv, s.E, h->stream);
  } else if (c->queue_on) {
    launch_mpc_step_queue(q, s.E, h->stream);
  } else {
    launch_mpc_step(q, s.E, h->stream);
  }
  HIPC(hipGetLastError());
}

// k_mpc_queue behind the step of lockstep tick `tick`: the rule on the slots' words, the refills
void enqueue_queue(mpcmmd_mpc* c, int tick) {
  MpcQueueParams p = c->qp;
  p.tick = tick;
  p.flags = c->s.logi + size_t(tick) * c->s.Emax * 4;
  launch_mpc_queue(p, c->s.h->stream);
  HIPC(hipGetLastError());
}

// what every queue call checks first
int queue_state(mpcmmd_mpc* c, const char* entry, bool need_reset) {
  if (c->s.val_on)
    return fail(MPCMMD_E_STATE, std::string(entry) + " with the validation stage on (its validators are keyed by the lockstep tick)");
  if (need_reset && !c->queue_ready)
    return fail(MPCMMD_E_STATE, std::string(entry) + (c->s.reset_done ? " after mpcmmd_mpc_reset: the queue needs mpcmmd_mpc_queue_reset"
                                                                     : " before mpcmmd_mpc_queue_reset"));
  return MPCMMD_OK;
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
  c->queue_on = c->queue_ready = false;  // nothing is in flight once the reset has synchronised
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
  if (!c->s.reset_done)
    return fail(MPCMMD_E_STATE, c->queue_ready ? "mpcmmd_mpc_run after mpcmmd_mpc_queue_reset: an ordinary run needs mpcmmd_mpc_reset"
                                               : "mpcmmd_mpc_run before mpcmmd_mpc_reset");
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
  c->queue_ready = false;  // like reset_done: the stage changes with the episodes
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
  c->queue_ready = false;  // the queue's refills point into the policy's arrays
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

int mpcmmd_mpc_queue_device(int32_t device, const mpcmmd_mpc_queue_io* io) {
  if (int rc = check_mpc_queue(io)) return rc;
  return guarded([&] {
    StepHarness hs;
    if (int rc = hs.open("mpc queue", device, io->n_slots)) return rc;
    const size_t E = size_t(io->n_slots), N = size_t(io->n_scenes);
    MpcQueueParams p{};
    p.E = io->n_slots, p.N = io->n_scenes, p.ticks_per_episode = io->ticks_per_episode, p.tick = io->tick;
    p.flags = hs.in(io->flags, E * 4);
    p.tab_key = hs.in(reinterpret_cast<const uint32_t*>(io->keys), N), p.tab_v_des = hs.in(io->v_des, N);
    MpcQueueState& st = p.st;
    st.scene = hs.io(io->scene, E, true), st.ltick = hs.io(io->ltick, E, true), st.done = hs.io(io->done, E, true);
    st.fresh = hs.io(io->fresh, E, false), st.key = hs.io(io->key, E, true);
    st.idx_mpc = hs.io(io->idx_mpc, E, false), st.v_des = hs.io(io->slot_v_des, E, true);
    st.sched = hs.io(io->sched, N * 4, true), st.count = hs.io(io->count, 2, true);
    launch_mpc_queue(p, nullptr);  // no state tables: the rule's words only
    hs.finish();
    return MPCMMD_OK;
  });
}

int mpcmmd_mpc_queue_reset(mpcmmd_mpc* c, int32_t n_slots, int32_t ticks_per_episode, const mpcmmd_mpc_scenes* sc,
                           const float* cov) {
  if (!c || !sc || !cov) return fail(MPCMMD_E_INVALID, "null argument");
  if (int rc = queue_state(c, "mpcmmd_mpc_queue_reset", false)) return rc;
  const size_t O = size_t(c->q.w.O);
  if (!sc->pos || !sc->vel || !sc->mean || !sc->v_des || !sc->keys || (O > 0 && !sc->vehicles))
    return fail(MPCMMD_E_INVALID, "null argument");
  if (n_slots < 1 || n_slots > c->s.Emax) return fail(MPCMMD_E_INVALID, "mpc queue: n_slots must be 1..max_configs of the handle");
  if (sc->n_scenes < 1 || sc->n_scenes > (1 << 24)) return fail(MPCMMD_E_INVALID, "mpc queue: 1 <= n_scenes <= 2^24");
  if (ticks_per_episode < 1) return fail(MPCMMD_E_INVALID, "mpc queue: ticks_per_episode >= 1");
  const bool planned = c->s.veh_on;
  if (planned ? (O > 0 && (!sc->veh_target || !sc->veh_acc)) : (sc->veh_target || sc->veh_acc))
    return fail(MPCMMD_E_INVALID, planned ? "mpc queue: the planned policy is on: veh_target and veh_acc are needed"
                                          : "mpc queue: veh_target and veh_acc need the planned policy (mpcmmd_mpc_plan_vehicles)");
  const size_t E = size_t(n_slots), N = size_t(sc->n_scenes), filled = std::min(E, N);
  // the slots' start: scene e in slot e; a slot beyond the table idles on a copy of scene 0
  auto of = [&](size_t e) { return e < filled ? e : size_t(0); };
  auto rows = [&](auto* tab, size_t width) {
    std::vector<std::remove_cv_t<std::remove_pointer_t<decltype(tab)>>> v(E * width);
    for (size_t e = 0; e < E; ++e) std::copy(tab + of(e) * width, tab + (of(e) + 1) * width, v.begin() + e * width);
    return v;
  };
  const std::vector<double> pos = rows(sc->pos, 2);
  const std::vector<float> vel = rows(sc->vel, 3), mean = rows(sc->mean, 8), vdes = rows(sc->v_des, 1);
  const std::vector<int32_t> keys = rows(sc->keys, 1);
  std::vector<int32_t> scene(E), done(E), idx(E), none(E, -1), sched(N * 4, 0), count = {int32_t(filled), 0};
  for (size_t e = 0; e < E; ++e) {
    scene[e] = e < filled ? int32_t(e) : -1, done[e] = e < filled ? -1 : 0;
    idx[e] = queue_idx(0, uint32_t(keys[e]));
  }
  for (size_t n = 0; n < N; ++n) sched[n * 4] = n < filled ? int32_t(n) : -1, sched[n * 4 + 1] = n < filled ? 0 : -1;
  c->s.reset_done = c->queue_ready = false;
  auto upload = [&](size_t) {
    mpcmmd_handle* h = c->s.h;
    HIPC(hipMemcpy(c->q.vel, vel.data(), E * 3 * 4, hipMemcpyHostToDevice));
    HIPC(hipMemcpy(const_cast<int32_t*>(h->p.idx_mpc), idx.data(), E * 4, hipMemcpyHostToDevice));
    HIPC(hipMemcpy(const_cast<float*>(h->p.v_des), vdes.data(), E * 4, hipMemcpyHostToDevice));
    if (O) {
      const std::vector<float> veh = rows(sc->vehicles, O * 4);
      HIPC(hipMemcpy(c->q.veh, veh.data(), E * O * 4 * 4, hipMemcpyHostToDevice));
    }
    if (planned && O) {
      const std::vector<float> tg = rows(sc->veh_target, O * 2), ac = rows(sc->veh_acc, O * 2);
      HIPC(hipMemcpy(const_cast<float*>(c->pv.target), tg.data(), E * O * 2 * 4, hipMemcpyHostToDevice));
      HIPC(hipMemcpy(c->pv.acc, ac.data(), E * O * 2 * 4, hipMemcpyHostToDevice));
    }
    Arena& a = c->queue;
    a.release();  // the last campaign's table
    MpcQueueParams& p = c->qp;
    p = MpcQueueParams{};
    p.E = n_slots, p.N = sc->n_scenes, p.ticks_per_episode = ticks_per_episode, p.O = int(O);
    p.tab_key = a.alloc<uint32_t>(N, sc->keys), p.tab_v_des = a.alloc<float>(N, sc->v_des);
    p.tab_pos = a.alloc<double>(N * 2, sc->pos), p.tab_vel = a.alloc<float>(N * 3, sc->vel);
    p.tab_veh = a.alloc<float>(N * O * 4, sc->vehicles), p.tab_mean = a.alloc<float>(N * 8, sc->mean);
    if (planned && O)
      p.tab_target = a.alloc<float>(N * O * 2, sc->veh_target), p.tab_acc = a.alloc<float>(N * O * 2, sc->veh_acc);
    p.pos = c->q.pos, p.vel = c->q.vel, p.veh = c->q.veh, p.mean = h->p.mean;
    p.target = const_cast<float*>(c->pv.target), p.acc = c->pv.acc;
    MpcQueueState& st = p.st;
    st.scene = a.alloc<int32_t>(E, scene.data()), st.ltick = a.alloc<int32_t>(E);
    HIPC(hipMemset(st.ltick, 0, E * 4));
    st.done = c->s.done, st.fresh = a.alloc<int32_t>(E, none.data()), st.key = c->s.keys_dev;
    st.idx_mpc = const_cast<int32_t*>(h->p.idx_mpc), st.v_des = const_cast<float*>(h->p.v_des);
    st.sched = a.alloc<int32_t>(N * 4, sched.data()), st.count = a.alloc<int32_t>(2, count.data());
  };
  c->queue_on = true;
  const int rc = reset_common(c->s, n_slots, pos.data(), mean.data(), cov, nullptr, keys.data(), [&] { sync_streams(c); },
                              upload, [&] {
    HIPC(hipMemcpy(c->s.done, done.data(), E * 4, hipMemcpyHostToDevice));  // the idle slots are frozen
    enqueue_step(c, -1, true);
    HIPC(hipStreamSynchronize(c->s.h->stream));
  });
  c->s.reset_done = false;  // an ordinary run needs an ordinary reset
  c->queue_ready = rc == MPCMMD_OK;
  return rc;
}

int mpcmmd_mpc_queue_run(mpcmmd_mpc* c, int32_t cost_kind, int32_t tick_begin, int32_t count, const float* cov) {
  if (!c || !cov) return fail(MPCMMD_E_INVALID, "null argument");
  if (int rc = queue_state(c, "mpcmmd_mpc_queue_run", true)) return rc;
  if (tick_begin < 0 || count < 0 || tick_begin + count > c->s.Tmax) return fail(MPCMMD_E_INVALID, "mpc: tick range");
  const std::vector<float> covs = replicate_cov(cov, c->s.E);
  for (int k = tick_begin; k < tick_begin + count; ++k) {
    if (int rc = begin_impl(c->s.h, c->s.E, cost_kind, nullptr, nullptr, nullptr, covs.data(), nullptr, nullptr, nullptr,
                            nullptr, nullptr, nullptr, true))
      return rc;
    if (int rc = mpcmmd_iterate(c->s.h, 0, c->s.h->T)) return rc;
    if (int rc = guarded([&] {
          enqueue_step(c, k, false);
          enqueue_queue(c, k);
          enqueue_step(c, k, true, true);  // st0, solve_c, obs, the population of the refilled slots
          return MPCMMD_OK;
        }))
      return rc;
  }
  return MPCMMD_OK;
}

int mpcmmd_mpc_queue_status(mpcmmd_mpc* c, int32_t* started, int32_t* finished) {
  if (!c || !started || !finished) return fail(MPCMMD_E_INVALID, "null argument");
  if (int rc = queue_state(c, "mpcmmd_mpc_queue_status", true)) return rc;
  return guarded([&] {
    check_device(c->s.h);
    sync_streams(c);
    int32_t count[2];
    HIPC(hipMemcpy(count, c->qp.st.count, sizeof count, hipMemcpyDeviceToHost));
    *started = count[0], *finished = count[1];
    return MPCMMD_OK;
  });
}

int mpcmmd_mpc_queue_log(mpcmmd_mpc* c, int32_t* sched) {
  if (!c || !sched) return fail(MPCMMD_E_INVALID, "null argument");
  if (int rc = queue_state(c, "mpcmmd_mpc_queue_log", true)) return rc;
  return guarded([&] {
    check_device(c->s.h);
    sync_streams(c);
    HIPC(hipMemcpy(sched, c->qp.st.sched, size_t(c->qp.N) * 16, hipMemcpyDeviceToHost));
    return MPCMMD_OK;
  });
}

}  // extern "C"
