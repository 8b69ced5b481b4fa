// libmpcmmd: the synthetic closed loop on the device (include/mpcmmd.h).
// mpcmmd_mpc_step_device uploads the model and the episodes' arrays, runs
// k_mpc_step once and reads everything back: it holds the kernel against the
// host twin.  The context (mpcmmd_mpc) keeps the model, the episodes' state,
// the variates and the log resident and chains, per tick, the resident begin
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
#include <array>
#include <cmath>
#include <cstring>

#include "handle.hpp"
#include "mpc.hpp"
#include "mpc_draw.hpp"
#include "mpc_host.hpp"
#include "mpc_validate.hpp"
#include "rng.hpp"
#include "solve_host.hpp"

using namespace mpcmmd;

struct mpcmmd_mpc {
  mpcmmd_handle* h = nullptr;
  int Tmax = 0, Emax = 0, E = 0;
  bool drawn = false;            // the variates are drawn in the kernel (no u given at the reset)
  std::vector<uint32_t> keys;    // [E] episode keys: idx_mpc = tick + key, and the variates' Philox key
  uint32_t* keys_dev = nullptr;  // [Emax]
  bool reset_done = false;
  std::vector<void*> bufs;  // every device allocation of the context
  MpcStepParams q{};        // the model's arrays and the state, filled at create
  float* u = nullptr;       // [Tmax][Emax][3]
  double* logd = nullptr;   // [Tmax][Emax][2]
  float* logf = nullptr;    // [Tmax][Emax][12]
  int32_t* logi = nullptr;  // [Tmax][Emax][4]
  float* plan = nullptr;    // [Tmax][Emax][30]
  double* chol = nullptr;   // [8][8]
  std::array<double, 64> chol_host{};
  // the validation stage (off: val_on false, none of the buffers, streams or events exists)
  bool val_on = false;
  size_t val_first = 0;       // its allocations are bufs[val_first ..]
  int val_S = 0;              // bandwidths
  bool val_overlap = false;   // the validators' launches go to the side stream
  ValidateRiskParams vq{};    // the packed plan inputs (vq.roll), the costs and the statistics' scratch
  MpcValidateParams vp{};     // the packed inputs once more, as k_mpc_validate_prep writes them
  int32_t *vl_count = nullptr, *vl_lane = nullptr;  // [Tmax][Emax]
  int32_t* vl_pos = nullptr;                        // [Tmax][Emax][3]
  float *vl_var = nullptr, *vl_cvar = nullptr, *vl_mean = nullptr, *vl_max = nullptr;  // [Tmax][Emax][3]
  float* vl_mmd = nullptr;                          // [Tmax][Emax][3][S]
  float* vl_est = nullptr;                          // [Tmax][Emax][2]
  hipStream_t side = nullptr;                       // the validators' stream of an overlapped stage
  hipEvent_t ev_prep = nullptr, ev_done = nullptr;  // the prep is done; the side stream's tick is done
  bool side_pending = false;                        // ev_done was recorded since the last synchronisation
  // the planned vehicles (off: veh_on false, none of the buffers exists)
  bool veh_on = false;
  int veh_E = 0;                 // the episodes the staged arrays are for
  std::vector<void*> veh_bufs;   // the policy's device allocations
  MpcVehParams pv{};             // the constants, the live accelerations, the targets
  float* veh_acc0 = nullptr;     // [Emax][O][2] the staged accelerations every reset starts from
  float* veh_log = nullptr;      // [Tmax][Emax][O][6]
};

namespace {

template <class T>
T* mpc_alloc(mpcmmd_mpc* c, size_t count, const void* src = nullptr) {
  void* d = nullptr;
  HIPC(hipMalloc(&d, (count ? count : 4) * sizeof(T)));
  c->bufs.push_back(d);
  if (src && count) HIPC(hipMemcpy(d, src, count * sizeof(T), hipMemcpyHostToDevice));
  return static_cast<T*>(d);
}

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
  mpcmmd_handle* h = c->h;
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
  const size_t row = size_t(reset ? 0 : tick) * c->Emax;
  q.u = c->drawn ? nullptr : c->u + row * 3;
  q.key = c->keys_dev, q.seed = h->cfg.seed;
  q.logd = c->logd + row * 2, q.logf = c->logf + row * 12, q.logi = c->logi + row * 4;
  q.plan = c->plan + row * 30;
  q.chol = c->chol;
  if (c->veh_on) {
    MpcVehParams pv = c->pv;
    pv.log = c->veh_log + row * size_t(q.w.O) * 6;
    launch_mpc_step_planned(q, pv, c->E, h->stream);
  } else {
    launch_mpc_step(q, c->E, h->stream);
  }
  HIPC(hipGetLastError());
}

// the validation stage of tick `tick`, behind its CEM iterations and before its step (the step
// overwrites pos, vel and obs, the next solve the results): the packed inputs on the handle's
// stream, then mpcmmd_validate's and mpcmmd_validate_risk's launches with K = E and the results
// pointed at the tick's log row -- behind the prep, or on the side stream between two events
void enqueue_validation(mpcmmd_mpc* c, int tick) {
  mpcmmd_handle* h = c->h;
  const int T = h->T, E = c->E;
  const size_t row = size_t(tick) * c->Emax;
  if (c->side_pending) {  // the previous tick's validators still own the packed inputs, the costs and the scratch
    HIPC(hipStreamWaitEvent(h->stream, c->ev_done, 0));
    c->side_pending = false;
  }
  MpcValidateParams p = c->vp;
  p.tick = tick;
  p.res = h->p.results + size_t(T - 1) * kResultStride, p.s_res = T * kResultStride;
  p.pos = c->q.pos, p.vel = c->q.vel;
  p.obs = h->p.obs;
  p.key = c->keys_dev;
  p.est = c->vl_est + row * 2;
  launch_mpc_validate_prep(p, E, h->stream);
  HIPC(hipGetLastError());
  hipStream_t s = h->stream;
  if (c->val_overlap) {
    HIPC(hipEventRecord(c->ev_prep, h->stream));
    HIPC(hipStreamWaitEvent(c->side, c->ev_prep, 0));
    s = c->side;
  }
  ValidateRiskParams q = c->vq;
  q.K = q.roll.K = E;
  ValidateParams v = q.roll;
  v.count = c->vl_count + row, v.count_lane = c->vl_lane + row;
  launch_validate(v, s);
  HIPC(hipGetLastError());
  q.count_pos = c->vl_pos + row * 3;
  q.var = c->vl_var + row * 3, q.cvar = c->vl_cvar + row * 3;
  q.mean = c->vl_mean + row * 3, q.vmax = c->vl_max + row * 3;
  q.mmd = c->val_S ? c->vl_mmd + row * 3 * c->val_S : nullptr;
  launch_vrisk_roll(q, s);
  HIPC(hipGetLastError());
  launch_vrisk_stats(q, s);
  HIPC(hipGetLastError());
  launch_vrisk_mmd(q, s);
  HIPC(hipGetLastError());
  if (c->val_overlap) {
    HIPC(hipEventRecord(c->ev_done, c->side));
    c->side_pending = true;
  }
}

// the handle's stream and the side stream idle
void sync_streams(mpcmmd_mpc* c) {
  HIPC(hipStreamSynchronize(c->h->stream));
  if (c->side) HIPC(hipStreamSynchronize(c->side));
  c->side_pending = false;
}

// frees the validation stage's buffers (the last allocations of the context), its stream and events
void drop_validation(mpcmmd_mpc* c) {
  if (!c->val_on) return;
  for (size_t i = c->val_first; i < c->bufs.size(); ++i) (void)hipFree(c->bufs[i]);
  c->bufs.resize(c->val_first);
  if (c->ev_prep) (void)hipEventDestroy(c->ev_prep);
  if (c->ev_done) (void)hipEventDestroy(c->ev_done);
  if (c->side) (void)hipStreamDestroy(c->side);
  c->ev_prep = c->ev_done = nullptr, c->side = nullptr;
  c->side_pending = false;
  c->val_on = false;
}

// frees the vehicle policy's buffers
void drop_vehicles(mpcmmd_mpc* c) {
  for (void* d : c->veh_bufs) (void)hipFree(d);
  c->veh_bufs.clear();
  c->pv = MpcVehParams{};
  c->veh_acc0 = c->veh_log = nullptr;
  c->veh_on = false, c->veh_E = 0;
}

template <class T>
T* veh_alloc(mpcmmd_mpc* c, size_t count, const void* src = nullptr) {
  void* d = nullptr;
  HIPC(hipMalloc(&d, (count ? count : 4) * sizeof(T)));
  c->veh_bufs.push_back(d);
  if (src && count) HIPC(hipMemcpy(d, src, count * sizeof(T), hipMemcpyHostToDevice));
  return static_cast<T*>(d);
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
                const mpcmmd_mpc_step_io* io, const mpcmmd_mpc_planned* pl);

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

}  // extern "C"

namespace {

int step_device(const mpcmmd_mpc_model* m, int32_t device, int32_t n_episodes, int32_t tick,
                const mpcmmd_mpc_step_io* io, const mpcmmd_mpc_planned* pl) {
  if (n_episodes < 1 || n_episodes > 65535) return fail(MPCMMD_E_INVALID, "mpc: 1 <= n_episodes <= 65535");
  return guarded([&] {
    int count = 0;
    HIPC(hipGetDeviceCount(&count));
    if (device < 0 || device >= count) return fail(MPCMMD_E_INVALID, "mpc: no such device");
    HIPC(hipSetDevice(device));
    const size_t E = size_t(n_episodes), O = size_t(m->num_obs), B = size_t(m->num_batch);
    Scratch sc;
    MpcStepParams q{};
    q.w = mpc_scalars(*m);
    q.tick = tick;
    q.s_plan = 11, q.H = 0;
    auto in = [&](const void* src, size_t bytes) { return sc.up(src, bytes); };
    q.pdot2 = static_cast<const double*>(in(m->pdot2, 22 * 8));
    q.pddot1 = static_cast<const double*>(in(m->pddot1, 11 * 8));
    q.chol = static_cast<const double*>(in(m->chol, 64 * 8));
    q.pop0 = static_cast<const float*>(in(m->pop0, B * 8 * 4));
    q.cx = static_cast<const float*>(in(io->cx, E * 11 * 4));
    q.cy = static_cast<const float*>(in(io->cy, E * 11 * 4));
    q.u = io->u ? static_cast<const float*>(in(io->u, E * 3 * 4)) : nullptr;
    q.key = io->key ? static_cast<const uint32_t*>(in(io->key, E * 4)) : nullptr;
    q.seed = m->seed;
    q.mean = static_cast<const float*>(in(io->mean, E * 8 * 4));
    // state: in and out; a world without vehicles still gets a pointer
    struct Out {
      void* dev;
      void* host;
      size_t bytes;
    };
    std::vector<Out> outs;
    auto io_buf = [&](void* host, size_t bytes, bool upload) {
      void* d = sc.up(upload && bytes ? host : nullptr, bytes ? bytes : 16);
      if (bytes) outs.push_back({d, host, bytes});
      return d;
    };
    q.pos = static_cast<double*>(io_buf(io->pos, E * 2 * 8, true));
    q.vel = static_cast<float*>(io_buf(io->vel, E * 3 * 4, true));
    q.veh = static_cast<float*>(io_buf(io->vehicles, E * O * 4 * 4, true));
    q.done = static_cast<int32_t*>(io_buf(io->done_tick, E * 4, true));
    q.init = static_cast<float*>(io_buf(io->init_state, E * 6 * 4, false));
    q.st0 = static_cast<float*>(io_buf(io->st0, E * 8 * 4, false));
    q.x_obs = static_cast<float*>(io_buf(io->x_obs, E * O * kMpcTrack * 4, false));
    q.y_obs = static_cast<float*>(io_buf(io->y_obs, E * O * kMpcTrack * 4, false));
    q.pop = static_cast<float*>(io_buf(io->pop, E * B * 8 * 4, false));
    q.logd = static_cast<double*>(io_buf(io->log_d, E * MPCMMD_MPC_LOG_D * 8, false));
    q.logf = static_cast<float*>(io_buf(io->log_f, E * MPCMMD_MPC_LOG_F * 4, false));
    q.logi = static_cast<int32_t*>(io_buf(io->log_i, E * MPCMMD_MPC_LOG_I * 4, false));
    if (pl) {
      const MpcVehTables t = mpc_vehicle_tables(m->dt);
      MpcVehParams pv{};
      pv.k = upload_vehicle_consts(
          t, [&](const double* src, size_t n) { return static_cast<const double*>(in(src, n * 8)); });
      pv.target = static_cast<const float*>(in(pl->veh_target, E * O * 2 * 4));
      pv.acc = static_cast<float*>(io_buf(pl->veh_acc, E * O * 2 * 4, true));
      pv.log = pl->veh_log ? static_cast<float*>(io_buf(pl->veh_log, E * O * 6 * 4, false)) : nullptr;
      launch_mpc_step_planned(q, pv, n_episodes, nullptr);
    } else {
      launch_mpc_step(q, n_episodes, nullptr);
    }
    HIPC(hipGetLastError());
    HIPC(hipDeviceSynchronize());
    for (const Out& o : outs) HIPC(hipMemcpy(o.host, o.dev, o.bytes, hipMemcpyDeviceToHost));
    return MPCMMD_OK;
  });
}

}  // namespace

extern "C" {

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
  c->h = h;
  c->Tmax = max_ticks, c->Emax = h->Gmax;
  int rc = guarded([&] {
    check_device(h);
    const size_t E = size_t(c->Emax), O = size_t(m->num_obs), Tm = size_t(max_ticks);
    if (h->pop0_normals.empty())
      h->pop0_normals = host_normals(kFixedKey0, h->cfg.seed, kStreamPop0, 0, size_t(h->B) * 8);
    const std::vector<double> kc = kkt_columns(h->pc);
    MpcStepParams& q = c->q;
    q.w = mpc_scalars(mm);
    q.pdot2 = mpc_alloc<double>(c, 22, m->pdot2), q.pddot1 = mpc_alloc<double>(c, 11, m->pddot1);
    q.kcol = mpc_alloc<double>(c, kc.size(), kc.data());
    q.pop0 = mpc_alloc<float>(c, h->pop0_normals.size(), h->pop0_normals.data());
    c->chol = mpc_alloc<double>(c, 64);
    q.pos = mpc_alloc<double>(c, E * 2), q.vel = mpc_alloc<float>(c, E * 3);
    q.veh = mpc_alloc<float>(c, E * O * 4), q.done = mpc_alloc<int32_t>(c, E);
    c->u = mpc_alloc<float>(c, Tm * E * 3);
    c->keys_dev = mpc_alloc<uint32_t>(c, E);
    c->logd = mpc_alloc<double>(c, Tm * E * 2), c->logf = mpc_alloc<float>(c, Tm * E * 12);
    c->logi = mpc_alloc<int32_t>(c, Tm * E * 4), c->plan = mpc_alloc<float>(c, Tm * E * 30);
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
  (void)hipSetDevice(c->h->device);
  if (c->h->stream) (void)hipStreamSynchronize(c->h->stream);  // the steps in flight
  if (c->side) (void)hipStreamSynchronize(c->side);            // and the validators
  drop_validation(c);
  drop_vehicles(c);
  for (void* d : c->bufs) (void)hipFree(d);
  delete c;
}

int mpcmmd_mpc_reset(mpcmmd_mpc* c, int32_t n_episodes, const double* pos, const float* vel, const float* vehicles,
                     const float* mean, const float* cov, const float* u, const int32_t* keys) {
  if (!c || !pos || !vel || !mean || !cov || !keys || (c->q.w.O > 0 && !vehicles))
    return fail(MPCMMD_E_INVALID, "null argument");
  if (n_episodes < 1 || n_episodes > c->Emax)
    return fail(MPCMMD_E_INVALID, "mpc: n_episodes must be 1..max_configs of the handle");
  if (c->veh_on && n_episodes != c->veh_E)
    return fail(MPCMMD_E_INVALID, "mpc: n_episodes is not the one mpcmmd_mpc_plan_vehicles staged");
  double cv[64];
  for (int i = 0; i < 64; ++i) cv[i] = double(cov[i]);
  if (!chol8(cv, c->chol_host.data())) return fail(MPCMMD_E_INVALID, "cov_param_init is not positive definite");
  return guarded([&] {
    mpcmmd_handle* h = c->h;
    check_device(h);
    sync_streams(c);  // a reset starts over: nothing of the last run is in flight
    const size_t E = size_t(n_episodes), O = size_t(c->q.w.O);
    c->E = n_episodes, c->drawn = u == nullptr;
    c->keys.assign(keys, keys + E);
    HIPC(hipMemcpy(c->keys_dev, c->keys.data(), E * 4, hipMemcpyHostToDevice));
    const std::vector<int32_t> running(E, -1);
    HIPC(hipMemcpy(c->q.pos, pos, E * 2 * 8, hipMemcpyHostToDevice));
    HIPC(hipMemcpy(c->q.vel, vel, E * 3 * 4, hipMemcpyHostToDevice));
    if (O) HIPC(hipMemcpy(c->q.veh, vehicles, E * O * 4 * 4, hipMemcpyHostToDevice));
    if (c->veh_on && O) HIPC(hipMemcpy(c->pv.acc, c->veh_acc0, E * O * 2 * 4, hipMemcpyDeviceToDevice));
    HIPC(hipMemcpy(c->q.done, running.data(), E * 4, hipMemcpyHostToDevice));
    HIPC(hipMemcpy(c->chol, c->chol_host.data(), 64 * 8, hipMemcpyHostToDevice));
    HIPC(hipMemcpy(h->p.mean, mean, E * 8 * 4, hipMemcpyHostToDevice));
    if (u)  // [Tmax][n_episodes][3] -> rows of Emax, one strided copy
      HIPC(hipMemcpy2D(c->u, size_t(c->Emax) * 12, u, E * 12, E * 12, size_t(c->Tmax), hipMemcpyHostToDevice));
    enqueue_step(c, -1, true);  // tick 0's st0, solve_c, obs and population from the start states
    HIPC(hipStreamSynchronize(h->stream));
    c->reset_done = true;
    return MPCMMD_OK;
  });
}

int mpcmmd_mpc_run(mpcmmd_mpc* c, int32_t cost_kind, int32_t tick_begin, int32_t count, const float* cov,
                   const float* v_des) {
  if (!c || !cov || !v_des) return fail(MPCMMD_E_INVALID, "null argument");
  if (!c->reset_done) return fail(MPCMMD_E_STATE, "mpcmmd_mpc_run before mpcmmd_mpc_reset");
  if (tick_begin < 0 || count < 0 || tick_begin + count > c->Tmax) return fail(MPCMMD_E_INVALID, "mpc: tick range");
  const int E = c->E;
  std::vector<int32_t> idx(E);
  std::vector<float> covs(size_t(E) * 64);
  for (int e = 0; e < E; ++e) std::memcpy(&covs[size_t(e) * 64], cov, 64 * 4);
  for (int k = tick_begin; k < tick_begin + count; ++k) {
    for (int e = 0; e < E; ++e) idx[e] = int32_t(uint32_t(k) + c->keys[e]);
    if (int rc = begin_impl(c->h, E, cost_kind, idx.data(), nullptr, nullptr, covs.data(), nullptr, nullptr, v_des,
                            nullptr, nullptr, nullptr, true))
      return rc;
    if (int rc = mpcmmd_iterate(c->h, 0, c->h->T)) return rc;
    if (int rc = guarded([&] {
          if (c->val_on) enqueue_validation(c, k);
          enqueue_step(c, k, false);
          return MPCMMD_OK;
        }))
      return rc;
  }
  return MPCMMD_OK;
}

int mpcmmd_mpc_log(mpcmmd_mpc* c, int32_t ticks, double* log_d, float* log_f, int32_t* log_i, float* plan,
                   int32_t* done_tick) {
  if (!c || !log_d || !log_f || !log_i || !plan || !done_tick) return fail(MPCMMD_E_INVALID, "null argument");
  if (ticks < 0 || ticks > c->Tmax) return fail(MPCMMD_E_INVALID, "mpc: tick range");
  return guarded([&] {
    check_device(c->h);
    sync_streams(c);
    const size_t E = size_t(c->E), Em = size_t(c->Emax);
    // rows of Emax -> [ticks][n_episodes]: one strided copy per array
    auto back = [&](void* dst, const void* src, size_t row_bytes) {
      if (ticks > 0 && E > 0)
        HIPC(hipMemcpy2D(dst, E * row_bytes, src, Em * row_bytes, E * row_bytes, size_t(ticks), hipMemcpyDeviceToHost));
    };
    back(log_d, c->logd, 2 * 8), back(log_f, c->logf, 12 * 4), back(log_i, c->logi, 4 * 4), back(plan, c->plan, 30 * 4);
    if (E > 0) HIPC(hipMemcpy(done_tick, c->q.done, E * 4, hipMemcpyDeviceToHost));
    return MPCMMD_OK;
  });
}

int mpcmmd_mpc_validate(mpcmmd_mpc* c, const mpcmmd_mpc_validation* cfg) {
  if (!c) return fail(MPCMMD_E_INVALID, "null argument");
  mpcmmd_handle* h = c->h;
  const int O = h->O, H = h->H;
  ValidateRiskParams q{};
  if (cfg) {
    const int R = cfg->num_rollouts, S = cfg->num_sigma;
    if (R < 1 || R > (1 << 20)) return fail(MPCMMD_E_INVALID, "mpc validation: num_rollouts out of 1..2^20");
    if (!(cfg->alpha >= 0.0f && cfg->alpha <= 1.0f))
      return fail(MPCMMD_E_INVALID, "mpc validation: alpha out of [0, 1]");
    if (S < 0 || S > kRiskMaxSigma) return fail(MPCMMD_E_INVALID, "mpc validation: num_sigma out of [0, 8]");
    for (int i = 0; i < S; ++i)
      if (!(std::isfinite(cfg->sigma[i]) && cfg->sigma[i] > 0.0f))
        return fail(MPCMMD_E_INVALID, "mpc validation: every sigma must be finite and > 0");
    if (cfg->overlap != 0 && cfg->overlap != 1) return fail(MPCMMD_E_INVALID, "mpc validation: overlap must be 0 or 1");
    if (!validate_shape_ok(O, H))
      return fail(MPCMMD_E_INVALID, "mpc validation: the validators take 1 <= num_obs <= 32 and 2 <= num_prime <= 100");
    q.R = q.roll.R = R, q.S = S;
    if (mpcmmd_quantile_position(R, cfg->alpha, &q.lo, &q.hi, &q.w_lo, &q.w_hi) != MPCMMD_OK)
      return fail(MPCMMD_E_INVALID, "mpc validation: quantile position");
  }
  const int rc = guarded([&] {
    check_device(h);
    sync_streams(c);  // nothing in flight reads the buffers about to go
    drop_validation(c);
    c->reset_done = false;  // the stage changes with the episodes: the next run needs a reset
    if (!cfg) return MPCMMD_OK;
    c->val_first = c->bufs.size();
    c->val_on = true;  // from here on drop_validation frees what exists
    c->val_S = q.S, c->val_overlap = cfg->overlap == 1;
    HIPC(hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking));
    HIPC(hipEventCreateWithFlags(&c->ev_prep, hipEventDisableTiming));
    HIPC(hipEventCreateWithFlags(&c->ev_done, hipEventDisableTiming));
    const size_t Em = size_t(c->Emax), Tm = size_t(c->Tmax), R = size_t(q.R), S = size_t(q.S);
    const size_t n3 = 3 * Em, tiles = (R + kRiskTile - 1) / kRiskTile;
    const ProblemConsts& pc = h->pc;
    const mpcmmd_config& hc = h->cfg;
    ValidateParams& v = q.roll;  // as plan_params (validate_api.hip)
    v.O = O, v.H = H, v.noise = hc.noise;
    v.noise_level = hc.noise_level, v.acc_const = hc.acc_const_noise, v.steer_const = hc.steer_const_noise;
    v.K_steer = pc.K_steer, v.y_lb = pc.y_lb, v.y_ub = pc.y_ub, v.seed = hc.seed;
    const std::vector<float> basis = pack_basis(pc);  // P, Pdot, Pddot
    v.Pdot = mpc_alloc<float>(c, size_t(kNum) * kNvar, basis.data() + kNum * kNvar);
    v.Pddot = mpc_alloc<float>(c, size_t(kNum) * kNvar, basis.data() + 2 * kNum * kNvar);
    MpcValidateParams& p = c->vp;
    p = MpcValidateParams{};
    p.H = H, p.O = O;
    v.cx = p.cx = mpc_alloc<double>(c, Em * kNvar), v.cy = p.cy = mpc_alloc<double>(c, Em * kNvar);
    v.init_state = p.init = mpc_alloc<double>(c, Em * 6);
    v.x_obs = p.x_obs = mpc_alloc<float>(c, Em * O * kMpcTrack);
    v.y_obs = p.y_obs = mpc_alloc<float>(c, Em * O * kMpcTrack);
    v.keys = p.keys = mpc_alloc<uint32_t>(c, Em);
    v.draws = nullptr;
    q.costs = mpc_alloc<float>(c, n3 * R);  // every element is stored by its rollout's thread
    q.np = mpc_alloc<int32_t>(c, n3);
    if (S > 0) {
      std::vector<float> sg(Em * S);
      for (size_t i = 0; i < sg.size(); ++i) sg[i] = cfg->sigma[i % S];
      q.sigma = mpc_alloc<float>(c, sg.size(), sg.data());
      q.u = mpc_alloc<float>(c, n3 * R);
      q.part = mpc_alloc<double>(c, n3 * tiles * S);
    }
    c->vq = q;
    const size_t rows = Tm * Em;
    c->vl_count = mpc_alloc<int32_t>(c, rows), c->vl_lane = mpc_alloc<int32_t>(c, rows);
    c->vl_pos = mpc_alloc<int32_t>(c, rows * 3);
    c->vl_var = mpc_alloc<float>(c, rows * 3), c->vl_cvar = mpc_alloc<float>(c, rows * 3);
    c->vl_mean = mpc_alloc<float>(c, rows * 3), c->vl_max = mpc_alloc<float>(c, rows * 3);
    c->vl_mmd = mpc_alloc<float>(c, rows * 3 * S), c->vl_est = mpc_alloc<float>(c, rows * 2);
    return MPCMMD_OK;
  });
  if (rc != MPCMMD_OK) {  // a failed allocation leaves no half-made stage
    drop_validation(c);
    (void)hipGetLastError();
  }
  return rc;
}

int mpcmmd_mpc_validation_log(mpcmmd_mpc* c, int32_t ticks, int32_t* counts, int32_t* count_pos, float* stats,
                              float* mmd, float* est) {
  if (!c || !counts || !count_pos || !stats || !est) return fail(MPCMMD_E_INVALID, "null argument");
  if (c->val_on && c->val_S > 0 && !mmd) return fail(MPCMMD_E_INVALID, "null argument");
  if (ticks < 0 || ticks > c->Tmax) return fail(MPCMMD_E_INVALID, "mpc: tick range");
  if (!c->val_on) return fail(MPCMMD_E_STATE, "mpcmmd_mpc_validation_log without a validation stage");
  return guarded([&] {
    check_device(c->h);
    sync_streams(c);
    if (ticks == 0 || c->E == 0) return MPCMMD_OK;
    const size_t E = size_t(c->E), Em = size_t(c->Emax), n = size_t(ticks) * E, S = size_t(c->val_S);
    // rows of Emax -> [ticks][n_episodes]: one strided copy per array
    auto back = [&](void* dst, const void* src, size_t row_bytes) {
      HIPC(hipMemcpy2D(dst, E * row_bytes, src, Em * row_bytes, E * row_bytes, size_t(ticks), hipMemcpyDeviceToHost));
    };
    std::vector<int32_t> c2(n * 2);
    back(c2.data(), c->vl_count, 4), back(c2.data() + n, c->vl_lane, 4);
    for (size_t i = 0; i < n; ++i)
      for (size_t k = 0; k < 2; ++k) counts[i * 2 + k] = c2[k * n + i];
    std::vector<float> s4(n * 12);
    back(s4.data(), c->vl_var, 12), back(s4.data() + n * 3, c->vl_cvar, 12);
    back(s4.data() + n * 6, c->vl_mean, 12), back(s4.data() + n * 9, c->vl_max, 12);
    for (size_t i = 0; i < n; ++i)
      for (size_t k = 0; k < 4; ++k) std::memcpy(stats + (i * 4 + k) * 3, &s4[(k * n + i) * 3], 12);
    back(count_pos, c->vl_pos, 12), back(est, c->vl_est, 8);
    if (S > 0) back(mmd, c->vl_mmd, 12 * S);
    return MPCMMD_OK;
  });
}

int mpcmmd_mpc_validation_inputs(mpcmmd_mpc* c, double* cx, double* cy, double* init_state, float* x_obs,
                                 float* y_obs, uint32_t* keys) {
  if (!c) return fail(MPCMMD_E_INVALID, "null argument");
  if (!c->val_on) return fail(MPCMMD_E_STATE, "mpcmmd_mpc_validation_inputs without a validation stage");
  return guarded([&] {
    check_device(c->h);
    sync_streams(c);
    const size_t E = size_t(c->E), O = size_t(c->vp.O);
    auto back = [&](void* dst, const void* src, size_t bytes) {
      if (dst && bytes) HIPC(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    };
    back(cx, c->vp.cx, E * kNvar * 8), back(cy, c->vp.cy, E * kNvar * 8), back(init_state, c->vp.init, E * 6 * 8);
    back(x_obs, c->vp.x_obs, E * O * kMpcTrack * 4), back(y_obs, c->vp.y_obs, E * O * kMpcTrack * 4);
    back(keys, c->vp.keys, E * 4);
    return MPCMMD_OK;
  });
}

int mpcmmd_mpc_plan_vehicles(mpcmmd_mpc* c, int32_t n_episodes, const float* veh_target, const float* veh_acc) {
  if (!c) return fail(MPCMMD_E_INVALID, "null argument");
  MpcVehTables t{};
  if (veh_target) {
    if (n_episodes < 1 || n_episodes > c->Emax)
      return fail(MPCMMD_E_INVALID, "mpc: n_episodes must be 1..max_configs of the handle");
    if (!(c->q.w.dt < 15.0f)) return fail(MPCMMD_E_INVALID, "mpc vehicles: 0 < dt < 15");
    try {
      t = mpc_vehicle_tables(c->q.w.dt);
    } catch (const std::exception& e) {
      return fail(MPCMMD_E_INVALID, e.what());
    }
  }
  const int rc = guarded([&] {
    check_device(c->h);
    sync_streams(c);  // nothing in flight reads the buffers about to go
    drop_vehicles(c);
    c->reset_done = false;  // the policy changes with the episodes: the next run needs a reset
    if (!veh_target) return MPCMMD_OK;
    const size_t Em = size_t(c->Emax), Tm = size_t(c->Tmax), O = size_t(c->q.w.O), n = size_t(n_episodes) * O * 2;
    c->pv.k = upload_vehicle_consts(t, [&](const double* src, size_t cnt) { return veh_alloc<double>(c, cnt, src); });
    c->pv.target = veh_alloc<float>(c, Em * O * 2, nullptr);
    c->pv.acc = veh_alloc<float>(c, Em * O * 2);
    c->veh_acc0 = veh_alloc<float>(c, Em * O * 2);
    c->veh_log = veh_alloc<float>(c, Tm * Em * O * 6);
    if (n) {
      HIPC(hipMemcpy(const_cast<float*>(c->pv.target), veh_target, n * 4, hipMemcpyHostToDevice));
      if (veh_acc) HIPC(hipMemcpy(c->veh_acc0, veh_acc, n * 4, hipMemcpyHostToDevice));
      else HIPC(hipMemset(c->veh_acc0, 0, n * 4));
    }
    c->veh_E = n_episodes;
    c->veh_on = true;
    return MPCMMD_OK;
  });
  if (rc != MPCMMD_OK) {  // a failed allocation leaves no half-made policy
    drop_vehicles(c);
    (void)hipGetLastError();
  }
  return rc;
}

int mpcmmd_mpc_vehicle_log(mpcmmd_mpc* c, int32_t ticks, float* veh) {
  if (!c || !veh) return fail(MPCMMD_E_INVALID, "null argument");
  if (ticks < 0 || ticks > c->Tmax) return fail(MPCMMD_E_INVALID, "mpc: tick range");
  if (!c->veh_on) return fail(MPCMMD_E_STATE, "mpcmmd_mpc_vehicle_log without the vehicle policy");
  return guarded([&] {
    check_device(c->h);
    sync_streams(c);
    const size_t row = size_t(c->q.w.O) * 6 * 4, E = size_t(c->E), Em = size_t(c->Emax);
    if (ticks > 0 && E > 0 && row > 0)  // rows of Emax -> [ticks][n_episodes]: one strided copy
      HIPC(hipMemcpy2D(veh, E * row, c->veh_log, Em * row, E * row, size_t(ticks), hipMemcpyDeviceToHost));
    return MPCMMD_OK;
  });
}

}  // extern "C"
