// libmpcmmd: the synthetic closed loop on the device (include/mpcmmd.h).
// mpcmmd_mpc_step_device uploads the model and the episodes' arrays, runs
// k_mpc_step once and reads everything back: it holds the kernel against the
// host twin.  The context (mpcmmd_mpc) keeps the model, the episodes' state,
// the variates and the log resident and chains, per tick, the resident begin
// (begin.hip), the CEM iterations and k_mpc_step on the handle's stream: the
// kernel reads the handle's result buffer and writes st0, solve_c, obs and
// iteration 0's population, so nothing crosses the host between two solves.
#include <array>
#include <cstring>

#include "handle.hpp"
#include "mpc.hpp"
#include "mpc_draw.hpp"
#include "mpc_host.hpp"
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
  launch_mpc_step(q, c->E, h->stream);
  HIPC(hipGetLastError());
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

int mpcmmd_mpc_step_device(const mpcmmd_mpc_model* m, int32_t device, int32_t n_episodes, int32_t tick,
                           const mpcmmd_mpc_step_io* io) {
  if (int rc = check_mpc(m, io)) return rc;
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
    launch_mpc_step(q, n_episodes, nullptr);
    HIPC(hipGetLastError());
    HIPC(hipDeviceSynchronize());
    for (const Out& o : outs) HIPC(hipMemcpy(o.host, o.dev, o.bytes, hipMemcpyDeviceToHost));
    return MPCMMD_OK;
  });
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
  for (void* d : c->bufs) (void)hipFree(d);
  delete c;
}

int mpcmmd_mpc_reset(mpcmmd_mpc* c, int32_t n_episodes, const double* pos, const float* vel, const float* vehicles,
                     const float* mean, const float* cov, const float* u, const int32_t* keys) {
  if (!c || !pos || !vel || !mean || !cov || !keys || (c->q.w.O > 0 && !vehicles))
    return fail(MPCMMD_E_INVALID, "null argument");
  if (n_episodes < 1 || n_episodes > c->Emax)
    return fail(MPCMMD_E_INVALID, "mpc: n_episodes must be 1..max_configs of the handle");
  double cv[64];
  for (int i = 0; i < 64; ++i) cv[i] = double(cov[i]);
  if (!chol8(cv, c->chol_host.data())) return fail(MPCMMD_E_INVALID, "cov_param_init is not positive definite");
  return guarded([&] {
    mpcmmd_handle* h = c->h;
    check_device(h);
    HIPC(hipStreamSynchronize(h->stream));  // a reset starts over: nothing of the last run is in flight
    const size_t E = size_t(n_episodes), O = size_t(c->q.w.O);
    c->E = n_episodes, c->drawn = u == nullptr;
    c->keys.assign(keys, keys + E);
    HIPC(hipMemcpy(c->keys_dev, c->keys.data(), E * 4, hipMemcpyHostToDevice));
    const std::vector<int32_t> running(E, -1);
    HIPC(hipMemcpy(c->q.pos, pos, E * 2 * 8, hipMemcpyHostToDevice));
    HIPC(hipMemcpy(c->q.vel, vel, E * 3 * 4, hipMemcpyHostToDevice));
    if (O) HIPC(hipMemcpy(c->q.veh, vehicles, E * O * 4 * 4, hipMemcpyHostToDevice));
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
    HIPC(hipStreamSynchronize(c->h->stream));
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

}  // extern "C"
