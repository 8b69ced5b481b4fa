// libmpcmmd: the surrogate world on the device (include/mpcmmd.h).
// mpcmmd_world_step_device uploads the model and the episodes' arrays, runs
// k_world_step once and reads everything back: it holds the kernel against
// the host twin.  The world context (mpcmmd_world) keeps the model, the
// episodes' state, the variates and the log resident and chains, per tick, the
// tick context's begin, the CEM iterations and k_world_step on the handle's
// stream: the kernel reads the handle's result buffers and writes the tick
// context's input image, st0 and iteration 0's population, so nothing crosses
// the host between two solves.
#include <array>
#include <cstring>

#include "handle.hpp"
#include "rng.hpp"
#include "tick.hpp"
#include "world.hpp"
#include "world_draw.hpp"
#include "world_host.hpp"

using namespace mpcmmd;

struct mpcmmd_world {
  mpcmmd_tick* t = nullptr;
  mpcmmd_handle* h = nullptr;
  WorldScalars w{};
  int Tmax = 0, Emax = 0, E = 0;
  bool drawn = false;            // the variates are drawn in the kernel (no u given at the reset)
  std::vector<uint32_t> keys;    // [E] episode keys: idx_mpc = tick + key, and the variates' Philox key
  uint32_t* keys_dev = nullptr;  // [Emax]
  bool reset_done = false;
  std::vector<void*> bufs;  // every device allocation of the context
  WorldStepParams q{};      // the model's arrays and the state, filled at create
  float* u = nullptr;       // [Tmax][Emax][4]
  double* logd = nullptr;   // [Tmax][Emax][3]
  float* logf = nullptr;    // [Tmax][Emax][13]
  int32_t* logi = nullptr;  // [Tmax][Emax][4]
  float* plan = nullptr;    // [Tmax][Emax][34]
  double* chol = nullptr;   // [8][8]
  std::array<double, 64> chol_host{};
};

namespace {

template <class T>
T* world_alloc(mpcmmd_world* w, size_t count, const void* src = nullptr) {
  void* d = nullptr;
  HIPC(hipMalloc(&d, (count ? count : 4) * sizeof(T)));
  w->bufs.push_back(d);
  if (src && count) HIPC(hipMemcpy(d, src, count * sizeof(T), hipMemcpyHostToDevice));
  return static_cast<T*>(d);
}

// one k_world_step over the context's episodes: the plan from the handle's results of the last
// iteration, the next inputs into the tick context's image
void enqueue_step(mpcmmd_world* w, int tick, bool reset) {
  mpcmmd_handle* h = w->h;
  const TickLayout l = tick_layout_of(w->t);
  WorldStepParams q = w->q;
  q.tick = tick, q.reset = reset ? 1 : 0;
  const int T = h->T;
  float* res = h->p.results + size_t(T - 1) * kResultStride;
  q.cx = res, q.cy = res + 11, q.s_plan = T * kResultStride;
  q.steer = h->p.res_steer + size_t(T - 1) * kNum, q.s_steer = T * kNum;
  q.mean = h->p.mean;
  float* in = tick_inputs_device(w->t);
  q.init = in, q.xw = in + l.xw, q.yw = in + l.yw, q.obs = in + l.obs;
  q.s_init = q.s_wp = q.s_obs = l.stride;
  q.pop = h->p.pop;
  q.st0 = const_cast<float*>(h->p.st0);
  const size_t row = size_t(reset ? 0 : tick) * w->Emax;
  q.u = w->drawn ? nullptr : w->u + row * 4;
  q.key = w->keys_dev, q.seed = h->cfg.seed;
  q.logd = w->logd + row * 3, q.logf = w->logf + row * 13, q.logi = w->logi + row * 4;
  q.plan = w->plan + row * 34;
  q.chol = w->chol;
  launch_world_step(q, w->E, h->stream);
  HIPC(hipGetLastError());
}

}  // namespace

extern "C" {

int mpcmmd_world_create(mpcmmd_tick* t, const mpcmmd_world_model* m, int32_t max_ticks, mpcmmd_world** out) {
  if (!t || !m || !out) return fail(MPCMMD_E_INVALID, "null argument");
  *out = nullptr;
  if (m->num_path < 2 || m->num_path > 2048 || m->num_obs < 1 || m->num_obs > kWorldMaxObs || m->total_obs < 0 ||
      m->total_obs > kWorldMaxObs || m->num_route < 2 || m->goal_index < 0 || m->goal_index >= m->num_route ||
      (m->noise != 0 && m->noise != 1))
    return fail(MPCMMD_E_INVALID, "world model out of range (mpcmmd_world_model)");
  if (!m->route_x || !m->route_y || !m->route_arc || !m->spline_x || !m->spline_y || !m->pdot4)
    return fail(MPCMMD_E_INVALID, "world model: null array");
  mpcmmd_handle* h = tick_handle(t);
  if (m->num_path != tick_num_path(t)) return fail(MPCMMD_E_INVALID, "world: num_path is not the tick context's");
  if (m->num_obs != h->O) return fail(MPCMMD_E_INVALID, "world: num_obs is not the handle's");
  if (max_ticks < 1 || max_ticks > (1 << 20)) return fail(MPCMMD_E_INVALID, "world: 1 <= max_ticks <= 2^20");
  auto* w = new mpcmmd_world();
  w->t = t, w->h = h;
  w->Tmax = max_ticks, w->Emax = h->Gmax;
  int rc = guarded([&] {
    check_device(h);
    mpcmmd_world_model mm = *m;
    mm.num_batch = h->B;  // the handle's population and its own pop0 normals
    w->w = world_scalars(mm);
    const size_t n = size_t(m->num_route), E = size_t(w->Emax), V = size_t(m->total_obs), Tm = size_t(max_ticks);
    if (h->pop0_normals.empty())
      h->pop0_normals = host_normals(kFixedKey0, h->cfg.seed, kStreamPop0, 0, size_t(h->B) * 8);
    WorldStepParams& q = w->q;
    q.w = w->w;
    q.route_x = world_alloc<double>(w, n, m->route_x), q.route_y = world_alloc<double>(w, n, m->route_y);
    q.arc = world_alloc<double>(w, n, m->route_arc);
    q.sx = world_alloc<double>(w, 4 * (n - 1), m->spline_x), q.sy = world_alloc<double>(w, 4 * (n - 1), m->spline_y);
    q.pdot4 = world_alloc<double>(w, 44, m->pdot4);
    q.pop0 = world_alloc<float>(w, h->pop0_normals.size(), h->pop0_normals.data());
    w->chol = world_alloc<double>(w, 64);
    q.pos = world_alloc<double>(w, E * 2), q.ego = world_alloc<float>(w, E * 3);
    q.veh = world_alloc<float>(w, E * V * 5), q.done = world_alloc<int32_t>(w, E);
    w->u = world_alloc<float>(w, Tm * E * 4);
    w->keys_dev = world_alloc<uint32_t>(w, E);
    w->logd = world_alloc<double>(w, Tm * E * 3), w->logf = world_alloc<float>(w, Tm * E * 13);
    w->logi = world_alloc<int32_t>(w, Tm * E * 4), w->plan = world_alloc<float>(w, Tm * E * 34);
    return MPCMMD_OK;
  });
  if (rc != MPCMMD_OK) {
    mpcmmd_world_destroy(w);
    (void)hipGetLastError();
    return rc;
  }
  *out = w;
  return MPCMMD_OK;
}

void mpcmmd_world_destroy(mpcmmd_world* w) {
  if (!w) return;
  (void)hipSetDevice(w->h->device);
  if (w->h->stream) (void)hipStreamSynchronize(w->h->stream);  // the steps in flight
  for (void* d : w->bufs) (void)hipFree(d);
  delete w;
}

int mpcmmd_world_reset(mpcmmd_world* w, int32_t n_episodes, const double* pos, const float* ego,
                       const float* vehicles, const float* mean, const float* cov, const float* u,
                       const int32_t* keys) {
  if (!w || !pos || !ego || !mean || !cov || !keys || (w->w.total > 0 && !vehicles))
    return fail(MPCMMD_E_INVALID, "null argument");
  if (n_episodes < 1 || n_episodes > w->Emax)
    return fail(MPCMMD_E_INVALID, "world: n_episodes must be 1..max_configs of the handle");
  double cv[64];
  for (int i = 0; i < 64; ++i) cv[i] = double(cov[i]);
  if (!chol8(cv, w->chol_host.data())) return fail(MPCMMD_E_INVALID, "cov_param_init is not positive definite");
  return guarded([&] {
    mpcmmd_handle* h = w->h;
    check_device(h);
    HIPC(hipStreamSynchronize(h->stream));  // a reset starts over: nothing of the last run is in flight
    const size_t E = size_t(n_episodes), V = size_t(w->w.total);
    w->E = n_episodes, w->drawn = u == nullptr;
    w->keys.assign(keys, keys + E);
    HIPC(hipMemcpy(w->keys_dev, w->keys.data(), E * 4, hipMemcpyHostToDevice));
    const std::vector<int32_t> running(E, -1);
    HIPC(hipMemcpy(w->q.pos, pos, E * 2 * 8, hipMemcpyHostToDevice));
    HIPC(hipMemcpy(w->q.ego, ego, E * 3 * 4, hipMemcpyHostToDevice));
    if (V) HIPC(hipMemcpy(w->q.veh, vehicles, E * V * 5 * 4, hipMemcpyHostToDevice));
    HIPC(hipMemcpy(w->q.done, running.data(), E * 4, hipMemcpyHostToDevice));
    HIPC(hipMemcpy(w->chol, w->chol_host.data(), 64 * 8, hipMemcpyHostToDevice));
    HIPC(hipMemcpy(h->p.mean, mean, E * 8 * 4, hipMemcpyHostToDevice));
    if (u)  // [Tmax][n_episodes][4] -> rows of Emax, one strided copy
      HIPC(hipMemcpy2D(w->u, size_t(w->Emax) * 16, u, E * 16, E * 16, size_t(w->Tmax), hipMemcpyHostToDevice));
    enqueue_step(w, -1, true);  // tick 0's inputs, st0 and population from the start states
    w->reset_done = true;
    return MPCMMD_OK;
  });
}

int mpcmmd_world_run(mpcmmd_world* w, int32_t cost_kind, int32_t tick_begin, int32_t count, const float* cov,
                     const float* v_des, float threshold) {
  if (!w || !cov || !v_des) return fail(MPCMMD_E_INVALID, "null argument");
  if (!w->reset_done) return fail(MPCMMD_E_STATE, "mpcmmd_world_run before mpcmmd_world_reset");
  if (tick_begin < 0 || count < 0 || tick_begin + count > w->Tmax) return fail(MPCMMD_E_INVALID, "world: tick range");
  const int E = w->E;
  std::vector<int32_t> idx(E);
  std::vector<float> covs(size_t(E) * 64);
  for (int e = 0; e < E; ++e) std::memcpy(&covs[size_t(e) * 64], cov, 64 * 4);
  for (int k = tick_begin; k < tick_begin + count; ++k) {
    for (int e = 0; e < E; ++e) idx[e] = int32_t(uint32_t(k) + w->keys[e]);
    if (int rc = tick_begin_chained(w->t, E, cost_kind, idx.data(), covs.data(), v_des, threshold)) return rc;
    if (int rc = mpcmmd_iterate(w->h, 0, w->h->T)) return rc;
    if (int rc = guarded([&] {
          enqueue_step(w, k, false);
          return MPCMMD_OK;
        }))
      return rc;
  }
  return MPCMMD_OK;
}

int mpcmmd_world_log(mpcmmd_world* w, int32_t ticks, double* log_d, float* log_f, int32_t* log_i, float* plan,
                     int32_t* done_tick) {
  if (!w || !log_d || !log_f || !log_i || !plan || !done_tick) return fail(MPCMMD_E_INVALID, "null argument");
  if (ticks < 0 || ticks > w->Tmax) return fail(MPCMMD_E_INVALID, "world: tick range");
  return guarded([&] {
    check_device(w->h);
    HIPC(hipStreamSynchronize(w->h->stream));
    const size_t E = size_t(w->E), Em = size_t(w->Emax);
    // rows of Emax -> [ticks][n_episodes]: one strided copy per array
    auto back = [&](void* dst, const void* src, size_t row_bytes) {
      if (ticks > 0)
        HIPC(hipMemcpy2D(dst, E * row_bytes, src, Em * row_bytes, E * row_bytes, size_t(ticks), hipMemcpyDeviceToHost));
    };
    back(log_d, w->logd, 3 * 8), back(log_f, w->logf, 13 * 4), back(log_i, w->logi, 4 * 4), back(plan, w->plan, 34 * 4);
    HIPC(hipMemcpy(done_tick, w->q.done, E * 4, hipMemcpyDeviceToHost));
    return MPCMMD_OK;
  });
}

}  // extern "C"

// the host step: here, not in world_host.cpp, because the drawn variates need rng.hpp
extern "C" int mpcmmd_world_step_host(const mpcmmd_world_model* m, int32_t tick, const mpcmmd_world_step_io* io) {
  if (int rc = check_world(m, io)) return rc;
  world_step_host(*m, tick, *io, world_draw);
  return MPCMMD_OK;
}

extern "C" int mpcmmd_world_step_device(const mpcmmd_world_model* m, int32_t device, int32_t n_episodes, int32_t tick,
                                        const mpcmmd_world_step_io* io) {
  if (int rc = check_world(m, io)) return rc;
  if (n_episodes < 1 || n_episodes > 65535) return fail(MPCMMD_E_INVALID, "world: 1 <= n_episodes <= 65535");
  return guarded([&] {
    int count = 0;
    HIPC(hipGetDeviceCount(&count));
    if (device < 0 || device >= count) return fail(MPCMMD_E_INVALID, "world: no such device");
    HIPC(hipSetDevice(device));
    const size_t E = size_t(n_episodes), n = size_t(m->num_route), P = size_t(m->num_path), O = size_t(m->num_obs);
    const size_t B = size_t(m->num_batch), V = size_t(m->total_obs);
    Scratch sc;
    WorldStepParams q{};
    q.w = world_scalars(*m);
    q.tick = tick;
    q.s_plan = 11, q.s_steer = 4, q.s_init = 6, q.s_wp = int(P), q.s_obs = int(O) * 5;
    auto in = [&](const void* src, size_t bytes) { return sc.up(src, bytes); };
    q.route_x = static_cast<const double*>(in(m->route_x, n * 8));
    q.route_y = static_cast<const double*>(in(m->route_y, n * 8));
    q.arc = static_cast<const double*>(in(m->route_arc, n * 8));
    q.sx = static_cast<const double*>(in(m->spline_x, 4 * (n - 1) * 8));
    q.sy = static_cast<const double*>(in(m->spline_y, 4 * (n - 1) * 8));
    q.pdot4 = static_cast<const double*>(in(m->pdot4, 44 * 8));
    q.chol = static_cast<const double*>(in(m->chol, 64 * 8));
    q.pop0 = static_cast<const float*>(in(m->pop0, B * 8 * 4));
    q.cx = static_cast<const float*>(in(io->cx, E * 11 * 4));
    q.cy = static_cast<const float*>(in(io->cy, E * 11 * 4));
    q.steer = static_cast<const float*>(in(io->steer, E * 4 * 4));
    q.u = io->u ? static_cast<const float*>(in(io->u, E * 4 * 4)) : nullptr;
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
    q.ego = static_cast<float*>(io_buf(io->ego, E * 3 * 4, true));
    q.veh = static_cast<float*>(io_buf(io->vehicles, E * V * 5 * 4, true));
    q.done = static_cast<int32_t*>(io_buf(io->done_tick, E * 4, true));
    q.init = static_cast<float*>(io_buf(io->init_state, E * 6 * 4, false));
    q.xw = static_cast<float*>(io_buf(io->x_wp, E * P * 4, false));
    q.yw = static_cast<float*>(io_buf(io->y_wp, E * P * 4, false));
    q.obs = static_cast<float*>(io_buf(io->obstacles, E * O * 5 * 4, false));
    q.pop = static_cast<float*>(io_buf(io->pop, E * B * 8 * 4, false));
    q.logd = static_cast<double*>(io_buf(io->log_d, E * MPCMMD_WORLD_LOG_D * 8, false));
    q.logf = static_cast<float*>(io_buf(io->log_f, E * MPCMMD_WORLD_LOG_F * 4, false));
    q.logi = static_cast<int32_t*>(io_buf(io->log_i, E * MPCMMD_WORLD_LOG_I * 4, false));
    launch_world_step(q, n_episodes, nullptr);
    HIPC(hipGetLastError());
    HIPC(hipDeviceSynchronize());
    for (const Out& o : outs) HIPC(hipMemcpy(o.host, o.dev, o.bytes, hipMemcpyDeviceToHost));
    return MPCMMD_OK;
  });
}
