// libmpcmmd: the surrogate world on the device (include/mpcmmd.h).
// mpcmmd_world_step_device uploads the model and the episodes' arrays, runs
// k_world_step once and reads everything back: it holds the kernel against
// the host twin.  The world context (mpcmmd_world) keeps the model, the
// episodes' state, the variates and the log resident and chains, per tick, the
// tick context's begin, the CEM iterations and k_world_step on the handle's
// stream: the kernel reads the handle's result buffers and writes the tick
// context's input image, st0 and iteration 0's population, so nothing crosses
// the host between two solves.  With a validation stage configured
// (mpcmmd_world_validate) each tick also enqueues, between
// its CEM iterations and its world step, the Monte-Carlo risk of the plan it
// just made: k_world_validate_prep packs the validators' inputs from the device
// buffers the solve used, then mpcmmd_validate_carla_risk's own launches write
// the tick's row of the validation log.  With routed vehicles configured
// (mpcmmd_world_route_vehicles) the reset's and every
// tick's step is the routed instantiation of k_world_step: the states, the
// parameters and the vehicle log live in the context.
#include <array>
#include <cmath>
#include <cstring>

#include "handle.hpp"
#include "rng.hpp"
#include "tick.hpp"
#include "world.hpp"
#include "world_draw.hpp"
#include "world_host.hpp"
#include "world_validate.hpp"

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
  // the validation stage (off: val_on false, none of the buffers exists)
  bool val_on = false;
  size_t val_first = 0;        // its allocations are bufs[val_first ..]
  int val_S = 0, val_lds = 0;  // bandwidths; the device's LDS per workgroup
  size_t val_nacc = 0;         // words of cnt_oh | cnt_lane
  ValidateCarlaParams vv{};    // the packed inputs, the accumulators and the costs
  ValidateRiskParams vq{};     // the statistics' scratch (the results point into the log per tick)
  WorldValidateParams vp{};    // the packed inputs once more, as k_world_validate_prep writes them
  int32_t *vl_count = nullptr, *vl_lane = nullptr, *vl_rows = nullptr;  // [Tmax][Emax]
  int32_t* vl_pos = nullptr;                                            // [Tmax][Emax][3]
  float *vl_var = nullptr, *vl_cvar = nullptr, *vl_mean = nullptr, *vl_max = nullptr;  // [Tmax][Emax][3]
  float* vl_mmd = nullptr;                                              // [Tmax][Emax][3][S]
  float* vl_est = nullptr;                                              // [Tmax][Emax][2]
  // the routed vehicles (off: veh_on false, none of the buffers exists)
  bool veh_on = false;
  int veh_E = 0;                // the episodes the staged arrays are for
  std::vector<void*> veh_bufs;  // the policy's device allocations
  WorldRoutedParams rv{};       // scalars, states [E][V], parameters
  double* veh_s0 = nullptr;     // [E][V] the staged start states
  float* veh_v0 = nullptr;
  double* veh_log_s = nullptr;  // [Tmax][Emax][V]
  float* veh_log = nullptr;     // [Tmax][Emax][V][2]
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
  if (w->veh_on) {
    WorldRoutedParams r = w->rv;
    r.log = w->veh_log + row * size_t(q.w.total) * 2, r.log_s = w->veh_log_s + row * size_t(q.w.total);
    launch_world_step_routed(q, r, w->E, h->stream);
  } else {
    launch_world_step(q, w->E, h->stream);
  }
  HIPC(hipGetLastError());
}

// the validation stage of tick `tick`, behind its CEM iterations and before its world step (the
// step overwrites the input image and st0): the packed inputs, the zeroed accumulators, then
// mpcmmd_validate_carla_risk's launches with K = E and the results pointed at the tick's log row
void enqueue_validation(mpcmmd_world* w, int tick) {
  mpcmmd_handle* h = w->h;
  const TickLayout l = tick_layout_of(w->t);
  const int T = h->T, E = w->E;
  const size_t row = size_t(tick) * w->Emax;
  WorldValidateParams p = w->vp;
  p.tick = tick;
  p.res = h->p.results + size_t(T - 1) * kResultStride, p.s_res = T * kResultStride;
  p.res_steer = h->p.res_steer + size_t(T - 1) * kNum, p.s_steer = T * kNum;
  p.in = tick_inputs_device(w->t), p.s_in = l.stride;
  p.path_in = h->p.path, p.obs = h->p.obs;
  p.key = w->keys_dev;
  p.est = w->vl_est + row * 2;
  launch_world_validate_prep(p, E, h->stream);
  HIPC(hipGetLastError());
  ValidateCarlaParams v = w->vv;
  v.K = E;
  v.count_rows = w->vl_rows + row, v.count = w->vl_count + row, v.count_lane = w->vl_lane + row;
  HIPC(hipMemsetAsync(v.cnt_oh, 0, w->val_nacc * 4, h->stream));
  HIPC(hipMemsetAsync(v.count_rows, 0, size_t(E) * 4, h->stream));
  if (!launch_validate_carla(v, size_t(w->val_lds), h->stream)) throw std::logic_error("world validation: LDS check");
  HIPC(hipGetLastError());
  ValidateRiskParams q = w->vq;
  q.K = E;
  q.count_pos = w->vl_pos + row * 3;
  q.var = w->vl_var + row * 3, q.cvar = w->vl_cvar + row * 3;
  q.mean = w->vl_mean + row * 3, q.vmax = w->vl_max + row * 3;
  q.mmd = w->val_S ? w->vl_mmd + row * 3 * w->val_S : nullptr;
  launch_vrisk_stats(q, h->stream);
  HIPC(hipGetLastError());
  launch_vrisk_mmd(q, h->stream);
  HIPC(hipGetLastError());
}

// frees the validation stage's buffers (the last allocations of the context)
void drop_validation(mpcmmd_world* w) {
  if (!w->val_on) return;
  for (size_t i = w->val_first; i < w->bufs.size(); ++i) (void)hipFree(w->bufs[i]);
  w->bufs.resize(w->val_first);
  w->val_on = false;
}

// frees the routed vehicles' buffers
void drop_vehicles(mpcmmd_world* w) {
  for (void* d : w->veh_bufs) (void)hipFree(d);
  w->veh_bufs.clear();
  w->rv = WorldRoutedParams{};
  w->veh_s0 = w->veh_log_s = nullptr;
  w->veh_v0 = w->veh_log = nullptr;
  w->veh_on = false, w->veh_E = 0;
}

template <class T>
T* veh_alloc(mpcmmd_world* w, size_t count, const void* src = nullptr) {
  void* d = nullptr;
  HIPC(hipMalloc(&d, (count ? count : 4) * sizeof(T)));
  w->veh_bufs.push_back(d);
  if (src && count) HIPC(hipMemcpy(d, src, count * sizeof(T), hipMemcpyHostToDevice));
  return static_cast<T*>(d);
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
  drop_vehicles(w);
  for (void* d : w->bufs) (void)hipFree(d);
  delete w;
}

int mpcmmd_world_reset(mpcmmd_world* w, int32_t n_episodes, const double* pos, const float* ego,
                       const float* vehicles, const float* mean, const float* cov, const float* u,
                       const int32_t* keys) {
  if (!w || !pos || !ego || !mean || !cov || !keys || (w->w.total > 0 && !vehicles && !w->veh_on))
    return fail(MPCMMD_E_INVALID, "null argument");
  if (n_episodes < 1 || n_episodes > w->Emax)
    return fail(MPCMMD_E_INVALID, "world: n_episodes must be 1..max_configs of the handle");
  if (w->veh_on && n_episodes != w->veh_E)
    return fail(MPCMMD_E_INVALID, "world: n_episodes is not the one mpcmmd_world_route_vehicles staged");
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
    if (w->veh_on && V) {  // the rows come from the reset-mode step
      HIPC(hipMemcpy(w->rv.s, w->veh_s0, E * V * 8, hipMemcpyDeviceToDevice));
      HIPC(hipMemcpy(w->rv.v, w->veh_v0, E * V * 4, hipMemcpyDeviceToDevice));
    } else if (V) {
      HIPC(hipMemcpy(w->q.veh, vehicles, E * V * 5 * 4, hipMemcpyHostToDevice));
    }
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
          if (w->val_on) enqueue_validation(w, k);
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

int mpcmmd_world_route_vehicles(mpcmmd_world* w, int32_t n_episodes, const double* veh_s, const float* veh_v,
                                const float* veh_param, const float* scalars) {
  if (!w) return fail(MPCMMD_E_INVALID, "null argument");
  const bool off = !veh_s && !veh_v && !veh_param;
  mpcmmd_world_routed rt{};
  if (!off) {
    if (!veh_s || !veh_v || !veh_param || !scalars) return fail(MPCMMD_E_INVALID, "null argument");
    if (n_episodes < 1 || n_episodes > w->Emax)
      return fail(MPCMMD_E_INVALID, "world: n_episodes must be 1..max_configs of the handle");
    rt.veh_s = const_cast<double*>(veh_s), rt.veh_v = const_cast<float*>(veh_v), rt.veh_param = veh_param;
    rt.acc_max = scalars[0], rt.brake = scalars[1], rt.gap0 = scalars[2], rt.headway = scalars[3];
    rt.length = scalars[4], rt.lane_tol = scalars[5], rt.gap_min = scalars[6], rt.acc_min = scalars[7];
    mpcmmd_world_model mm{};
    mm.total_obs = w->w.total;
    if (int rc = check_world_routed(&mm, &rt)) return rc;
  }
  const int rc = guarded([&] {
    check_device(w->h);
    HIPC(hipStreamSynchronize(w->h->stream));  // nothing in flight reads the buffers about to go
    drop_vehicles(w);
    w->reset_done = false;  // the policy changes with the episodes: the next run needs a reset
    if (off) return MPCMMD_OK;
    const size_t E = size_t(n_episodes), V = size_t(w->w.total), rows = size_t(w->Tmax) * size_t(w->Emax);
    w->rv.p = veh_scalars(rt);
    w->veh_s0 = veh_alloc<double>(w, E * V, veh_s), w->veh_v0 = veh_alloc<float>(w, E * V, veh_v);
    w->rv.param = veh_alloc<float>(w, E * V * 2, veh_param);
    w->rv.s = veh_alloc<double>(w, E * V), w->rv.v = veh_alloc<float>(w, E * V);
    w->veh_log_s = veh_alloc<double>(w, rows * V), w->veh_log = veh_alloc<float>(w, rows * V * 2);
    HIPC(hipDeviceSynchronize());
    w->veh_E = n_episodes;
    w->veh_on = true;
    return MPCMMD_OK;
  });
  if (rc != MPCMMD_OK) {  // a failed allocation leaves no half-made policy
    drop_vehicles(w);
    (void)hipGetLastError();
  }
  return rc;
}

int mpcmmd_world_vehicle_log(mpcmmd_world* w, int32_t ticks, double* veh_s, float* veh_va) {
  if (!w || !veh_s || !veh_va) return fail(MPCMMD_E_INVALID, "null argument");
  if (ticks < 0 || ticks > w->Tmax) return fail(MPCMMD_E_INVALID, "world: tick range");
  if (!w->veh_on) return fail(MPCMMD_E_STATE, "mpcmmd_world_vehicle_log without routed vehicles");
  return guarded([&] {
    check_device(w->h);
    HIPC(hipStreamSynchronize(w->h->stream));
    const size_t E = size_t(w->E), Em = size_t(w->Emax), V = size_t(w->w.total);
    if (ticks == 0 || E == 0 || V == 0) return MPCMMD_OK;
    // rows of Emax -> [ticks][n_episodes]: one strided copy per array
    HIPC(hipMemcpy2D(veh_s, E * V * 8, w->veh_log_s, Em * V * 8, E * V * 8, size_t(ticks), hipMemcpyDeviceToHost));
    HIPC(hipMemcpy2D(veh_va, E * V * 8, w->veh_log, Em * V * 8, E * V * 8, size_t(ticks), hipMemcpyDeviceToHost));
    return MPCMMD_OK;
  });
}

int mpcmmd_world_validate(mpcmmd_world* w, const mpcmmd_world_validation* cfg) {
  if (!w) return fail(MPCMMD_E_INVALID, "null argument");
  mpcmmd_handle* h = w->h;
  const int O = h->O, H = h->H, P = tick_num_path(w->t);
  ValidateRiskParams q{};
  if (cfg) {
    const int R = cfg->num_rollouts, S = cfg->num_sigma;
    if (R < 1 || R > (1 << 20) || int64_t(R) * H >= (int64_t(1) << 31))
      return fail(MPCMMD_E_INVALID, "world validation: num_rollouts out of 1..2^20 (and R H < 2^31)");
    if (!(cfg->alpha >= 0.0f && cfg->alpha <= 1.0f))
      return fail(MPCMMD_E_INVALID, "world validation: alpha out of [0, 1]");
    if (S < 0 || S > kRiskMaxSigma) return fail(MPCMMD_E_INVALID, "world validation: num_sigma out of [0, 8]");
    for (int i = 0; i < S; ++i)
      if (!(std::isfinite(cfg->sigma[i]) && cfg->sigma[i] > 0.0f))
        return fail(MPCMMD_E_INVALID, "world validation: every sigma must be finite and > 0");
    if (!validate_carla_shape_ok(O, H, P))
      return fail(MPCMMD_E_INVALID, "world validation: the validator takes num_obs <= 32 and num_prime >= 2");
    q.R = R, q.S = S;
    if (mpcmmd_quantile_position(R, cfg->alpha, &q.lo, &q.hi, &q.w_lo, &q.w_hi) != MPCMMD_OK)
      return fail(MPCMMD_E_INVALID, "world validation: quantile position");
  }
  const int rc = guarded([&] {
    check_device(h);
    HIPC(hipStreamSynchronize(h->stream));  // nothing in flight reads the buffers about to go
    drop_validation(w);
    w->reset_done = false;  // the stage changes with the episodes: the next run needs a reset
    if (!cfg) return MPCMMD_OK;
    int lds_max = 0;
    HIPC(hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, h->device));
    const size_t need = validate_carla_lds(O, H, P, true);
    if (need > size_t(lds_max))
      return fail(MPCMMD_E_UNSUPPORTED, "world validation: the shape's workgroup needs " + std::to_string(need) +
                                            " B of LDS, the device has " + std::to_string(lds_max));
    w->val_first = w->bufs.size();
    w->val_on = true;  // from here on drop_validation frees what exists
    const size_t Em = size_t(w->Emax), Tm = size_t(w->Tmax), R = size_t(q.R), S = size_t(q.S);
    const size_t n3 = 3 * Em, tiles = (R + kRiskTile - 1) / kRiskTile;
    w->val_S = q.S, w->val_lds = lds_max;
    const ProblemConsts& pc = h->pc;
    const mpcmmd_config& c = h->cfg;
    ValidateCarlaParams& v = w->vv;
    v = ValidateCarlaParams{};
    v.O = O, v.H = H, v.R = q.R, v.P = P, v.noise = c.noise, v.seed = c.seed;  // as carla_plan_params (validate_api.hip)
    v.sigma_acc = v.sigma_steer = c.noise_level;
    v.K_steer = float(pc.K_steer * double(c.noise_level));
    v.acc_const = c.acc_const_noise, v.steer_const = c.steer_const_noise;
    v.y_lb = float(pc.y_lb), v.y_ub = float(pc.y_ub), v.wheel_base = float(pc.wheel_base);
    v.obs_a2 = float(pc.a_obs * pc.a_obs), v.obs_b2 = float(pc.b_obs * pc.b_obs);
    v.init_mu_x = float(pc.init_mu_x), v.init_mu_y = float(pc.init_mu_y);
    v.init_sigma_x = float(pc.init_sigma_x), v.init_sigma_y = float(pc.init_sigma_y);
    WorldValidateParams& p = w->vp;
    p = WorldValidateParams{};
    p.H = H, p.O = O, p.P = P;
    p.pd = world_alloc<double>(w, size_t(kNum) * kNvar, pc.Pd.data());
    v.acc = p.acc = world_alloc<float>(w, Em * H), v.steer = p.steer = world_alloc<float>(w, Em * H);
    v.st0 = p.st0 = world_alloc<float>(w, Em * 8), v.path = p.path = world_alloc<float>(w, Em * 6 * P);
    v.x_obs = p.x_obs = world_alloc<float>(w, Em * O * kNum), v.y_obs = p.y_obs = world_alloc<float>(w, Em * O * kNum);
    v.keys = p.keys = world_alloc<uint32_t>(w, Em);
    const size_t n_oh = Em * O * H;
    w->val_nacc = n_oh + Em * 2 * H;
    v.cnt_oh = world_alloc<int32_t>(w, w->val_nacc), v.cnt_lane = v.cnt_oh + n_oh;
    q.costs = v.costs = world_alloc<float>(w, n3 * R);  // every element is stored by its row's workgroup
    q.np = world_alloc<int32_t>(w, n3);
    if (S > 0) {
      std::vector<float> sg(Em * S);
      for (size_t i = 0; i < sg.size(); ++i) sg[i] = cfg->sigma[i % S];
      q.sigma = world_alloc<float>(w, sg.size(), sg.data());
      q.u = world_alloc<float>(w, n3 * R);
      q.part = world_alloc<double>(w, n3 * tiles * S);
    }
    w->vq = q;
    const size_t rows = Tm * Em;
    w->vl_count = world_alloc<int32_t>(w, rows), w->vl_lane = world_alloc<int32_t>(w, rows);
    w->vl_rows = world_alloc<int32_t>(w, rows), w->vl_pos = world_alloc<int32_t>(w, rows * 3);
    w->vl_var = world_alloc<float>(w, rows * 3), w->vl_cvar = world_alloc<float>(w, rows * 3);
    w->vl_mean = world_alloc<float>(w, rows * 3), w->vl_max = world_alloc<float>(w, rows * 3);
    w->vl_mmd = world_alloc<float>(w, rows * 3 * S), w->vl_est = world_alloc<float>(w, rows * 2);
    return MPCMMD_OK;
  });
  if (rc != MPCMMD_OK) {  // a failed allocation leaves no half-made stage
    drop_validation(w);
    (void)hipGetLastError();
  }
  return rc;
}

int mpcmmd_world_validation_log(mpcmmd_world* w, int32_t ticks, int32_t* counts, int32_t* count_pos, float* stats,
                                float* mmd, float* est) {
  if (!w || !counts || !count_pos || !stats || !est) return fail(MPCMMD_E_INVALID, "null argument");
  if (w->val_on && w->val_S > 0 && !mmd) return fail(MPCMMD_E_INVALID, "null argument");
  if (ticks < 0 || ticks > w->Tmax) return fail(MPCMMD_E_INVALID, "world: tick range");
  if (!w->val_on) return fail(MPCMMD_E_STATE, "mpcmmd_world_validation_log without a validation stage");
  return guarded([&] {
    check_device(w->h);
    HIPC(hipStreamSynchronize(w->h->stream));
    if (ticks == 0 || w->E == 0) return MPCMMD_OK;
    const size_t E = size_t(w->E), Em = size_t(w->Emax), n = size_t(ticks) * E, S = size_t(w->val_S);
    // rows of Emax -> [ticks][n_episodes]: one strided copy per array
    auto back = [&](void* dst, const void* src, size_t row_bytes) {
      HIPC(hipMemcpy2D(dst, E * row_bytes, src, Em * row_bytes, E * row_bytes, size_t(ticks), hipMemcpyDeviceToHost));
    };
    std::vector<int32_t> c3(n * 3);
    back(c3.data(), w->vl_count, 4), back(c3.data() + n, w->vl_lane, 4), back(c3.data() + 2 * n, w->vl_rows, 4);
    for (size_t i = 0; i < n; ++i)
      for (size_t k = 0; k < 3; ++k) counts[i * 3 + k] = c3[k * n + i];
    std::vector<float> s4(n * 12);
    back(s4.data(), w->vl_var, 12), back(s4.data() + n * 3, w->vl_cvar, 12);
    back(s4.data() + n * 6, w->vl_mean, 12), back(s4.data() + n * 9, w->vl_max, 12);
    for (size_t i = 0; i < n; ++i)
      for (size_t k = 0; k < 4; ++k) std::memcpy(stats + (i * 4 + k) * 3, &s4[(k * n + i) * 3], 12);
    back(count_pos, w->vl_pos, 12), back(est, w->vl_est, 8);
    if (S > 0) back(mmd, w->vl_mmd, 12 * S);
    return MPCMMD_OK;
  });
}

int mpcmmd_world_validation_inputs(mpcmmd_world* w, float* acc, float* steer, float* st0, float* path, float* x_obs,
                                   float* y_obs, uint32_t* keys) {
  if (!w) return fail(MPCMMD_E_INVALID, "null argument");
  if (!w->val_on) return fail(MPCMMD_E_STATE, "mpcmmd_world_validation_inputs without a validation stage");
  return guarded([&] {
    check_device(w->h);
    HIPC(hipStreamSynchronize(w->h->stream));
    const size_t E = size_t(w->E), H = size_t(w->vp.H), O = size_t(w->vp.O), P = size_t(w->vp.P);
    auto back = [&](void* dst, const void* src, size_t bytes) {
      if (dst && bytes) HIPC(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    };
    back(acc, w->vp.acc, E * H * 4), back(steer, w->vp.steer, E * H * 4), back(st0, w->vp.st0, E * 8 * 4);
    back(path, w->vp.path, E * 6 * P * 4);
    back(x_obs, w->vp.x_obs, E * O * kNum * 4), back(y_obs, w->vp.y_obs, E * O * kNum * 4);
    back(keys, w->vp.keys, E * 4);
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

extern "C" int mpcmmd_world_step_host_routed(const mpcmmd_world_model* m, int32_t tick, const mpcmmd_world_step_io* io,
                                             const mpcmmd_world_routed* rt) {
  if (int rc = check_world(m, io)) return rc;
  if (int rc = check_world_routed(m, rt)) return rc;
  world_step_host(*m, tick, *io, world_draw, rt);
  return MPCMMD_OK;
}

// one launch over the harness's arrays; rt: the routed instantiation
static int world_step_device(const mpcmmd_world_model* m, int32_t device, int32_t n_episodes, int32_t tick,
                             const mpcmmd_world_step_io* io, const mpcmmd_world_routed* rt) {
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
    q.tick = tick, q.reset = rt && tick < 0 ? 1 : 0;
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
    // a reset-mode launch writes no log row: what the caller's arrays hold goes up and comes back
    const bool keep = q.reset != 0;
    q.logd = static_cast<double*>(io_buf(io->log_d, E * MPCMMD_WORLD_LOG_D * 8, keep));
    q.logf = static_cast<float*>(io_buf(io->log_f, E * MPCMMD_WORLD_LOG_F * 4, keep));
    q.logi = static_cast<int32_t*>(io_buf(io->log_i, E * MPCMMD_WORLD_LOG_I * 4, keep));
    if (rt) {
      WorldRoutedParams r{};
      r.p = veh_scalars(*rt);
      r.s = static_cast<double*>(io_buf(rt->veh_s, E * V * 8, true));
      r.v = static_cast<float*>(io_buf(rt->veh_v, E * V * 4, true));
      r.param = static_cast<const float*>(sc.up(V ? rt->veh_param : nullptr, V ? E * V * 2 * 4 : 16));
      r.log = rt->veh_log ? static_cast<float*>(io_buf(rt->veh_log, E * V * 2 * 4, true)) : nullptr;
      launch_world_step_routed(q, r, n_episodes, nullptr);
    } else {
      launch_world_step(q, n_episodes, nullptr);
    }
    HIPC(hipGetLastError());
    HIPC(hipDeviceSynchronize());
    for (const Out& o : outs) HIPC(hipMemcpy(o.host, o.dev, o.bytes, hipMemcpyDeviceToHost));
    return MPCMMD_OK;
  });
}

extern "C" int mpcmmd_world_step_device(const mpcmmd_world_model* m, int32_t device, int32_t n_episodes, int32_t tick,
                                        const mpcmmd_world_step_io* io) {
  if (int rc = check_world(m, io)) return rc;
  return world_step_device(m, device, n_episodes, tick, io, nullptr);
}

extern "C" int mpcmmd_world_step_device_routed(const mpcmmd_world_model* m, int32_t device, int32_t n_episodes,
                                               int32_t tick, const mpcmmd_world_step_io* io,
                                               const mpcmmd_world_routed* rt) {
  if (int rc = check_world(m, io)) return rc;
  if (int rc = check_world_routed(m, rt)) return rc;
  return world_step_device(m, device, n_episodes, tick, io, rt);
}
