// libmpcmmd: the surrogate world on the device (include/mpcmmd.h).
// mpcmmd_world_step_device holds k_world_step against the host twin.  The world
// context (mpcmmd_world) is an episode context (episodes.hpp owns the buffers,
// the reset's prologue, the tick loop and the read-backs) whose tick is the
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
#include "episodes.hpp"
#include "rng.hpp"
#include "tick.hpp"
#include "world.hpp"
#include "world_draw.hpp"
#include "world_host.hpp"
#include "world_validate.hpp"

using namespace mpcmmd;

// hidden, as everything of episodes.hpp it embeds: no constructor or destructor becomes a dynamic symbol
struct __attribute__((visibility("hidden"))) mpcmmd_world {
  Episodes s;  // the episodes, the log and the two stages' common state (episodes.hpp)
  mpcmmd_tick* t = nullptr;
  WorldScalars w{};
  WorldStepParams q{};  // the model's arrays and the state, filled at create
  // the validation stage
  int val_lds = 0;            // the device's LDS per workgroup
  size_t val_nacc = 0;        // words of cnt_oh | cnt_lane
  ValidateCarlaParams vv{};   // the packed inputs, the accumulators and the costs
  WorldValidateParams vp{};   // the packed inputs once more, as k_world_validate_prep writes them
  // the routed vehicles
  WorldRoutedParams rv{};       // scalars, states [E][V], parameters
  double* veh_s0 = nullptr;     // [E][V] the staged start states
  float* veh_v0 = nullptr;
  double* veh_log_s = nullptr;  // [Tmax][Emax][V]
  float* veh_log = nullptr;     // [Tmax][Emax][V][2]
};

namespace {

// one k_world_step over the context's episodes: the plan from the handle's results of the last
// iteration, the next inputs into the tick context's image
void enqueue_step(mpcmmd_world* w, int tick, bool reset) {
  const Episodes& s = w->s;
  mpcmmd_handle* h = s.h;
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
  const size_t row = size_t(reset ? 0 : tick) * s.Emax;
  q.u = s.drawn ? nullptr : s.u + row * 4;
  q.key = s.keys_dev, q.seed = h->cfg.seed;
  q.logd = s.logd + row * 3, q.logf = s.logf + row * 13, q.logi = s.logi + row * 4;
  q.plan = s.plan + row * 34;
  q.chol = s.chol;
  if (s.veh_on) {
    WorldRoutedParams r = w->rv;
    r.log = w->veh_log + row * size_t(q.w.total) * 2, r.log_s = w->veh_log_s + row * size_t(q.w.total);
    launch_world_step_routed(q, r, s.E, h->stream);
  } else {
    launch_world_step(q, s.E, h->stream);
  }
  HIPC(hipGetLastError());
}

// the validation stage of tick `tick`, behind its CEM iterations and before its world step (the
// step overwrites the input image and st0): the packed inputs, the zeroed accumulators, then
// mpcmmd_validate_carla_risk's launches with K = E and the results pointed at the tick's log row
void enqueue_validation(mpcmmd_world* w, int tick) {
  const Episodes& s = w->s;
  mpcmmd_handle* h = s.h;
  const TickLayout l = tick_layout_of(w->t);
  const int T = h->T, E = s.E;
  const size_t row = size_t(tick) * s.Emax;
  WorldValidateParams p = w->vp;
  p.tick = tick;
  p.res = h->p.results + size_t(T - 1) * kResultStride, p.s_res = T * kResultStride;
  p.res_steer = h->p.res_steer + size_t(T - 1) * kNum, p.s_steer = T * kNum;
  p.in = tick_inputs_device(w->t), p.s_in = l.stride;
  p.path_in = h->p.path, p.obs = h->p.obs;
  p.key = s.keys_dev;
  p.est = s.vl.est + row * 2;
  launch_world_validate_prep(p, E, h->stream);
  HIPC(hipGetLastError());
  ValidateCarlaParams v = w->vv;
  v.K = E;
  v.count = s.vl.count[0] + row, v.count_lane = s.vl.count[1] + row, v.count_rows = s.vl.count[2] + row;
  HIPC(hipMemsetAsync(v.cnt_oh, 0, w->val_nacc * 4, h->stream));
  HIPC(hipMemsetAsync(v.count_rows, 0, size_t(E) * 4, h->stream));
  if (!launch_validate_carla(v, size_t(w->val_lds), h->stream)) throw std::logic_error("world validation: LDS check");
  HIPC(hipGetLastError());
  ValidateRiskParams q = s.vq;
  q.K = E;
  s.vl.point(q, row);
  launch_vrisk_stats(q, h->stream);
  HIPC(hipGetLastError());
  launch_vrisk_mmd(q, h->stream);
  HIPC(hipGetLastError());
}

// nothing of the context is in flight
void sync(mpcmmd_world* w) { HIPC(hipStreamSynchronize(w->s.h->stream)); }

void drop_validation(mpcmmd_world* w) {
  w->s.val.release();
  w->s.val_on = false;
}

void drop_vehicles(mpcmmd_world* w) {
  w->s.veh.release();
  w->rv = WorldRoutedParams{};
  w->veh_s0 = w->veh_log_s = nullptr;
  w->veh_v0 = w->veh_log = nullptr;
  w->s.veh_on = false, w->s.veh_E = 0;
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
  Episodes& s = w->s;
  w->t = t, s.h = h;
  s.Tmax = max_ticks, s.Emax = h->Gmax;
  int rc = guarded([&] {
    check_device(h);
    mpcmmd_world_model mm = *m;
    mm.num_batch = h->B;  // the handle's population and its own pop0 normals
    w->w = world_scalars(mm);
    const size_t n = size_t(m->num_route), E = size_t(s.Emax), V = size_t(m->total_obs);
    if (h->pop0_normals.empty())
      h->pop0_normals = host_normals(kFixedKey0, h->cfg.seed, kStreamPop0, 0, size_t(h->B) * 8);
    WorldStepParams& q = w->q;
    Arena& a = s.base;
    q.w = w->w;
    q.route_x = a.alloc<double>(n, m->route_x), q.route_y = a.alloc<double>(n, m->route_y);
    q.arc = a.alloc<double>(n, m->route_arc);
    q.sx = a.alloc<double>(4 * (n - 1), m->spline_x), q.sy = a.alloc<double>(4 * (n - 1), m->spline_y);
    q.pdot4 = a.alloc<double>(44, m->pdot4);
    q.pop0 = a.alloc<float>(h->pop0_normals.size(), h->pop0_normals.data());
    s.chol = a.alloc<double>(64);
    q.pos = s.pos = a.alloc<double>(E * 2), q.ego = a.alloc<float>(E * 3);
    q.veh = a.alloc<float>(E * V * 5), q.done = s.done = a.alloc<int32_t>(E);
    s.alloc_rows(4, MPCMMD_WORLD_LOG_D, MPCMMD_WORLD_LOG_F, MPCMMD_WORLD_LOG_I, 34);
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
  (void)hipSetDevice(w->s.h->device);
  if (w->s.h->stream) (void)hipStreamSynchronize(w->s.h->stream);  // the steps in flight
  delete w;  // the three arenas free their buffers
}

int mpcmmd_world_reset(mpcmmd_world* w, int32_t n_episodes, const double* pos, const float* ego,
                       const float* vehicles, const float* mean, const float* cov, const float* u,
                       const int32_t* keys) {
  if (!w || !pos || !ego || !mean || !cov || !keys || (w->w.total > 0 && !vehicles && !w->s.veh_on))
    return fail(MPCMMD_E_INVALID, "null argument");
  if (n_episodes < 1 || n_episodes > w->s.Emax)
    return fail(MPCMMD_E_INVALID, "world: n_episodes must be 1..max_configs of the handle");
  if (w->s.veh_on && n_episodes != w->s.veh_E)
    return fail(MPCMMD_E_INVALID, "world: n_episodes is not the one mpcmmd_world_route_vehicles staged");
  auto upload = [&](size_t E) {
    const size_t V = size_t(w->w.total);
    HIPC(hipMemcpy(w->q.ego, ego, E * 3 * 4, hipMemcpyHostToDevice));
    if (w->s.veh_on && V) {  // the rows come from the reset-mode step
      HIPC(hipMemcpy(w->rv.s, w->veh_s0, E * V * 8, hipMemcpyDeviceToDevice));
      HIPC(hipMemcpy(w->rv.v, w->veh_v0, E * V * 4, hipMemcpyDeviceToDevice));
    } else if (V) {
      HIPC(hipMemcpy(w->q.veh, vehicles, E * V * 5 * 4, hipMemcpyHostToDevice));
    }
  };
  // the step: tick 0's inputs, st0 and population from the start states
  return reset_common(w->s, n_episodes, pos, mean, cov, u, keys, [&] { sync(w); }, upload,
                      [&] { enqueue_step(w, -1, true); });
}

int mpcmmd_world_run(mpcmmd_world* w, int32_t cost_kind, int32_t tick_begin, int32_t count, const float* cov,
                     const float* v_des, float threshold) {
  if (!w || !cov || !v_des) return fail(MPCMMD_E_INVALID, "null argument");
  if (!w->s.reset_done) return fail(MPCMMD_E_STATE, "mpcmmd_world_run before mpcmmd_world_reset");
  if (tick_begin < 0 || count < 0 || tick_begin + count > w->s.Tmax) return fail(MPCMMD_E_INVALID, "world: tick range");
  return run_ticks(
      w->s, tick_begin, count, cov,
      [&](const int32_t* idx, const float* covs) {
        return tick_begin_chained(w->t, w->s.E, cost_kind, idx, covs, v_des, threshold);
      },
      [&](int k) {
        if (w->s.val_on) enqueue_validation(w, k);
        enqueue_step(w, k, false);
      });
}

int mpcmmd_world_log(mpcmmd_world* w, int32_t ticks, double* log_d, float* log_f, int32_t* log_i, float* plan,
                     int32_t* done_tick) {
  if (!w || !log_d || !log_f || !log_i || !plan || !done_tick) return fail(MPCMMD_E_INVALID, "null argument");
  if (ticks < 0 || ticks > w->s.Tmax) return fail(MPCMMD_E_INVALID, "world: tick range");
  return guarded([&] {
    check_device(w->s.h);
    sync(w);
    if (ticks > 0) log_rows_back(w->s, ticks, log_d, log_f, log_i, plan);
    HIPC(hipMemcpy(done_tick, w->s.done, size_t(w->s.E) * 4, hipMemcpyDeviceToHost));
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
    if (n_episodes < 1 || n_episodes > w->s.Emax)
      return fail(MPCMMD_E_INVALID, "world: n_episodes must be 1..max_configs of the handle");
    rt.veh_s = const_cast<double*>(veh_s), rt.veh_v = const_cast<float*>(veh_v), rt.veh_param = veh_param;
    rt.acc_max = scalars[0], rt.brake = scalars[1], rt.gap0 = scalars[2], rt.headway = scalars[3];
    rt.length = scalars[4], rt.lane_tol = scalars[5], rt.gap_min = scalars[6], rt.acc_min = scalars[7];
    mpcmmd_world_model mm{};
    mm.total_obs = w->w.total;
    if (int rc = check_world_routed(&mm, &rt)) return rc;
  }
  return remake_stage(w->s, !off, [&] { sync(w); }, [&] { drop_vehicles(w); }, [&] {
    Episodes& s = w->s;
    const size_t E = size_t(n_episodes), V = size_t(w->w.total), rows = size_t(s.Tmax) * size_t(s.Emax);
    w->rv.p = veh_scalars(rt);
    w->veh_s0 = s.veh.alloc<double>(E * V, veh_s), w->veh_v0 = s.veh.alloc<float>(E * V, veh_v);
    w->rv.param = s.veh.alloc<float>(E * V * 2, veh_param);
    w->rv.s = s.veh.alloc<double>(E * V), w->rv.v = s.veh.alloc<float>(E * V);
    w->veh_log_s = s.veh.alloc<double>(rows * V), w->veh_log = s.veh.alloc<float>(rows * V * 2);
    HIPC(hipDeviceSynchronize());
    s.veh_E = n_episodes;
    s.veh_on = true;
    return MPCMMD_OK;
  });
}

int mpcmmd_world_vehicle_log(mpcmmd_world* w, int32_t ticks, double* veh_s, float* veh_va) {
  if (!w || !veh_s || !veh_va) return fail(MPCMMD_E_INVALID, "null argument");
  if (ticks < 0 || ticks > w->s.Tmax) return fail(MPCMMD_E_INVALID, "world: tick range");
  if (!w->s.veh_on) return fail(MPCMMD_E_STATE, "mpcmmd_world_vehicle_log without routed vehicles");
  return guarded([&] {
    check_device(w->s.h);
    sync(w);
    const size_t E = size_t(w->s.E), Em = size_t(w->s.Emax), V = size_t(w->w.total);
    if (ticks == 0 || E == 0 || V == 0) return MPCMMD_OK;
    rows_back(veh_s, w->veh_log_s, V * 8, ticks, E, Em), rows_back(veh_va, w->veh_log, V * 8, ticks, E, Em);
    return MPCMMD_OK;
  });
}

int mpcmmd_world_validate(mpcmmd_world* w, const mpcmmd_world_validation* cfg) {
  if (!w) return fail(MPCMMD_E_INVALID, "null argument");
  Episodes& s = w->s;
  mpcmmd_handle* h = s.h;
  const int O = h->O, H = h->H, P = tick_num_path(w->t);
  ValidateRiskParams q{};
  if (cfg) {
    // num_rollouts with the world's R H clause, in the world's words: the shared check's own
    // num_rollouts clause cannot fire behind this one
    const int R = cfg->num_rollouts;
    if (R < 1 || R > (1 << 20) || int64_t(R) * H >= (int64_t(1) << 31))
      return fail(MPCMMD_E_INVALID, "world validation: num_rollouts out of 1..2^20 (and R H < 2^31)");
    q.R = R, q.S = cfg->num_sigma;
    if (int rc = check_risk_config("world", R, cfg->alpha, q.S, cfg->sigma, &q.lo, &q.hi, &q.w_lo, &q.w_hi)) return rc;
    if (!validate_carla_shape_ok(O, H, P))
      return fail(MPCMMD_E_INVALID, "world validation: the validator takes num_obs <= 32 and num_prime >= 2");
  }
  return remake_stage(s, cfg != nullptr, [&] { sync(w); }, [&] { drop_validation(w); }, [&] {
    int lds_max = 0;
    HIPC(hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, h->device));
    const size_t need = validate_carla_lds(O, H, P, true);
    if (need > size_t(lds_max))
      return fail(MPCMMD_E_UNSUPPORTED, "world validation: the shape's workgroup needs " + std::to_string(need) +
                                            " B of LDS, the device has " + std::to_string(lds_max));
    s.val_on = true;
    Arena& a = s.val;
    const size_t Em = size_t(s.Emax);
    w->val_lds = lds_max;
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
    p.pd = a.alloc<double>(size_t(kNum) * kNvar, pc.Pd.data());
    v.acc = p.acc = a.alloc<float>(Em * H), v.steer = p.steer = a.alloc<float>(Em * H);
    v.st0 = p.st0 = a.alloc<float>(Em * 8), v.path = p.path = a.alloc<float>(Em * 6 * P);
    v.x_obs = p.x_obs = a.alloc<float>(Em * O * kNum), v.y_obs = p.y_obs = a.alloc<float>(Em * O * kNum);
    v.keys = p.keys = a.alloc<uint32_t>(Em);
    const size_t n_oh = Em * O * H;
    w->val_nacc = n_oh + Em * 2 * H;
    v.cnt_oh = a.alloc<int32_t>(w->val_nacc), v.cnt_lane = v.cnt_oh + n_oh;
    alloc_risk_scratch(a, q, Em, cfg->sigma);
    v.costs = q.costs;  // every element is stored by its row's workgroup
    s.vq = q;
    s.vl.alloc(a, size_t(s.Tmax) * Em, size_t(q.S), 3);
    return MPCMMD_OK;
  });
}

int mpcmmd_world_validation_log(mpcmmd_world* w, int32_t ticks, int32_t* counts, int32_t* count_pos, float* stats,
                                float* mmd, float* est) {
  if (!w) return fail(MPCMMD_E_INVALID, "null argument");
  return validation_log_back(w->s, "world", "mpcmmd_world_validation_log", ticks, counts, count_pos, stats, mmd, est,
                             [&] { sync(w); });
}

int mpcmmd_world_validation_inputs(mpcmmd_world* w, float* acc, float* steer, float* st0, float* path, float* x_obs,
                                   float* y_obs, uint32_t* keys) {
  if (!w) return fail(MPCMMD_E_INVALID, "null argument");
  if (!w->s.val_on) return fail(MPCMMD_E_STATE, "mpcmmd_world_validation_inputs without a validation stage");
  return guarded([&] {
    check_device(w->s.h);
    sync(w);
    const size_t E = size_t(w->s.E), H = size_t(w->vp.H), O = size_t(w->vp.O), P = size_t(w->vp.P);
    back_if(acc, w->vp.acc, E * H * 4), back_if(steer, w->vp.steer, E * H * 4), back_if(st0, w->vp.st0, E * 8 * 4);
    back_if(path, w->vp.path, E * 6 * P * 4);
    back_if(x_obs, w->vp.x_obs, E * O * kNum * 4), back_if(y_obs, w->vp.y_obs, E * O * kNum * 4);
    back_if(keys, w->vp.keys, E * 4);
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
  return guarded([&] {
    StepHarness hs;
    if (int rc = hs.open("world", device, n_episodes)) return rc;
    const size_t E = size_t(n_episodes), n = size_t(m->num_route), P = size_t(m->num_path), O = size_t(m->num_obs);
    const size_t B = size_t(m->num_batch), V = size_t(m->total_obs);
    WorldStepParams q{};
    q.w = world_scalars(*m);
    q.tick = tick, q.reset = rt && tick < 0 ? 1 : 0;
    q.s_plan = 11, q.s_steer = 4, q.s_init = 6, q.s_wp = int(P), q.s_obs = int(O) * 5;
    q.route_x = hs.in(m->route_x, n), q.route_y = hs.in(m->route_y, n), q.arc = hs.in(m->route_arc, n);
    q.sx = hs.in(m->spline_x, 4 * (n - 1)), q.sy = hs.in(m->spline_y, 4 * (n - 1));
    q.pdot4 = hs.in(m->pdot4, 44), q.chol = hs.in(m->chol, 64), q.pop0 = hs.in(m->pop0, B * 8);
    q.cx = hs.in(io->cx, E * 11), q.cy = hs.in(io->cy, E * 11), q.steer = hs.in(io->steer, E * 4);
    q.u = io->u ? hs.in(io->u, E * 4) : nullptr;
    q.key = io->key ? hs.in(io->key, E) : nullptr;
    q.seed = m->seed;
    q.mean = hs.in(io->mean, E * 8);
    // state: in and out; a world without vehicles still gets a pointer
    q.pos = hs.io(io->pos, E * 2, true), q.ego = hs.io(io->ego, E * 3, true);
    q.veh = hs.io(io->vehicles, E * V * 5, true), q.done = hs.io(io->done_tick, E, true);
    q.init = hs.io(io->init_state, E * 6, false);
    q.xw = hs.io(io->x_wp, E * P, false), q.yw = hs.io(io->y_wp, E * P, false);
    q.obs = hs.io(io->obstacles, E * O * 5, false), q.pop = hs.io(io->pop, E * B * 8, false);
    // a reset-mode launch writes no log row: what the caller's arrays hold goes up and comes back
    const bool keep = q.reset != 0;
    q.logd = hs.io(io->log_d, E * MPCMMD_WORLD_LOG_D, keep), q.logf = hs.io(io->log_f, E * MPCMMD_WORLD_LOG_F, keep);
    q.logi = hs.io(io->log_i, E * MPCMMD_WORLD_LOG_I, keep);
    if (rt) {
      WorldRoutedParams r{};
      r.p = veh_scalars(*rt);
      r.s = hs.io(rt->veh_s, E * V, true), r.v = hs.io(rt->veh_v, E * V, true);
      r.param = V ? hs.in(rt->veh_param, E * V * 2) : hs.in<float>(nullptr, 4);
      r.log = rt->veh_log ? hs.io(rt->veh_log, E * V * 2, true) : nullptr;
      launch_world_step_routed(q, r, n_episodes, nullptr);
    } else {
      launch_world_step(q, n_episodes, nullptr);
    }
    hs.finish();
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
