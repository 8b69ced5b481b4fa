// libmpcmmd: the stand-alone Monte-Carlo validation entry points
// (mpcmmd_validate, mpcmmd_validate_carla, mpcmmd_validate_risk,
// mpcmmd_validate_carla_risk).  They use no
// handle: every call allocates, uploads, launches its kernels and reads the
// results back.
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "api_common.hpp"
#include "kernels.hpp"
#include "solve_host.hpp"

using namespace mpcmmd;

namespace {

// the device visible and selected, or a throw
void select_device(int device) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) throw HipError("no HIP device visible");
  if (device < 0 || device >= ndev) throw std::invalid_argument("device out of range");
  HIPC(hipSetDevice(device));
}

// the noise kind and the variant family of a validation call (carla: a CARLA
// town; else static / dynamic): MPCMMD_OK, or the entry point's own code and
// message for a variant of the other family
int check_noise_variant(int noise, int variant, bool carla, int code, const char* msg) {
  if (noise != MPCMMD_NOISE_GAUSSIAN && noise != MPCMMD_NOISE_BETA) return fail(MPCMMD_E_INVALID, "noise");
  const bool ok = carla ? variant == MPCMMD_VARIANT_CARLA_TOWN05 || variant == MPCMMD_VARIANT_CARLA_TOWN10HD
                        : variant == MPCMMD_VARIANT_STATIC || variant == MPCMMD_VARIANT_DYNAMIC;
  return ok ? MPCMMD_OK : fail(code, msg);
}

// the plan inputs of mpcmmd_validate / mpcmmd_validate_risk on the device
// (count and count_lane stay null)
template <class Args>
void plan_params(const Args& a, Scratch& dev, ValidateParams& v) {
  const int K = a.num_cfg, O = a.num_obs, H = a.num_prime, R = a.num_rollouts;
  const ProblemConsts pc = build_constants(H, a.variant);
  const std::vector<float> basis = pack_basis(pc);  // P, Pdot, Pddot
  v.K = K, v.O = O, v.H = H, v.R = R, v.noise = a.noise;
  v.noise_level = a.noise_level, v.acc_const = a.acc_const_noise, v.steer_const = a.steer_const_noise;
  v.K_steer = pc.K_steer, v.y_lb = pc.y_lb, v.y_ub = pc.y_ub, v.seed = a.seed;
  v.Pdot = (const float*)dev.up(basis.data() + kNum * kNvar, kNum * kNvar * 4);
  v.Pddot = (const float*)dev.up(basis.data() + 2 * kNum * kNvar, kNum * kNvar * 4);
  v.cx = (const double*)dev.up(a.cx, size_t(K) * 11 * 8);
  v.cy = (const double*)dev.up(a.cy, size_t(K) * 11 * 8);
  v.init_state = (const double*)dev.up(a.init_state, size_t(K) * 6 * 8);
  v.x_obs = (const float*)dev.up(a.x_obs, size_t(K) * O * 100 * 4);
  v.y_obs = (const float*)dev.up(a.y_obs, size_t(K) * O * 100 * 4);
  v.draws = a.draws ? (const double*)dev.up(a.draws, size_t(K) * 3 * R * H * 8) : nullptr;
  v.keys = (const uint32_t*)dev.up(a.keys, size_t(K) * 4);
}

// the plan inputs and the integer counters of mpcmmd_validate_carla /
// mpcmmd_validate_carla_risk on the device (costs stays null); the counters
// are one allocation of n_all words from v.cnt_oh: count_oh | lane |
// count_rows | count | count_lane
template <class Args>
size_t carla_plan_params(const Args& a, Scratch& dev, ValidateCarlaParams& v) {
  const int K = a.num_cfg, O = a.num_obs, H = a.num_prime, R = a.num_rollouts, P = a.num_path;
  const ProblemConsts pc = build_constants(H, a.variant);
  // the plan's controls and the tick's initial state as carla_rows forms it
  std::vector<float> acc, steer, st0(size_t(K) * 8, 0.0f);
  plan_controls(a.v, a.steer, K, H, acc, steer);
  for (int k = 0; k < K; ++k) {
    const float* is = a.init_state + size_t(k) * 6;
    float* o = st0.data() + size_t(k) * 8;
    o[0] = is[0], o[1] = is[1];
    carla_velocity_heading(is[2], is[4], &o[2], &o[3], &o[4]);
  }
  v.K = K, v.O = O, v.H = H, v.R = R, v.P = P, v.noise = a.noise, v.seed = a.seed;
  v.sigma_acc = v.sigma_steer = a.noise_level;
  v.K_steer = float(pc.K_steer * double(a.noise_level));
  v.acc_const = a.acc_const_noise, v.steer_const = a.steer_const_noise;
  v.y_lb = float(pc.y_lb), v.y_ub = float(pc.y_ub), v.wheel_base = float(pc.wheel_base);
  v.obs_a2 = float(pc.a_obs * pc.a_obs), v.obs_b2 = float(pc.b_obs * pc.b_obs);
  v.init_mu_x = float(pc.init_mu_x), v.init_mu_y = float(pc.init_mu_y);
  v.init_sigma_x = float(pc.init_sigma_x), v.init_sigma_y = float(pc.init_sigma_y);
  v.st0 = (const float*)dev.up(st0.data(), st0.size() * 4);
  v.acc = (const float*)dev.up(acc.data(), acc.size() * 4);
  v.steer = (const float*)dev.up(steer.data(), steer.size() * 4);
  v.x_obs = (const float*)dev.up(a.x_obs, size_t(K) * O * kNum * 4);
  v.y_obs = (const float*)dev.up(a.y_obs, size_t(K) * O * kNum * 4);
  v.path = (const float*)dev.up(a.path, size_t(K) * 6 * P * 4);
  v.draws = a.draws ? (const float*)dev.up(a.draws, size_t(K) * 3 * R * H * 4) : nullptr;
  v.init_eps = a.init_eps ? (const float*)dev.up(a.init_eps, size_t(K) * R * 4 * 4) : nullptr;
  v.keys = (const uint32_t*)dev.up(a.keys, size_t(K) * 4);
  const size_t n_oh = size_t(K) * O * H, n_lane = size_t(K) * 2 * H, n_all = n_oh + n_lane + size_t(3) * K;
  int32_t* ctr = (int32_t*)dev.up(nullptr, n_all * 4);
  v.cnt_oh = ctr, v.cnt_lane = ctr + n_oh, v.count_rows = v.cnt_lane + n_lane;
  v.count = v.count_rows + K, v.count_lane = v.count + K;
  return n_all;
}

// the shape limits shared by the two CARLA validation entry points
bool carla_shape_ok(int K, int O, int H, int R, int P) {
  return K >= 0 && K <= 65535 && R >= 1 && validate_carla_shape_ok(O, H, P) &&
         int64_t(R) * H < (int64_t(1) << 31);
}

// the device's LDS per workgroup against the shape's need: MPCMMD_OK, or MPCMMD_E_UNSUPPORTED
int carla_lds_check(const char* who, int device, int O, int H, int P, bool costs, int* lds_max) {
  HIPC(hipDeviceGetAttribute(lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, device));
  const size_t need = validate_carla_lds(O, H, P, costs);
  if (need > size_t(*lds_max))
    return fail(MPCMMD_E_UNSUPPORTED, std::string(who) + ": the shape's workgroup needs " + std::to_string(need) +
                                          " B of LDS, the device has " + std::to_string(*lds_max));
  return MPCMMD_OK;
}

}  // namespace

extern "C" {

int mpcmmd_validate(const mpcmmd_validate_args* a) {
  if (!a) return fail(MPCMMD_E_INVALID, "null argument");
  const int K = a->num_cfg, O = a->num_obs, H = a->num_prime, R = a->num_rollouts;
  if (K < 0 || R < 1 || !validate_shape_ok(O, H)) return fail(MPCMMD_E_INVALID, "validate: shape out of range");
  if (int rc = check_noise_variant(a->noise, a->variant, false, MPCMMD_E_UNSUPPORTED,
                                   "validate: static / dynamic variants (S/validation.py, D/validation.py); CARLA "
                                   "plans: mpcmmd_validate_carla"))
    return rc;
  if (K == 0) return MPCMMD_OK;
  if (!a->cx || !a->cy || !a->init_state || !a->x_obs || !a->y_obs || !a->keys || !a->count || !a->count_lane)
    return fail(MPCMMD_E_INVALID, "null argument");
  return guarded([&] {
    select_device(a->device);
    Scratch dev;
    ValidateParams v{};
    plan_params(*a, dev, v);
    v.count = (int32_t*)dev.up(nullptr, size_t(K) * 4);
    v.count_lane = (int32_t*)dev.up(nullptr, size_t(K) * 4);
    launch_validate(v, nullptr);
    HIPC(hipGetLastError());
    HIPC(hipDeviceSynchronize());
    HIPC(hipMemcpy(a->count, v.count, size_t(K) * 4, hipMemcpyDeviceToHost));
    HIPC(hipMemcpy(a->count_lane, v.count_lane, size_t(K) * 4, hipMemcpyDeviceToHost));
    return MPCMMD_OK;
  });
}

int mpcmmd_validate_carla(const mpcmmd_validate_carla_args* a) {
  if (!a) return fail(MPCMMD_E_INVALID, "null argument");
  const int K = a->num_cfg, O = a->num_obs, H = a->num_prime, R = a->num_rollouts, P = a->num_path;
  if (!carla_shape_ok(K, O, H, R, P)) return fail(MPCMMD_E_INVALID, "validate_carla: shape out of range");
  if (int rc = check_noise_variant(a->noise, a->variant, true, MPCMMD_E_INVALID,
                                   "validate_carla: a CARLA variant (static / dynamic optima: mpcmmd_validate)"))
    return rc;
  if (K == 0) return MPCMMD_OK;
  if (!a->init_state || !a->v || !a->steer || !a->x_obs || !a->y_obs || !a->path || !a->keys || !a->count ||
      !a->count_lane || !a->count_rows)
    return fail(MPCMMD_E_INVALID, "null argument");
  return guarded([&] {
    select_device(a->device);
    int lds_max = 0;
    if (int rc = carla_lds_check("validate_carla", a->device, O, H, P, false, &lds_max)) return rc;
    struct Events {  // declared before the buffers: destroyed after they are freed
      hipEvent_t e0 = nullptr, e1 = nullptr;
      ~Events() {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
      }
    } ev;
    Scratch dev;
    ValidateCarlaParams v{};
    const size_t n_all = carla_plan_params(*a, dev, v), n_oh = size_t(K) * O * H;
    if (a->elapsed_ms) {
      HIPC(hipEventCreate(&ev.e0));
      HIPC(hipEventCreate(&ev.e1));
      HIPC(hipEventRecord(ev.e0, nullptr));
    }
    HIPC(hipMemsetAsync(v.cnt_oh, 0, n_all * 4, nullptr));
    if (!launch_validate_carla(v, size_t(lds_max), nullptr)) throw std::logic_error("validate_carla: LDS check");
    HIPC(hipGetLastError());
    if (a->elapsed_ms) HIPC(hipEventRecord(ev.e1, nullptr));
    HIPC(hipDeviceSynchronize());
    if (a->elapsed_ms) HIPC(hipEventElapsedTime(a->elapsed_ms, ev.e0, ev.e1));
    HIPC(hipMemcpy(a->count, v.count, size_t(K) * 4, hipMemcpyDeviceToHost));
    HIPC(hipMemcpy(a->count_lane, v.count_lane, size_t(K) * 4, hipMemcpyDeviceToHost));
    HIPC(hipMemcpy(a->count_rows, v.count_rows, size_t(K) * 4, hipMemcpyDeviceToHost));
    if (a->count_oh) HIPC(hipMemcpy(a->count_oh, v.cnt_oh, n_oh * 4, hipMemcpyDeviceToHost));
    return MPCMMD_OK;
  });
}

int mpcmmd_validate_carla_risk(const mpcmmd_validate_carla_risk_args* a) {
  if (!a) return fail(MPCMMD_E_INVALID, "null argument");
  const int K = a->num_cfg, O = a->num_obs, H = a->num_prime, R = a->num_rollouts, P = a->num_path;
  const int S = a->num_sigma;
  if (!carla_shape_ok(K, O, H, R, P) || R > (1 << 20))
    return fail(MPCMMD_E_INVALID, "validate_carla_risk: shape out of range");
  if (S < 0 || S > kRiskMaxSigma) return fail(MPCMMD_E_INVALID, "validate_carla_risk: num_sigma out of [0, 8]");
  if (!(a->alpha >= 0.0f && a->alpha <= 1.0f))
    return fail(MPCMMD_E_INVALID, "validate_carla_risk: alpha out of [0, 1]");
  if (int rc = check_noise_variant(a->noise, a->variant, true, MPCMMD_E_INVALID,
                                   "validate_carla_risk: a CARLA variant (static / dynamic optima: "
                                   "mpcmmd_validate_risk)"))
    return rc;
  if (K == 0) return MPCMMD_OK;
  if (!a->init_state || !a->v || !a->steer || !a->x_obs || !a->y_obs || !a->path || !a->keys)
    return fail(MPCMMD_E_INVALID, "null argument");
  if (!a->count_pos || !a->var || !a->cvar || !a->mean || !a->max || (S > 0 && (!a->sigma || !a->mmd)))
    return fail(MPCMMD_E_INVALID, "null argument");
  for (size_t i = 0; i < size_t(K) * S; ++i)
    if (!(std::isfinite(a->sigma[i]) && a->sigma[i] > 0.0f))
      return fail(MPCMMD_E_INVALID, "validate_carla_risk: every sigma must be finite and > 0");
  ValidateRiskParams q{};  // the statistics stages of mpcmmd_validate_risk on the cost buffer (roll unused)
  q.K = K, q.R = R, q.S = S;
  if (mpcmmd_quantile_position(R, a->alpha, &q.lo, &q.hi, &q.w_lo, &q.w_hi) != MPCMMD_OK)
    return fail(MPCMMD_E_INVALID, "validate_carla_risk: quantile position");
  return guarded([&] {
    select_device(a->device);
    int lds_max = 0;
    if (int rc = carla_lds_check("validate_carla_risk", a->device, O, H, P, true, &lds_max)) return rc;
    struct Events {  // declared before the buffers: destroyed after they are freed
      hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};
      ~Events() {
        for (hipEvent_t x : e)
          if (x) (void)hipEventDestroy(x);
      }
    } ev;
    Scratch dev;
    ValidateCarlaParams v{};
    const size_t n_all = carla_plan_params(*a, dev, v), n_oh = size_t(K) * O * H;
    const size_t n3 = size_t(3) * K, nc = n3 * R, T = (size_t(R) + kRiskTile - 1) / kRiskTile;
    v.costs = q.costs = (float*)dev.up(nullptr, nc * 4);  // every element is stored by its row's workgroup
    // one allocation of the per-channel results: count_pos | np | var | cvar | mean | max
    int32_t* res = (int32_t*)dev.up(nullptr, n3 * 6 * 4);
    q.count_pos = res, q.np = res + n3;
    q.var = (float*)(res + 2 * n3), q.cvar = q.var + n3, q.mean = q.cvar + n3, q.vmax = q.mean + n3;
    if (S > 0) {
      q.sigma = (const float*)dev.up(a->sigma, size_t(K) * S * 4);
      q.u = (float*)dev.up(nullptr, nc * 4);
      q.part = (double*)dev.up(nullptr, n3 * T * S * 8);
      q.mmd = (float*)dev.up(nullptr, n3 * S * 4);
    }
    if (a->elapsed_ms)
      for (hipEvent_t& x : ev.e) HIPC(hipEventCreate(&x));
    auto stamp = [&](int i) {
      if (a->elapsed_ms) HIPC(hipEventRecord(ev.e[i], nullptr));
    };
    stamp(0);
    HIPC(hipMemsetAsync(v.cnt_oh, 0, n_all * 4, nullptr));
    if (!launch_validate_carla(v, size_t(lds_max), nullptr))
      throw std::logic_error("validate_carla_risk: LDS check");
    HIPC(hipGetLastError());
    stamp(1);
    launch_vrisk_stats(q, nullptr);
    HIPC(hipGetLastError());
    stamp(2);
    launch_vrisk_mmd(q, nullptr);
    HIPC(hipGetLastError());
    stamp(3);
    HIPC(hipDeviceSynchronize());
    if (a->elapsed_ms)
      for (int i = 0; i < 3; ++i) HIPC(hipEventElapsedTime(a->elapsed_ms + i, ev.e[i], ev.e[i + 1]));
    HIPC(hipMemcpy(a->count_pos, q.count_pos, n3 * 4, hipMemcpyDeviceToHost));
    HIPC(hipMemcpy(a->var, q.var, n3 * 4, hipMemcpyDeviceToHost));
    HIPC(hipMemcpy(a->cvar, q.cvar, n3 * 4, hipMemcpyDeviceToHost));
    HIPC(hipMemcpy(a->mean, q.mean, n3 * 4, hipMemcpyDeviceToHost));
    HIPC(hipMemcpy(a->max, q.vmax, n3 * 4, hipMemcpyDeviceToHost));
    if (S > 0) HIPC(hipMemcpy(a->mmd, q.mmd, n3 * S * 4, hipMemcpyDeviceToHost));
    if (a->costs) HIPC(hipMemcpy(a->costs, q.costs, nc * 4, hipMemcpyDeviceToHost));
    if (a->count) HIPC(hipMemcpy(a->count, v.count, size_t(K) * 4, hipMemcpyDeviceToHost));
    if (a->count_lane) HIPC(hipMemcpy(a->count_lane, v.count_lane, size_t(K) * 4, hipMemcpyDeviceToHost));
    if (a->count_rows) HIPC(hipMemcpy(a->count_rows, v.count_rows, size_t(K) * 4, hipMemcpyDeviceToHost));
    if (a->count_oh) HIPC(hipMemcpy(a->count_oh, v.cnt_oh, n_oh * 4, hipMemcpyDeviceToHost));
    return MPCMMD_OK;
  });
}

int mpcmmd_validate_risk(const mpcmmd_validate_risk_args* a) {
  if (!a) return fail(MPCMMD_E_INVALID, "null argument");
  const int K = a->num_cfg, O = a->num_obs, H = a->num_prime, R = a->num_rollouts, S = a->num_sigma;
  if (K < 0 || K > 65535 || R < 1 || R > (1 << 20) || !validate_shape_ok(O, H))
    return fail(MPCMMD_E_INVALID, "validate_risk: shape out of range");
  if (S < 0 || S > kRiskMaxSigma) return fail(MPCMMD_E_INVALID, "validate_risk: num_sigma out of [0, 8]");
  if (!(a->alpha >= 0.0f && a->alpha <= 1.0f)) return fail(MPCMMD_E_INVALID, "validate_risk: alpha out of [0, 1]");
  if (int rc = check_noise_variant(a->noise, a->variant, false, MPCMMD_E_UNSUPPORTED,
                                   "validate_risk: static / dynamic variants only"))
    return rc;
  if (K == 0) return MPCMMD_OK;
  if (!a->costs_in &&
      (!a->cx || !a->cy || !a->init_state || !a->x_obs || !a->y_obs || !a->keys))
    return fail(MPCMMD_E_INVALID, "null argument");
  if (!a->count_pos || !a->var || !a->cvar || !a->mean || !a->max || (S > 0 && (!a->sigma || !a->mmd)))
    return fail(MPCMMD_E_INVALID, "null argument");
  for (size_t i = 0; i < size_t(K) * S; ++i)
    if (!(std::isfinite(a->sigma[i]) && a->sigma[i] > 0.0f))
      return fail(MPCMMD_E_INVALID, "validate_risk: every sigma must be finite and > 0");
  ValidateRiskParams v{};
  v.K = K, v.R = R, v.S = S;
  if (mpcmmd_quantile_position(R, a->alpha, &v.lo, &v.hi, &v.w_lo, &v.w_hi) != MPCMMD_OK)
    return fail(MPCMMD_E_INVALID, "validate_risk: quantile position");
  return guarded([&] {
    select_device(a->device);
    struct Events {  // declared before the buffers: destroyed after they are freed
      hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};
      ~Events() {
        for (hipEvent_t x : e)
          if (x) (void)hipEventDestroy(x);
      }
    } ev;
    Scratch dev;
    const size_t n3 = size_t(3) * K, nc = n3 * R, T = (size_t(R) + kRiskTile - 1) / kRiskTile;
    v.costs = (float*)dev.up(a->costs_in, nc * 4);
    if (!a->costs_in) plan_params(*a, dev, v.roll);
    // one allocation of the per-channel results: count_pos | np | var | cvar | mean | max
    int32_t* res = (int32_t*)dev.up(nullptr, n3 * 6 * 4);
    v.count_pos = res, v.np = res + n3;
    v.var = (float*)(res + 2 * n3), v.cvar = v.var + n3, v.mean = v.cvar + n3, v.vmax = v.mean + n3;
    if (S > 0) {
      v.sigma = (const float*)dev.up(a->sigma, size_t(K) * S * 4);
      v.u = (float*)dev.up(nullptr, nc * 4);
      v.part = (double*)dev.up(nullptr, n3 * T * S * 8);
      v.mmd = (float*)dev.up(nullptr, n3 * S * 4);
    }
    if (a->elapsed_ms)
      for (hipEvent_t& x : ev.e) HIPC(hipEventCreate(&x));
    auto stamp = [&](int i) {
      if (a->elapsed_ms) HIPC(hipEventRecord(ev.e[i], nullptr));
    };
    stamp(0);
    if (!a->costs_in) launch_vrisk_roll(v, nullptr);
    HIPC(hipGetLastError());
    stamp(1);
    launch_vrisk_stats(v, nullptr);
    HIPC(hipGetLastError());
    stamp(2);
    launch_vrisk_mmd(v, nullptr);
    HIPC(hipGetLastError());
    stamp(3);
    HIPC(hipDeviceSynchronize());
    if (a->elapsed_ms)
      for (int i = 0; i < 3; ++i) HIPC(hipEventElapsedTime(a->elapsed_ms + i, ev.e[i], ev.e[i + 1]));
    HIPC(hipMemcpy(a->count_pos, v.count_pos, n3 * 4, hipMemcpyDeviceToHost));
    HIPC(hipMemcpy(a->var, v.var, n3 * 4, hipMemcpyDeviceToHost));
    HIPC(hipMemcpy(a->cvar, v.cvar, n3 * 4, hipMemcpyDeviceToHost));
    HIPC(hipMemcpy(a->mean, v.mean, n3 * 4, hipMemcpyDeviceToHost));
    HIPC(hipMemcpy(a->max, v.vmax, n3 * 4, hipMemcpyDeviceToHost));
    if (S > 0) HIPC(hipMemcpy(a->mmd, v.mmd, n3 * S * 4, hipMemcpyDeviceToHost));
    if (a->costs) HIPC(hipMemcpy(a->costs, v.costs, nc * 4, hipMemcpyDeviceToHost));
    return MPCMMD_OK;
  });
}

}  // extern "C"
