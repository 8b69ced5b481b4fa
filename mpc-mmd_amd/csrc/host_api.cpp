// libmpcmmd: the entry points that never touch a GPU, the thread's last error
// and mpcmmd_create_batch's range checks.  No HIP: compiled by g++ and built a
// second time under ASan/UBSan (tests/native/asan_host.cpp).
#include "host_api.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "layout.hpp"

using namespace mpcmmd;

namespace {
thread_local std::string g_err;
}

int mpcmmd::fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

PathView mpcmmd::view_of(const mpcmmd_path& p) {
  return path_view(p.num_path, p.x_path, p.y_path, p.arc_vec, p.Fx_dot, p.Fy_dot, p.kappa);
}

int mpcmmd::check_create_ranges(const mpcmmd_config& c, int32_t max_configs) {
  if (c.num_reduced < 2 || c.num_obs < 1 || c.num_prime < 2 || c.num_prime > 100 || c.num_batch < 20 ||
      c.num_batch > 4096 || c.maxiter_cem < 1 || (c.noise != 0 && c.noise != 1) || c.variant < 0 || c.variant > 3)
    return fail(MPCMMD_E_INVALID,
                "config out of range (num_reduced>=2, num_obs>=1, 2<=num_prime<=100, 20<=num_batch<=4096)");
  if (c.num_reduced > 1024) return fail(MPCMMD_E_UNSUPPORTED, "num_reduced > 1024");
  if (size_t(c.num_obs) * c.num_prime > 8192) return fail(MPCMMD_E_UNSUPPORTED, "num_obs * num_prime > 8192");
  if (max_configs < 1) return fail(MPCMMD_E_INVALID, "max_configs must be >= 1");
  // grid limits: candidates on grid y / z (<= 65535), Beta fix-up list entries (32-bit)
  const size_t Bt = size_t(max_configs) * c.num_batch;
  if (Bt > 65535 || Bt * c.num_prime * c.num_reduced >= (size_t(1) << 32))
    return fail(MPCMMD_E_UNSUPPORTED, "max_configs * num_batch too large (<= 65535 candidates per handle)");
  return MPCMMD_OK;
}

extern "C" {

int32_t mpcmmd_abi_version(void) { return MPCMMD_ABI_VERSION; }
const char* mpcmmd_last_error(void) { return g_err.c_str(); }

int mpcmmd_path_smoothing(int32_t num_path, const float* x_wp, const float* y_wp, float threshold, float* x_path,
                          float* y_path) {
  if (num_path < 4 || num_path > kMaxPath || !x_wp || !y_wp || !x_path || !y_path)
    return fail(MPCMMD_E_INVALID, "path smoothing: 4 <= num_path <= 2048, non-null arrays");
  try {
    path_smoothing(num_path, x_wp, y_wp, threshold, x_path, y_path);
    return MPCMMD_OK;
  } catch (const std::exception& e) {
    return fail(MPCMMD_E_INVALID, e.what());
  }
}

int mpcmmd_path_parameters(int32_t num_path, const float* x_path, const float* y_path, float* Fx_dot, float* Fy_dot,
                           float* Fx_ddot, float* Fy_ddot, float* arc_vec, float* kappa, float* arc_length) {
  if (num_path < 3 || !x_path || !y_path || !Fx_dot || !Fy_dot || !Fx_ddot || !Fy_ddot || !arc_vec || !kappa)
    return fail(MPCMMD_E_INVALID, "path parameters: num_path >= 3, non-null arrays");
  try {
    path_parameters(num_path, x_path, y_path, Fx_dot, Fy_dot, Fx_ddot, Fy_ddot, arc_vec, kappa, arc_length);
    return MPCMMD_OK;
  } catch (const std::exception& e) {
    return fail(MPCMMD_E_INVALID, e.what());
  }
}

int mpcmmd_global_to_frenet(const mpcmmd_path* path, int32_t count, const float* x, const float* y, const float* v,
                            const float* vdot, const float* psi, const float* psidot, float* out) {
  if (!path || count < 0 || (count > 0 && (!x || !y || !v || !vdot || !psi || !psidot || !out)))
    return fail(MPCMMD_E_INVALID, "null argument");
  if (path->num_path < 2 || !path->x_path || !path->y_path || !path->arc_vec || !path->Fx_dot || !path->Fy_dot ||
      !path->kappa)
    return fail(MPCMMD_E_INVALID, "path: num_path >= 2 and six arrays");
  const PathView pv = view_of(*path);
  for (int i = 0; i < count; ++i) {
    const FrenetState f = global_to_frenet(pv, x[i], y[i], v[i], vdot[i], psi[i], psidot[i]);
    float* o = out + size_t(i) * 7;
    o[0] = f.x, o[1] = f.y, o[2] = f.vx, o[3] = f.vy, o[4] = f.ax, o[5] = f.ay, o[6] = f.psi;
  }
  return MPCMMD_OK;
}

int mpcmmd_carla_tick_host(int32_t num_path, int32_t num_obs, const float init_state[6], const float* x_wp,
                           const float* y_wp, const float* obstacles, float threshold, float* path6, float* x_obs,
                           float* y_obs) {
  if (num_path < 4 || num_path > kMaxPath) return fail(MPCMMD_E_INVALID, "tick: 4 <= num_path <= 2048");
  if (num_obs < 0 || !init_state || !x_wp || !y_wp || !path6 || (num_obs > 0 && (!obstacles || !x_obs || !y_obs)))
    return fail(MPCMMD_E_INVALID, "null argument");
  if (!std::isfinite(threshold)) return fail(MPCMMD_E_INVALID, "tick: threshold must be finite");
  try {
    carla_tick_host(num_path, num_obs, x_wp, y_wp, obstacles, threshold, path6, x_obs, y_obs);
    return MPCMMD_OK;
  } catch (const std::exception& e) {
    return fail(MPCMMD_E_INVALID, e.what());
  }
}

int mpcmmd_host_constant(const mpcmmd_config* cfg, const char* name, double* dst, size_t count) {
  if (!cfg || !name) return fail(MPCMMD_E_INVALID, "null argument");
  try {
    ProblemConsts c = build_constants(cfg->num_prime, cfg->variant);
    const std::vector<double>* v = nullptr;
    std::string n(name);
    if (n == "P") v = &c.P;
    else if (n == "Pdot") v = &c.Pd;
    else if (n == "Pddot") v = &c.Pdd;
    else if (n == "P_prime") v = &c.P_prime;
    else if (n == "P64") v = &c.P64;
    else if (n == "Pdot64") v = &c.Pd64;
    else if (n == "Pddot64") v = &c.Pdd64;
    else if (n == "guess_kinv_x") v = &c.guess_kinv_x;
    else if (n == "guess_kinv_y") v = &c.guess_kinv_y;
    else if (n == "proj_kinv_x") v = &c.proj_kinv_x;
    else if (n == "proj_kinv_y") v = &c.proj_kinv_y;
    else if (n == "fit") v = &c.fit;
    std::vector<double> dk[2];
    if (n == "det_kinv_x" || n == "det_kinv_y") {
      det_projection_kinv(c, cfg->num_obs, dk[0], dk[1]);
      v = &dk[n == "det_kinv_y" ? 1 : 0];
    }
    // the variant's scalars the synthetic closed loop's model takes (mpcmmd_mpc_model): y_lb, y_ub, K_steer
    const std::vector<double> mpc_scalars = {c.y_lb, c.y_ub, c.K_steer};
    if (n == "mpc_scalars") v = &mpc_scalars;
    if (!v) return fail(MPCMMD_E_INVALID, "unknown constant " + n);
    if (dst) {
      if (count < v->size()) return fail(MPCMMD_E_INVALID, "dst too small");
      std::memcpy(dst, v->data(), v->size() * 8);
    }
    return int(v->size());
  } catch (const std::exception& e) {
    return fail(MPCMMD_E_INVALID, e.what());
  }
}

int mpcmmd_obs_dynamic_traj(int32_t num_obs, const float* x0, const float* y0, const float* vx0, const float* vy0,
                            const float* v_des, float y_des, float* x_traj, float* y_traj) {
  if (num_obs < 0) return fail(MPCMMD_E_INVALID, "num_obs < 0");
  if (num_obs > 0 && (!x0 || !y0 || !vx0 || !vy0 || !v_des || !x_traj || !y_traj))
    return fail(MPCMMD_E_INVALID, "null argument");
  try {
    static const DynObsConsts c = build_dyn_obs_consts();
    dyn_obs_traj(c, num_obs, x0, y0, vx0, vy0, v_des, y_des, x_traj, y_traj);
    return MPCMMD_OK;
  } catch (const std::exception& e) {
    return fail(MPCMMD_E_INVALID, e.what());
  }
}

// The linear quantile's position among n ascending samples with JAX's fp32
// weights (jnp.quantile: pos = alpha (n - 1) in fp32, low = floor, w = pos -
// low).  mpcmmd_validate_risk takes its order statistics from here.
int mpcmmd_quantile_position(int32_t n, float alpha, int32_t* lo, int32_t* hi, float* w_lo, float* w_hi) {
  if (n < 1 || !(alpha >= 0.0f && alpha <= 1.0f) || !lo || !hi || !w_lo || !w_hi) return MPCMMD_E_INVALID;
  const float pos = alpha * float(n - 1);
  const float fl = std::floor(pos), ce = std::ceil(pos);
  const float hw = pos - fl;
  *w_hi = hw;
  *w_lo = 1.0f - hw;
  *lo = int32_t(std::min(std::max(fl, 0.0f), float(n - 1)));
  *hi = int32_t(std::min(std::max(ce, 0.0f), float(n - 1)));
  return MPCMMD_OK;
}

}  // extern "C"
