// The surrogate world's arithmetic, written once for
// the host twin (world_host.cpp, g++) and the kernel (k_world.hip): every
// per-element expression of a world step.  The two callers differ only in how
// they spread the elements over threads and in the Math policy that names the
// transcendentals (host libm / OCML, each evaluated in fp64 and rounded once).
// No HIP header: plain C++ with an attribute macro.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define WORLD_FN __host__ __device__ inline
#else
#define WORLD_FN inline
#endif

namespace mpcmmd {

constexpr int kWorldMaxObs = 64;       // vehicles in a world, and obstacles handed to the optimizer
constexpr float kWheelBase = 2.875f;   // compute_rollout_one_step (C/opt/cem_helper.py:732-751)
constexpr double kGoalRadius = 7.0;    // main_carla.py:329
constexpr double kBehind = 5.0 * 3.141592653589793 / 6.0;  // compute_obs_data's 5 pi / 6 (main_carla.py:87-90)
constexpr uint32_t kQuietNaN = 0x7FC00000u;

// The scalars of a world model (mpcmmd_world_model without its arrays).
struct WorldScalars {
  int P, O, total, n_route, goal_index, B, noise;
  float dt, sigma_acc, sigma_steer, acc_const, steer_const, steer_max, a_obs, b_obs, y_lb, y_ub;
};

// An fp32 output formed by a subtraction stores every NaN as the quiet NaN
// 0x7FC00000: IEEE 754 leaves a NaN result's sign open, and gfx950 forms a - b
// as a + (-b), which flips the sign of a NaN b where the host keeps it.
WORLD_FN float canon_nan(float x) { return x != x ? __builtin_bit_cast(float, kQuietNaN) : x; }

// np.clip on one value: NaN stays NaN
WORLD_FN float clip_sym(float x, float m) { return x < -m ? -m : (x > m ? m : x); }

// ---- controller and perturbation (main_carla.py:408-436) ------------------------
struct WorldControl {
  float a_c, s_c, a, s;
};

// v_best[0..3] as plan_speed forms them and the means: a_c, s_c (a, s not set)
WORLD_FN WorldControl world_controller(const WorldScalars& w, const double* pdot4, const float* cx, const float* cy,
                                       const float* steer, float v) {
  float vb[4];
  for (int i = 0; i < 4; ++i) {
    double sx = 0.0, sy = 0.0;
    for (int k = 0; k < 11; ++k) {
      sx += pdot4[i * 11 + k] * double(cx[k]);
      sy += pdot4[i * 11 + k] * double(cy[k]);
    }
    const float xd = float(sx), yd = float(sy);
    vb[i] = sqrtf(xd * xd + yd * yd);
  }
  WorldControl c;
  const float v_c = (((vb[0] + vb[1]) + vb[2]) + vb[3]) / 4.0f;
  c.s_c = clip_sym((((steer[0] + steer[1]) + steer[2]) + steer[3]) / 4.0f, w.steer_max);
  c.a_c = (v_c - v) / (3.0f * 0.15f);
  c.a = c.s = 0.0f;
  return c;
}

// the perturbed controls from the variates u[4] (given, or drawn once a_c and s_c are known)
WORLD_FN void world_perturb(const WorldScalars& w, const float* u, WorldControl& c) {
  if (w.noise == 0) {  // one normal for both controls (main_carla.py:418-421)
    c.a = (c.a_c + (w.sigma_acc * fabsf(c.a_c)) * u[0]) + w.acc_const * u[2];
    c.s = (c.s_c + (w.sigma_steer * fabsf(c.s_c)) * u[0]) + w.steer_const * u[3];
  } else {
    c.a = (c.a_c + w.sigma_acc * (2.0f * u[0] - 1.0f)) + w.acc_const * u[2];
    c.s = (c.s_c + w.sigma_steer * (2.0f * u[1] - 1.0f)) + w.steer_const * u[3];
  }
  c.s = clip_sym(c.s, w.steer_max);  // stands in for CARLA's normalised steer clamp
}

// ---- ego (compute_rollout_one_step with the world's dt) --------------------------
struct WorldEgo {
  double x, y;
  float v, psi, psidot;
};

template <class M>
WORLD_FN WorldEgo world_ego_step(const WorldEgo& e, float a, float s, float dt) {
  WorldEgo n;
  const float vn = e.v + a * dt;
  n.v = vn < 0.0f ? 0.0f : vn;
  n.psidot = n.v * M::tan(s) / kWheelBase;
  const float psi = e.psi + n.psidot * dt;
  float sn, cs;
  M::sincos(psi, sn, cs);
  n.x = e.x + double(n.v * cs * dt);
  n.y = e.y + double(n.v * sn * dt);
  n.psi = M::atan2(sn, cs);
  return n;
}

// ---- flags -------------------------------------------------------------------------
// 1 - (longitudinal / a)^2 - (lateral / b)^2 of the ego in vehicle o's frame
template <class M>
WORLD_FN float clear_term(const WorldScalars& w, const WorldEgo& e, const float* veh) {
  const float dx = float(e.x - double(veh[0])), dy = float(e.y - double(veh[1]));
  float sn, cs;
  M::sincos(veh[4], sn, cs);
  const float lo = (dx * cs + dy * sn) / w.a_obs, la = (-dx * sn + dy * cs) / w.b_obs;
  return 1.0f - lo * lo - la * la;
}

// ---- route ------------------------------------------------------------------------
// Key of route point j for the argmin: the fp64 distance's bit pattern + 1, 0
// for a NaN, so the smallest (key, j) is np.argmin of the sqrt values (the
// first minimum, the first NaN if any): the rule test_gpu_frenet_ties.py pins
// for frenet_point_quad, in fp64.
WORLD_FN uint64_t route_key(double ex, double ey, double rx, double ry) {
  const double dx = ex - rx, dy = ey - ry;
  const double d = sqrt(dx * dx + dy * dy);
  if (d != d) return 0;
  return __builtin_bit_cast(uint64_t, d) + 1;
}

// the spline piece that holds s: the last breakpoint <= s, within [0, n - 2] (scipy's extrapolation)
WORLD_FN int spline_piece(const double* arc, int n, double s) {
  int lo = 0, hi = n - 1;  // arc[lo] <= s < arc[hi] once s is inside
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (arc[mid] <= s) lo = mid; else hi = mid;
  }
  return lo;
}

// scipy PPoly's evaluation order: res = c3; z = h; res += c2 z; z *= h; ...
WORLD_FN double spline_eval(const double* c, int n, int i, double h) {
  const int m = n - 1;
  double res = 0.0, z = 1.0;
  res = res + c[3 * m + i] * z;
  z *= h;
  res = res + c[2 * m + i] * z;
  z *= h;
  res = res + c[1 * m + i] * z;
  z *= h;
  res = res + c[0 * m + i] * z;
  return res;
}

WORLD_FN double spline_slope(const double* c, int n, int i, double h) {
  const int m = n - 1;
  return (3.0 * c[0 * m + i] * h + 2.0 * c[1 * m + i]) * h + c[2 * m + i];
}

// np.linspace(s0, s0 + 300, P)[i]
WORLD_FN double look_at(double s0, int P, int i) {
  const double stop = s0 + 300.0;
  if (P > 1 && i == P - 1) return stop;
  const double step = P > 1 ? (stop - s0) / double(P - 1) : 0.0;
  return double(i) * step + s0;
}

// waypoint i of the next tick, shifted to the ego and rounded
WORLD_FN void world_waypoint(const WorldScalars& w, const double* arc, const double* sx, const double* sy, double s0,
                             const WorldEgo& e, int i, float* xw, float* yw) {
  const double s = look_at(s0, w.P, i);
  const int p = spline_piece(arc, w.n_route, s);
  const double h = s - arc[p];
  *xw = canon_nan(float(spline_eval(sx, w.n_route, p, h) - e.x));
  *yw = canon_nan(float(spline_eval(sy, w.n_route, p, h) - e.y));
}

// signed lateral offset from the route at point idx (left positive), heading from the spline slopes
WORLD_FN float world_lateral(const WorldScalars& w, const double* rx, const double* ry, const double* arc,
                             const double* sx, const double* sy, int idx, const WorldEgo& e) {
  const int p = idx < w.n_route - 1 ? idx : w.n_route - 2;
  const double h = arc[idx] - arc[p];
  const double tx = spline_slope(sx, w.n_route, p, h), ty = spline_slope(sy, w.n_route, p, h);
  return canon_nan(float((-(e.x - rx[idx]) * ty + (e.y - ry[idx]) * tx) / sqrt(tx * tx + ty * ty)));
}

WORLD_FN bool world_goal(const WorldScalars& w, const double* rx, const double* ry, const WorldEgo& e) {
  const double dx = e.x - rx[w.goal_index], dy = e.y - ry[w.goal_index];
  return sqrt(dx * dx + dy * dy) < kGoalRadius;
}

// ---- obstacles (compute_obs_data, as replay.nearest_obstacles restates it) ---------
// not behind the ego: arccos(clip(rel . (v heading), -1, 1)) <= 5 pi / 6, all in
// fp64 as the restatement has it (the dot product is not normalised: the
// reference's quirk)
template <class M>
WORLD_FN bool obstacle_kept(const WorldEgo& e, const float* veh) {
  const double r0 = double(veh[0]) - e.x, r1 = double(veh[1]) - e.y;
  double sn, cs;
  M::sincos64(double(e.psi), sn, cs);
  const double h0 = double(e.v) * cs, h1 = double(e.v) * sn;
  double dot = r0 * h0 + r1 * h1;
  dot = dot < -1.0 ? -1.0 : (dot > 1.0 ? 1.0 : dot);
  return M::acos64(dot) <= kBehind;
}

// an obstacle's coordinate shifted to the ego
WORLD_FN float obstacle_shift(float c, double ego) { return canon_nan(float(double(c) - ego)); }

WORLD_FN double obstacle_dist2(const WorldEgo& e, float x, float y) {
  const double dx = e.x - double(x), dy = e.y - double(y);
  return dx * dx + dy * dy;
}

// a sorts before b in the stable sort by distance: ascending, every NaN last, ties by position
WORLD_FN bool dist_before(double a, int ia, double b, int ib) {
  const bool na = a != a, nb = b != b;
  if (na || nb) return na == nb ? ia < ib : nb;
  return a < b || (a == b && ia < ib);
}

// ---- first population (initial_population of solve_host.cpp with a given factor) ---
WORLD_FN float world_pop(const float* mean, const double* L, const float* z, int a) {
  double s = double(mean[a]);
  for (int c = 0; c <= a; ++c) s += L[a * 8 + c] * double(z[c]);
  float v = float(s);
  if (a < 4) v = fminf(fmaxf(v, 0.1f), 30.0f);
  return v;
}

}  // namespace mpcmmd
