// The receding-horizon world of the synthetic variants,
// written once for the host twin (mpc_host.cpp, g++) and the kernel
// (k_mpc.hip): every per-element expression of a step.  The world is the
// optimizer's own rollout model with one realised draw: compute_controls at
// step 0, the noisy_from perturbation, bicycle_step_cr_t's step with wheel base
// 2.5, constant-velocity vehicles.  fp32 in the order written
// (-ffp-contract=off), transcendentals evaluated in fp64 and rounded once, the
// ego position in fp64.  The two callers differ only in how they spread the
// elements over threads and in the Math policy that names the fp64
// transcendentals (host libm / OCML).  No HIP header: plain C++ with an
// attribute macro (world_step.hpp's).
#pragma once
#include "world_step.hpp"  // canon_nan, world_pop (initial_population with a given factor)

namespace mpcmmd {

constexpr int kMpcMaxObs = 64;          // vehicles: one lane of a wave each
constexpr float kMpcWheelBase = 2.5f;   // cem.py:26
constexpr float kMpcPlanDt = 0.15f;     // prob.t: the spacing of the plan's points (cem.py:40)
constexpr int kMpcTrack = 100;          // points of an obstacle track

// The scalars of a model (mpcmmd_mpc_model without its arrays).
struct MpcScalars {
  int O, B, noise;
  float dt, sigma_acc, sigma_steer, acc_const, steer_const, K_steer, a_obs, b_obs, y_lb, y_ub, goal_x;
};

WORLD_FN double canon_nan64(double x) { return x != x ? __builtin_bit_cast(double, 0x7FF8000000000000ull) : x; }

// ---- controller: compute_controls at step 0 (S/opt/cem_helper.py:540-551) ----------
struct MpcControl {
  float a_c, s_c, curv, a, s;
};

// one element of Pdot cx as plan_speed forms it: a sequential fp64 sum, rounded once
WORLD_FN float mpc_row_dot(const double* row, const float* c) {
  double s = 0.0;
  for (int k = 0; k < 11; ++k) s += row[k] * double(c[k]);
  return float(s);
}

// pdot2: rows 0, 1 of Pdot; pddot1: row 0 of Pddot.  M::atan64 is the fp64 arctangent.
template <class M>
WORLD_FN MpcControl mpc_controller(const double* pdot2, const double* pddot1, const float* cx, const float* cy) {
  const float xd0 = mpc_row_dot(pdot2, cx), yd0 = mpc_row_dot(pdot2, cy);
  const float xd1 = mpc_row_dot(pdot2 + 11, cx), yd1 = mpc_row_dot(pdot2 + 11, cy);
  const float xdd0 = mpc_row_dot(pddot1, cx), ydd0 = mpc_row_dot(pddot1, cy);
  const float v0 = sqrtf(xd0 * xd0 + yd0 * yd0), v1 = sqrtf(xd1 * xd1 + yd1 * yd1);
  MpcControl c;
  c.a_c = canon_nan((v1 - v0) / kMpcPlanDt);
  const float s2 = xd0 * xd0 + yd0 * yd0;
  c.curv = canon_nan((ydd0 * xd0 - yd0 * xdd0) / (s2 * sqrtf(s2)));
  c.s_c = canon_nan(float(M::atan64(double(c.curv * kMpcWheelBase))));
  c.a = c.s = 0.0f;
  return c;
}

// the optimizer's noisy_from (rollout.hpp) on one realised draw u[3]; K_steer holds
// float32(K_steer * sigma_steer) as Params::K_steer does
WORLD_FN void mpc_perturb(const MpcScalars& w, const float* u, MpcControl& c) {
  float ap, sp;
  if (w.noise == 0) {
    ap = (w.sigma_acc * fabsf(c.a_c)) * u[0];
    sp = (w.sigma_steer * fabsf(c.s_c)) * u[1];
  } else {
    ap = w.sigma_acc * (2.0f * u[0] - 1.0f);
    sp = w.K_steer * (2.0f * u[1] - 1.0f);
  }
  c.a = canon_nan((c.a_c + ap) + w.acc_const * u[2]);
  c.s = canon_nan((c.s_c + sp) + w.steer_const * u[2]);
}

// ---- ego: bicycle_step_cr_t's expression (rollout.hpp) with the model's dt ----------
struct MpcEgo {
  double x, y;
  float vx, vy, psi;
};

// the step, and the accelerations (vx' - vx) / dt, (vy' - vy) / dt of the next init_state
template <class M>
WORLD_FN MpcEgo mpc_ego_step(const MpcEgo& e, float a, float s, float dt, float* ax, float* ay) {
  MpcEgo n;
  float v = sqrtf(e.vx * e.vx + e.vy * e.vy);
  v = v + a * dt;
  const float tn = float(M::tan64(double(s)));
  const float psidot = (v * tn) / kMpcWheelBase;
  n.psi = canon_nan(e.psi + psidot * dt);
  double sp, cp;
  M::sincos64(double(n.psi), sp, cp);
  n.vx = canon_nan(v * float(cp));
  n.vy = canon_nan(v * float(sp));
  n.x = canon_nan64(e.x + double(n.vx * dt));
  n.y = canon_nan64(e.y + double(n.vy * dt));
  *ax = canon_nan((n.vx - e.vx) / dt);
  *ay = canon_nan((n.vy - e.vy) / dt);
  return n;
}

// ---- vehicles and flags -----------------------------------------------------------
// 1 - (dx / a)^2 - (dy / b)^2 of the ego against vehicle row (x, y, vx, vy)
WORLD_FN float mpc_clear_term(const MpcScalars& w, const MpcEgo& e, const float* veh) {
  const float dx = float(e.x - double(veh[0])), dy = float(e.y - double(veh[1]));
  const float lo = dx / w.a_obs, la = dy / w.b_obs;
  return canon_nan(1.0f - lo * lo - la * la);
}

// np.linspace(0, 15, 100).astype(float32)[k]
WORLD_FN float mpc_track_time(int k) { return k == kMpcTrack - 1 ? 15.0f : float(double(k) * (15.0 / 99.0)); }

// point k of a vehicle's constant-velocity track: c + v tt[k]
WORLD_FN float mpc_track(float c, float v, int k) { return c + v * mpc_track_time(k); }

WORLD_FN bool mpc_lane_out(const MpcScalars& w, const MpcEgo& e) { return e.y < double(w.y_lb) || e.y > double(w.y_ub); }
WORLD_FN bool mpc_goal(const MpcScalars& w, const MpcEgo& e) { return e.x >= double(w.goal_x); }

// ---- the next solve's st0 (solve_host.cpp: initial_state) ---------------------------
// initial_state takes the heading as the host libm's atan2f(vy, vx), which is not
// correctly rounded, so no fp64 evaluation reproduces it.  This is that routine's
// algorithm (the fdlibm single-precision atan2 / atan, as glibc before 2.41 ships
// them) restated operation for operation in plain fp32, so the kernel forms the
// bits the host route uploads; tests/test_mpc_host.py holds it against the libm.
WORLD_FN float mpc_atanf(float x) {
  // the routine's own decimal literals (its hex comments differ from them in places)
  const float hi[4] = {4.6364760399e-01f, 7.8539812565e-01f, 9.8279368877e-01f, 1.5707962513e+00f};
  const float lo[4] = {5.0121582440e-09f, 3.7748947079e-08f, 3.4473217170e-08f, 7.5497894159e-08f};
  const float aT[11] = {3.3333334327e-01f,  -2.0000000298e-01f, 1.4285714924e-01f, -1.1111110449e-01f,
                        9.0908870101e-02f,  -7.6918758452e-02f, 6.6610731184e-02f, -5.8335702866e-02f,
                        4.9768779427e-02f,  -3.6531571299e-02f, 1.6285819933e-02f};
  const int32_t hx = __builtin_bit_cast(int32_t, x), ix = hx & 0x7fffffff;
  int id;
  if (ix >= 0x4c000000) {  // |x| >= 2^25
    if (ix > 0x7f800000) return x + x;
    return hx > 0 ? hi[3] + lo[3] : -hi[3] - lo[3];
  }
  if (ix < 0x3ee00000) {  // |x| < 0.4375
    if (ix < 0x31000000) return x;  // |x| < 2^-29
    id = -1;
  } else {
    x = fabsf(x);
    if (ix < 0x3f980000) {  // |x| < 1.1875
      if (ix < 0x3f300000) id = 0, x = (2.0f * x - 1.0f) / (2.0f + x);
      else id = 1, x = (x - 1.0f) / (x + 1.0f);
    } else {
      if (ix < 0x401c0000) id = 2, x = (x - 1.5f) / (1.0f + 1.5f * x);
      else id = 3, x = -1.0f / x;
    }
  }
  const float z = x * x, w = z * z;
  const float s1 = z * (aT[0] + w * (aT[2] + w * (aT[4] + w * (aT[6] + w * (aT[8] + w * aT[10])))));
  const float s2 = w * (aT[1] + w * (aT[3] + w * (aT[5] + w * (aT[7] + w * aT[9]))));
  if (id < 0) return x - x * (s1 + s2);
  const float r = hi[id] - ((x * (s1 + s2) - lo[id]) - x);
  return hx < 0 ? -r : r;
}

WORLD_FN float mpc_atan2f(float y, float x) {
  const float tiny = 1.0e-30f, pi_o_4 = __builtin_bit_cast(float, 0x3f490fdbu);
  const float pi_o_2 = __builtin_bit_cast(float, 0x3fc90fdbu), pi = __builtin_bit_cast(float, 0x40490fdbu);
  const float pi_lo = __builtin_bit_cast(float, 0xb3bbbd2eu);
  const int32_t hx = __builtin_bit_cast(int32_t, x), hy = __builtin_bit_cast(int32_t, y);
  const int32_t ix = hx & 0x7fffffff, iy = hy & 0x7fffffff;
  if (ix > 0x7f800000 || iy > 0x7f800000) return canon_nan(x + y);
  if (hx == 0x3f800000) return mpc_atanf(y);
  const int m = ((hy >> 31) & 1) | ((hx >> 30) & 2);  // 2 sign(x) + sign(y)
  if (iy == 0) return m < 2 ? y : (m == 2 ? pi + tiny : -pi - tiny);
  if (ix == 0) return hy < 0 ? -pi_o_2 - tiny : pi_o_2 + tiny;
  if (ix == 0x7f800000) {
    if (iy == 0x7f800000)
      return m == 0 ? pi_o_4 + tiny : m == 1 ? -pi_o_4 - tiny : m == 2 ? 3.0f * pi_o_4 + tiny : -3.0f * pi_o_4 - tiny;
    return m == 0 ? 0.0f : m == 1 ? -0.0f : m == 2 ? pi + tiny : -pi - tiny;
  }
  if (iy == 0x7f800000) return hy < 0 ? -pi_o_2 - tiny : pi_o_2 + tiny;
  const int32_t k = (iy - ix) >> 23;
  float z;
  if (k > 60) z = pi_o_2 + 0.5f * pi_lo;
  else if (hx < 0 && k < -60) z = 0.0f;
  else z = mpc_atanf(fabsf(y / x));
  if (m == 0) return z;
  if (m == 1) return -z;
  if (m == 2) return pi - (z - pi_lo);
  return (z - pi_lo) - pi;
}

// the next init_state: the position rounded, the velocity, the accelerations of the step
WORLD_FN void mpc_init_state(const MpcEgo& e, float ax, float ay, float* init) {
  init[0] = canon_nan(float(e.x)), init[1] = canon_nan(float(e.y));
  init[2] = e.vx, init[3] = e.vy, init[4] = ax, init[5] = ay;
}

// initial_state of the init_state (x, y, vx, vy, ax, ay)
WORLD_FN void mpc_st0(const float* init, float* s0) {
  s0[0] = init[0], s0[1] = init[1], s0[2] = init[2], s0[3] = init[3], s0[4] = mpc_atan2f(init[3], init[2]);
  s0[5] = s0[6] = s0[7] = 0.0f;
}

// element k of solve_c (solve_host.cpp: solve_columns) from the packed KKT columns kcol [4][11][4]:
// bx = (x, vx, ax), by = (y, vy, ay, 0), the products added in order to 0.0
WORLD_FN double mpc_solve_column(const double* kcol, const float* init, int k) {
  const bool isy = (k / 11) & 1;
  const double b[4] = {double(init[isy ? 1 : 0]), double(init[isy ? 3 : 2]), double(init[isy ? 5 : 4]), 0.0};
  const double* a = kcol + size_t(k) * 4;
  double sc = 0.0;
  const int ne = isy ? 4 : 3;
  for (int e = 0; e < ne; ++e) sc += a[e] * b[e];
  return sc;
}

}  // namespace mpcmmd
