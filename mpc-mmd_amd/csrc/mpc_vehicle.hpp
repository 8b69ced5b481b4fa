// Planned vehicles of the synthetic closed loop, written
// once for the host twin (mpc_host.cpp, g++) and the kernel (k_mpc.hip): a
// vehicle follows the dynamic driver's lane-tracking QP (obs_data.
// compute_obs_guess, host_constants.hpp: DynObsConsts) and re-plans it every
// tick from its own state S = (x, y, vx, vy, ax, ay) towards its constant
// target (v_des, y_des).  Three pure functions, each element a sequential fp64
// sum started at 0.0 and rounded once to fp32 (-ffp-contract=off), every
// rounded value stored through canon_nan; no transcendental, so the host's and
// the device's bits agree unconditionally.  No HIP header: plain C++ with
// world_step.hpp's attribute macro.
#pragma once
#include "world_step.hpp"  // WORLD_FN, canon_nan

namespace mpcmmd {

constexpr int kVehCoef = 22;  // cxf[11], cyf[11] of one vehicle

// The constants: build_dyn_obs_consts()'s, and the basis rows at the tick length.
struct MpcVehConsts {
  const double* kinv_x;    // [14][14]
  const double* kinv_y;    // [15][15]
  const double* colsum_x;  // [11]
  const double* colsum_y;  // [11]
  const double* P;         // [100][11] the fp32-rounded basis
  const double* adv;       // [3][11] rows P, Pdot, Pddot at double(dt), fp32-rounded
};

// plan: coefficient j of the QP's solution from S [6] and target [2]; j < 11 is cxf[j], else
// cyf[j - 11].  With ax = ay = 0 this is dyn_obs_traj's sum: a term k * 0.0 adds +0.0.
WORLD_FN float mpc_veh_coef(const MpcVehConsts& c, const float* S, const float* target, int j) {
  double s = 0.0;
  if (j < 11) {
    const double tv = -2.0 * double(target[0]);
    const double* k = c.kinv_x + j * 14;
    for (int i = 0; i < 11; ++i) s += k[i] * (tv * c.colsum_x[i]);
    s += k[11] * double(S[0]);
    s += k[12] * double(S[2]);
    s += k[13] * double(S[4]);
  } else {
    const double ty = -2.0 * double(target[1]);
    const double* k = c.kinv_y + (j - 11) * 15;
    for (int i = 0; i < 11; ++i) s += k[i] * (ty * c.colsum_y[i]);
    s += k[11] * double(S[1]);
    s += k[12] * double(S[3]);
    s += k[13] * double(S[5]);
    s += k[14] * 0.0;
  }
  return canon_nan(float(s));
}

// one basis row against 11 fp32 coefficients
WORLD_FN float mpc_veh_row(const double* row, const float* c) {
  double s = 0.0;
  for (int j = 0; j < 11; ++j) s += row[j] * double(c[j]);
  return canon_nan(float(s));
}

// track: point k < 100 of the track of coefficients c [11]
WORLD_FN float mpc_veh_track(const double* P, const float* c, int k) { return mpc_veh_row(P + k * 11, c); }

// advance: element e of S' = (x, y, vx, vy, ax, ay) one tick along the plan coef [22]
WORLD_FN float mpc_veh_advance(const double* adv, const float* coef, int e) {
  return mpc_veh_row(adv + (e >> 1) * 11, coef + (e & 1) * 11);
}

}  // namespace mpcmmd
