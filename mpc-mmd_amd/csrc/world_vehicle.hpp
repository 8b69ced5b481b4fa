// The routed vehicles of the surrogate world, written
// once for the host twin (world_host.cpp, g++) and the routed instantiation of
// k_world_step (k_world.hip).  A routed vehicle follows the route's splines at a
// constant signed lateral offset d (left positive, world_lateral's convention)
// and holds the state (s, v): fp64 arc length and fp32 speed.  Its acceleration
// is the intelligent-driver car-following model towards its own target speed v0,
// behind the nearest vehicle or ego ahead of it on its lane.  Every expression is
// fp64 in the order written and rounded to fp32 once where it says so; fp64
// sqrt and division are correctly rounded on both sides, the only
// transcendentals are the Math policy's atan2 and sincos of the pose.  No HIP
// header: plain C++ like world_step.hpp.
#pragma once
#include "world_step.hpp"

namespace mpcmmd {

// the policy's scalars (mpcmmd_world_routed without its arrays)
struct VehScalars {
  float acc_max, brake, gap0, headway, length, lane_tol, gap_min, acc_min;
};

constexpr uint64_t kQuietNaN64 = 0x7FF8000000000000ull;
WORLD_FN double canon_nan64(double x) { return x != x ? __builtin_bit_cast(double, kQuietNaN64) : x; }

struct VehLeader {
  bool has;
  double gap;  // (s_lead - s) - length
  float v;     // the leader's speed
};

// candidate (sk, dk, vk) against vehicle (sj, dj): the nearer of `best` and it.  A strict
// comparison: on equal gaps the candidate seen first stays.  A NaN s or d fails a test.
WORLD_FN void leader_candidate(const VehScalars& p, double sj, float dj, double sk, float dk, float vk, VehLeader& best) {
  const double off = double(dk) - double(dj);
  if (!((off < 0.0 ? -off : off) < double(p.lane_tol))) return;
  if (!(sk > sj)) return;
  const double gap = (sk - sj) - double(p.length);
  if (!best.has || gap < best.gap) best.has = true, best.gap = gap, best.v = vk;
}

// the leader of vehicle j among the vehicles (s, d, v: the values before the step; d at
// stride d_stride) in index order, then the ego (after its move)
WORLD_FN VehLeader vehicle_leader(const VehScalars& p, int j, int n, const double* s, const float* d, int d_stride,
                                  const float* v, double ego_s, float ego_d, float ego_v) {
  VehLeader best{false, 0.0, 0.0f};
  for (int k = 0; k < n; ++k)
    if (k != j) leader_candidate(p, s[j], d[j * d_stride], s[k], d[k * d_stride], v[k], best);
  leader_candidate(p, s[j], d[j * d_stride], ego_s, ego_d, ego_v, best);
  return best;
}

// the intelligent-driver model's acceleration, clipped to [acc_min, acc_max]; a NaN stays NaN
WORLD_FN float vehicle_accel(const VehScalars& p, float v, float v0, const VehLeader& l) {
  const double r = double(v) / double(v0);
  const double free = 1.0 - (r * r) * (r * r);
  double inter = 0.0;
  if (l.has) {
    const double t = double(v) * double(p.headway) +
                     double(v) * (double(v) - double(l.v)) / (2.0 * sqrt(double(p.acc_max) * double(p.brake)));
    const double ss = double(p.gap0) + (t > 0.0 ? t : 0.0);
    const double g = l.gap > double(p.gap_min) ? l.gap : double(p.gap_min);
    inter = (ss / g) * (ss / g);
  }
  double a = double(p.acc_max) * (free - inter);
  a = a < double(p.acc_min) ? double(p.acc_min) : a;
  a = a > double(p.acc_max) ? double(p.acc_max) : a;
  return canon_nan(float(a));
}

// one step of (s, v) under the acceleration of `l`; !(v0 > 0): parked.  *a: the acceleration applied
WORLD_FN void vehicle_advance(const VehScalars& p, float dt, float v0, const VehLeader& l, double* s, float* v,
                              float* a) {
  if (!(v0 > 0.0f)) {
    *v = 0.0f, *a = 0.0f;
    return;
  }
  *a = vehicle_accel(p, *v, v0, l);
  const float vn = *v + *a * dt;
  *v = canon_nan(vn < 0.0f ? 0.0f : vn);
  *s = canon_nan64(*s + double(*v * dt));
}

// the row (x, y, vx, vy, psi) of a vehicle at (s, d) with speed v; past the route's ends the
// first / last spline piece extrapolates, as for the waypoints
template <class M>
WORLD_FN void vehicle_pose(const double* arc, const double* sx, const double* sy, int n, double s, float d, float v,
                           float* row) {
  const int p = spline_piece(arc, n, s);
  const double h = s - arc[p];
  const double X = spline_eval(sx, n, p, h), Y = spline_eval(sy, n, p, h);
  const double tx = spline_slope(sx, n, p, h), ty = spline_slope(sy, n, p, h);
  const double nrm = sqrt(tx * tx + ty * ty);
  const double ux = tx / nrm, uy = ty / nrm;
  row[0] = canon_nan(float(X + double(d) * (-uy)));
  row[1] = canon_nan(float(Y + double(d) * ux));
  const float psi = canon_nan(M::atan2(float(uy), float(ux)));
  float sn, cs;
  M::sincos(psi, sn, cs);
  row[2] = canon_nan(v * cs);
  row[3] = canon_nan(v * sn);
  row[4] = psi;
}

}  // namespace mpcmmd
