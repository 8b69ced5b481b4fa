// k_world_step: one step of the surrogate world, one
// workgroup of 256 threads per episode.  Every expression is world_step.hpp's,
// shared with the host twin (world_host.cpp), so the outputs are bit-equal to
// mpcmmd_world_step_host wherever OCML's fp64 transcendentals round to the
// host libm's values; the kernel only spreads the elements:
//   1  thread 0: controller, the variates (given, or drawn: world_draw.hpp), perturbation, ego step
//   2  wave 0, a lane per vehicle: the vehicles' step and the clear terms,
//      their maximum by a wave reduction (a NaN term makes it the quiet NaN)
//      all threads: the route argmin as a minimum of (distance bits, index)
//      keys, per thread, per wave, then over the four waves
//   3  a thread per waypoint (binary search of the spline piece, fp64 Horner
//      in scipy's order); thread 64: lateral offset, flags, log row, init_state
//      (and st0 for the chained route); threads 128..161: the plan's log
//      wave 0, a lane per vehicle: the not-behind filter, compacted by ballot
//   4  wave 0, a lane per padded candidate: distance keys
//   5  wave 0: the stable rank by (key, position) compares; rank < O writes
//      all threads: the first population, an element per thread
// Latency-bound by construction (a handful of dependent fp64 chains); launched
// once per tick.
//
// The kernel is a template on the vehicle policy (world.hpp).  With
// WorldRoutedParams the vehicles need the ego's route
// point and lateral offset, so phase 2 only stages their (s, d, v) in LDS beside
// the route argmin, and after that barrier wave 0, a lane per vehicle, finds its
// leader by broadcast reads of the staged states (the values before the step),
// advances (s, v), evaluates its pose on the splines and writes its row; one
// more barrier then hands the rows' clear term to thread 64.
#include <type_traits>

#include "cr_math.hpp"
#include "world.hpp"
#include "world_draw.hpp"

namespace mpcmmd {

namespace {

struct DevMath {
  static DEVI float tan(float a) { return cr_tan(a); }
  static DEVI float atan2(float y, float x) { return cr_atan2(y, x); }
  static DEVI void sincos(float a, float& s, float& c) { cr_sincos(a, s, c); }
  static DEVI void sincos64(double a, double& s, double& c) { ::sincos(a, &s, &c); }
  static DEVI double acos64(double a) { return ::acos(a); }
};

template <class Policy>
__global__ __launch_bounds__(kWorldThreads) void k_world_step(const WorldStepParams q, const Policy pol) {
  constexpr bool kRouted = std::is_same<Policy, WorldRoutedParams>::value;
  const WorldScalars& w = q.w;
  const int ep = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  __shared__ WorldEgo s_ego;
  __shared__ WorldControl s_ctl;
  __shared__ float s_u[4];
  __shared__ float s_veh[kWorldMaxObs][5];
  __shared__ float s_clear;
  __shared__ unsigned long long s_key[kWorldThreads / 64];
  __shared__ uint32_t s_idx[kWorldThreads / 64];
  __shared__ int s_src[kWorldMaxObs];
  __shared__ double s_dist[kWorldMaxObs];
  __shared__ int s_kept;
  __shared__ double s_rs[kRouted ? kWorldMaxObs : 1];  // the routed vehicles' states before the step
  __shared__ float s_rd[kRouted ? kWorldMaxObs : 1], s_rv[kRouted ? kWorldMaxObs : 1];

  const bool frozen = q.reset || q.done[ep] >= 0;
  float* veh = q.veh + size_t(ep) * w.total * 5;

  // 1
  if (tid == 0) {
    WorldEgo e{q.pos[ep * 2], q.pos[ep * 2 + 1], q.ego[ep * 3], q.ego[ep * 3 + 1], q.ego[ep * 3 + 2]};
    WorldControl c{};
    float u[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (!q.reset) {  // a reset runs before any solve: the result buffers hold nothing yet
      c = world_controller(w, q.pdot4, q.cx + size_t(ep) * q.s_plan, q.cy + size_t(ep) * q.s_plan,
                           q.steer + size_t(ep) * q.s_steer, e.v);
      if (q.u) for (int k = 0; k < 4; ++k) u[k] = q.u[ep * 4 + k];
      else world_draw(w.noise, q.key[ep], q.seed, q.tick, c.a_c, c.s_c, u);
      world_perturb(w, u, c);
    }
    for (int k = 0; k < 4; ++k) s_u[k] = u[k];
    if (!frozen) {
      e = world_ego_step<DevMath>(e, c.a, c.s, w.dt);
      q.pos[ep * 2] = e.x, q.pos[ep * 2 + 1] = e.y;
      q.ego[ep * 3] = e.v, q.ego[ep * 3 + 1] = e.psi, q.ego[ep * 3 + 2] = e.psidot;
    }
    s_ego = e;
    s_ctl = c;
  }
  __syncthreads();
  const WorldEgo e = s_ego;

  // 2
  if constexpr (kRouted) {
    if (wave == 0 && lane < w.total) {
      const size_t j = size_t(ep) * w.total + lane;
      s_rs[lane] = pol.s[j], s_rd[lane] = pol.param[j * 2], s_rv[lane] = pol.v[j];
    }
  } else if (wave == 0) {
    float t = -INFINITY;
    if (lane < w.total) {
      float v[5];
      for (int k = 0; k < 5; ++k) v[k] = veh[lane * 5 + k];
      if (!frozen) {
        v[0] = v[0] + v[2] * w.dt;
        v[1] = v[1] + v[3] * w.dt;
        veh[lane * 5] = v[0], veh[lane * 5 + 1] = v[1];
      }
      for (int k = 0; k < 5; ++k) s_veh[lane][k] = v[k];
      t = clear_term<DevMath>(w, e, v);
    }
    const bool any_nan = __ballot(t != t) != 0;
    const float m = wave_max(t != t ? -INFINITY : t);
    if (lane == 0) s_clear = any_nan ? canon_nan(NAN) : m;
  }
  unsigned long long best = ~0ull;
  uint32_t bi = ~0u;
  for (int j = tid; j < w.n_route; j += kWorldThreads) {
    const unsigned long long k = route_key(e.x, e.y, q.route_x[j], q.route_y[j]);
    if (k < best) best = k, bi = uint32_t(j);
  }
  {
    const unsigned long long wk = wave_min_u64(best);
    const uint32_t wi = wave_min_u32(best == wk ? bi : ~0u);
    if (lane == 0) s_key[wave] = wk, s_idx[wave] = wi;
  }
  __syncthreads();
  unsigned long long kmin = s_key[0];
  for (int k = 1; k < kWorldThreads / 64; ++k) kmin = s_key[k] < kmin ? s_key[k] : kmin;
  uint32_t uidx = ~0u;
  for (int k = 0; k < kWorldThreads / 64; ++k)
    if (s_key[k] == kmin && s_idx[k] < uidx) uidx = s_idx[k];
  const int idx = int(uidx);  // n_route >= 1: some thread holds a key below ~0
  const double s0 = q.arc[idx];

  if constexpr (kRouted) {  // the vehicles, behind the ego's route point
    if (wave == 0) {
      float t = -INFINITY;
      if (lane < w.total) {
        const size_t j = size_t(ep) * w.total + lane;
        double s = s_rs[lane];
        float v = s_rv[lane], a = 0.0f;
        if (!frozen) {
          const float d_ego = world_lateral(w, q.route_x, q.route_y, q.arc, q.sx, q.sy, idx, e);
          const VehLeader l = vehicle_leader(pol.p, lane, w.total, s_rs, s_rd, 1, s_rv, s0, d_ego, e.v);
          vehicle_advance(pol.p, w.dt, pol.param[j * 2 + 1], l, &s, &v, &a);
          pol.s[j] = s, pol.v[j] = v;
        }
        if (!q.reset) {
          if (pol.log) pol.log[j * 2] = v, pol.log[j * 2 + 1] = a;
          if (pol.log_s) pol.log_s[j] = s;
        }
        float row[5];
        vehicle_pose<DevMath>(q.arc, q.sx, q.sy, w.n_route, s, s_rd[lane], v, row);
        for (int k = 0; k < 5; ++k) veh[lane * 5 + k] = row[k], s_veh[lane][k] = row[k];
        t = clear_term<DevMath>(w, e, row);
      }
      const bool any_nan = __ballot(t != t) != 0;
      const float m = wave_max(t != t ? -INFINITY : t);
      if (lane == 0) s_clear = any_nan ? canon_nan(NAN) : m;
    }
  }

  // 3
  for (int i = tid; i < w.P; i += kWorldThreads)
    world_waypoint(w, q.arc, q.sx, q.sy, s0, e, i, q.xw + size_t(ep) * q.s_wp + i, q.yw + size_t(ep) * q.s_wp + i);
  if (tid == 64) {
    float* in = q.init + size_t(ep) * q.s_init;
    in[0] = 0.0f, in[1] = 0.0f, in[2] = e.v, in[3] = 0.0f, in[4] = e.psi, in[5] = e.psidot;
    if (q.st0) {  // initial_state (solve_host.cpp) of that init_state
      float* s0r = q.st0 + size_t(ep) * 8;
      s0r[0] = 0.0f, s0r[1] = 0.0f, s0r[2] = e.v, s0r[3] = 0.0f, s0r[4] = atan2f(0.0f, e.v);
      s0r[5] = s0r[6] = s0r[7] = 0.0f;
    }
  }
  if constexpr (kRouted) __syncthreads();  // s_clear of the rows just written
  if (tid == 64 && !q.reset) {
    const WorldControl c = s_ctl;
    const float clear = s_clear;
    const float d = world_lateral(w, q.route_x, q.route_y, q.arc, q.sx, q.sy, idx, e);
    const bool lane_out = d < w.y_lb || d > w.y_ub;
    const bool collided = !(clear <= 0.0f);
    const bool goal = world_goal(w, q.route_x, q.route_y, e);
    if (!frozen && (collided || goal)) q.done[ep] = q.tick;
    double* ld = q.logd + size_t(ep) * 3;
    ld[0] = e.x, ld[1] = e.y, ld[2] = s0;
    float* lf = q.logf + size_t(ep) * 13;
    const float* u = s_u;
    lf[0] = e.v, lf[1] = e.psi, lf[2] = e.psidot, lf[3] = c.a_c, lf[4] = c.s_c, lf[5] = c.a, lf[6] = c.s;
    lf[7] = u[0], lf[8] = u[1], lf[9] = u[2], lf[10] = u[3], lf[11] = clear, lf[12] = d;
    int32_t* li = q.logi + size_t(ep) * 4;
    li[0] = idx, li[1] = lane_out, li[2] = collided, li[3] = goal;
  }
  if (q.plan && !q.reset && tid >= 128 && tid < 128 + 34) {  // the plan this step consumed
    const int i = tid - 128;
    const float v = i < 11 ? q.cx[size_t(ep) * q.s_plan + i]
                  : i < 22 ? q.cy[size_t(ep) * q.s_plan + i - 11]
                  : i < 26 ? q.steer[size_t(ep) * q.s_steer + i - 22] : q.mean[ep * 8 + i - 26];
    q.plan[size_t(ep) * 34 + i] = v;
  }
  if (wave == 0) {
    const bool kept = lane < w.total && obstacle_kept<DevMath>(e, s_veh[lane]);  // s_veh[lane]: this lane's own write
    const unsigned long long mask = __ballot(kept);
    if (kept) s_src[__popcll(mask & ((1ull << lane) - 1ull))] = lane;
    if (lane == 0) s_kept = __popcll(mask);
  }
  __syncthreads();

  // 4
  const int K = s_kept, Lp = K > w.O ? K : w.O;  // <= 64: total <= 64 and O <= 64
  float row[5] = {300.0f, 300.0f, 0.0f, 0.0f, 0.0f};  // none kept: every candidate 300 m away
  double key = 0.0;
  if (wave == 0 && lane < Lp) {
    if (K > 0) {
      const int src = s_src[lane < K ? lane : K - 1];  // padded by the last kept vehicle
      for (int k = 0; k < 5; ++k) row[k] = s_veh[src][k];
    }
    key = obstacle_dist2(e, row[0], row[1]);
    s_dist[lane] = key;
  }
  __syncthreads();

  // 5
  if (wave == 0 && lane < Lp) {
    int rank = 0;
    for (int i = 0; i < Lp; ++i) rank += dist_before(s_dist[i], i, key, lane) ? 1 : 0;
    if (rank < w.O) {
      float* out = q.obs + size_t(ep) * q.s_obs + rank * 5;
      out[0] = obstacle_shift(row[0], e.x), out[1] = obstacle_shift(row[1], e.y);
      out[2] = row[2], out[3] = row[3], out[4] = row[4];
    }
  }
  const float* mean = q.mean + ep * 8;
  for (int i = tid; i < w.B * 8; i += kWorldThreads)
    q.pop[size_t(ep) * w.B * 8 + i] = world_pop(mean, q.chol, q.pop0 + size_t(i >> 3) * 8, i & 7);
}

}  // namespace

void launch_world_step(const WorldStepParams& q, int episodes, hipStream_t s) {
  hipLaunchKernelGGL(k_world_step<WorldConstantVelocity>, dim3(episodes), dim3(kWorldThreads), 0, s, q,
                     WorldConstantVelocity{});
}

void launch_world_step_routed(const WorldStepParams& q, const WorldRoutedParams& r, int episodes, hipStream_t s) {
  hipLaunchKernelGGL(k_world_step<WorldRoutedParams>, dim3(episodes), dim3(kWorldThreads), 0, s, q, r);
}

}  // namespace mpcmmd
