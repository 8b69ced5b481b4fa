// k_mpc_step: one step of the synthetic closed loop, one
// workgroup of 256 threads per episode.  Every expression is mpc_step.hpp's,
// shared with the host twin (mpc_host.cpp), so the outputs are bit-equal to
// mpcmmd_mpc_step_host wherever OCML's fp64 transcendentals round to the host
// libm's values; the kernel only spreads the elements:
//   1  thread 0: controller, the variates (given, or drawn: mpc_draw.hpp),
//      perturbation, ego step, the next init_state
//   2  wave 0, a lane per vehicle: the vehicles' step and the clear terms,
//      their maximum by a wave reduction (a NaN term makes it the quiet NaN)
//   3  all threads: the tracks, an element per thread, into obs (the chained
//      route: the first H points) or x_obs / y_obs (the harness: all 100);
//      threads 0..43: solve_c; thread 64: flags, log row, init_state, st0;
//      threads 128..157: the plan's log; all threads: the first population
// Static LDS only (about 1.1 KB).  Latency-bound by construction (a handful of
// dependent fp64 chains); launched once per tick.
#include "mpc.hpp"
#include "mpc_draw.hpp"

namespace mpcmmd {

namespace {

struct DevMath {
  static DEVI double atan64(double a) { return ::atan(a); }
  static DEVI double tan64(double a) { return ::tan(a); }
  static DEVI void sincos64(double a, double& s, double& c) { ::sincos(a, &s, &c); }
};

__global__ __launch_bounds__(kMpcThreads) void k_mpc_step(const MpcStepParams q) {
  const MpcScalars& w = q.w;
  const int ep = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  __shared__ MpcEgo s_ego;
  __shared__ MpcControl s_ctl;
  __shared__ float s_u[3];
  __shared__ float s_init[6];
  __shared__ float s_veh[kMpcMaxObs][4];
  __shared__ float s_clear;

  const bool frozen = q.reset || q.done[ep] >= 0;
  const float* cx = q.cx + size_t(ep) * q.s_plan;
  const float* cy = q.cy + size_t(ep) * q.s_plan;

  // 1
  if (tid == 0) {
    MpcEgo e{q.pos[ep * 2], q.pos[ep * 2 + 1], q.vel[ep * 3], q.vel[ep * 3 + 1], q.vel[ep * 3 + 2]};
    MpcControl c{};
    float u[3] = {0.0f, 0.0f, 0.0f};
    if (!q.reset) {  // a reset runs before any solve: the result buffers hold nothing yet
      c = mpc_controller<DevMath>(q.pdot2, q.pddot1, cx, cy);
      if (q.u) for (int k = 0; k < 3; ++k) u[k] = q.u[ep * 3 + k];
      else mpc_draw(w.noise, q.key[ep], q.seed, q.tick, c.a_c, c.s_c, u);
      mpc_perturb(w, u, c);
    }
    for (int k = 0; k < 3; ++k) s_u[k] = u[k];
    float ax = 0.0f, ay = 0.0f;  // a frozen state has no acceleration
    if (!frozen) {
      e = mpc_ego_step<DevMath>(e, c.a, c.s, w.dt, &ax, &ay);
      q.pos[ep * 2] = e.x, q.pos[ep * 2 + 1] = e.y;
      q.vel[ep * 3] = e.vx, q.vel[ep * 3 + 1] = e.vy, q.vel[ep * 3 + 2] = e.psi;
    }
    mpc_init_state(e, ax, ay, s_init);
    s_ego = e;
    s_ctl = c;
  }
  __syncthreads();
  const MpcEgo e = s_ego;

  // 2
  if (wave == 0) {
    float t = -INFINITY;
    if (lane < w.O) {
      float* veh = q.veh + (size_t(ep) * w.O + lane) * 4;
      float v[4];
      for (int k = 0; k < 4; ++k) v[k] = veh[k];
      if (!frozen) {
        v[0] = v[0] + v[2] * w.dt;
        v[1] = v[1] + v[3] * w.dt;
        veh[0] = v[0], veh[1] = v[1];
      }
      for (int k = 0; k < 4; ++k) s_veh[lane][k] = v[k];
      t = mpc_clear_term(w, e, v);
    }
    const bool any_nan = __ballot(t != t) != 0;
    const float m = wave_max(t != t ? -INFINITY : t);
    if (lane == 0) s_clear = any_nan ? canon_nan(NAN) : m;
  }
  __syncthreads();

  // 3
  if (q.obs) {  // obstacle_transpose's layout: [2][O][H]
    float* ob = q.obs + size_t(ep) * 2 * w.O * q.H;
    for (int i = tid; i < w.O * q.H; i += kMpcThreads) {
      const int o = i / q.H, k = i - o * q.H;
      ob[i] = mpc_track(s_veh[o][0], s_veh[o][2], k);
      ob[size_t(w.O) * q.H + i] = mpc_track(s_veh[o][1], s_veh[o][3], k);
    }
  }
  if (q.x_obs) {
    float* xo = q.x_obs + size_t(ep) * w.O * kMpcTrack;
    float* yo = q.y_obs + size_t(ep) * w.O * kMpcTrack;
    for (int i = tid; i < w.O * kMpcTrack; i += kMpcThreads) {
      const int o = i / kMpcTrack, k = i - o * kMpcTrack;
      xo[i] = mpc_track(s_veh[o][0], s_veh[o][2], k);
      yo[i] = mpc_track(s_veh[o][1], s_veh[o][3], k);
    }
  }
  if (q.kcol && tid < 44) q.solve_c[size_t(ep) * 44 + tid] = mpc_solve_column(q.kcol, s_init, tid);
  if (tid == 64) {
    if (q.init)
      for (int k = 0; k < 6; ++k) q.init[size_t(ep) * 6 + k] = s_init[k];
    mpc_st0(s_init, q.st0 + size_t(ep) * 8);
  }
  if (tid == 64 && !q.reset) {
    const MpcControl c = s_ctl;
    const float clear = s_clear;
    const bool lane_out = mpc_lane_out(w, e), collided = !(clear <= 0.0f), goal = mpc_goal(w, e);
    if (!frozen && (collided || goal)) q.done[ep] = q.tick;
    double* ld = q.logd + size_t(ep) * 2;
    ld[0] = e.x, ld[1] = e.y;
    float* lf = q.logf + size_t(ep) * 12;
    lf[0] = e.vx, lf[1] = e.vy, lf[2] = e.psi, lf[3] = c.a_c, lf[4] = c.s_c, lf[5] = c.a, lf[6] = c.s;
    lf[7] = s_u[0], lf[8] = s_u[1], lf[9] = s_u[2], lf[10] = clear, lf[11] = c.curv;
    int32_t* li = q.logi + size_t(ep) * 4;
    li[0] = lane_out, li[1] = collided, li[2] = goal, li[3] = frozen;
  }
  const float* mean = q.mean + ep * 8;
  if (q.plan && !q.reset && tid >= 128 && tid < 128 + 30) {  // the plan this step consumed
    const int i = tid - 128;
    q.plan[size_t(ep) * 30 + i] = i < 11 ? cx[i] : i < 22 ? cy[i - 11] : mean[i - 22];
  }
  for (int i = tid; i < w.B * 8; i += kMpcThreads)
    q.pop[size_t(ep) * w.B * 8 + i] = world_pop(mean, q.chol, q.pop0 + size_t(i >> 3) * 8, i & 7);
}

}  // namespace

void launch_mpc_step(const MpcStepParams& q, int episodes, hipStream_t s) {
  hipLaunchKernelGGL(k_mpc_step, dim3(episodes), dim3(kMpcThreads), 0, s, q);
}

}  // namespace mpcmmd
