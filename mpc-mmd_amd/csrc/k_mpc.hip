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
// k_mpc_step_planned is the same step with the vehicles following their
// re-planned QP, k_mpc_step_queue and
// k_mpc_step_planned_queue the same two steps with a tick per slot and a mask
// (the scene queue): the body below is written once and
// instantiated four times.
#include "mpc.hpp"
#include "mpc_draw.hpp"

namespace mpcmmd {

namespace {

struct DevMath {
  static DEVI double atan64(double a) { return ::atan(a); }
  static DEVI double tan64(double a) { return ::tan(a); }
  static DEVI void sincos64(double a, double& s, double& c) { ::sincos(a, &s, &c); }
};

// kPlanned: the vehicles follow their re-planned QP (mpc_vehicle.hpp) --
//   a  before phase 1's barrier, from the last thread down (thread 0 has the controller): the
//      O x 22 coefficients of plan(S_k) into s_coef, and the basis rows into s_P
//   b  phase 2, a lane per vehicle: S_k+1 = advance, written back and logged; the clear term
//   c  all threads: the coefficients of plan(S_k+1)
//   d  phase 3's tracks: two 11-term sums per (vehicle, point); consecutive threads share a
//      vehicle (its coefficients broadcast) and read rows of s_P 88 B apart (no bank shared)
// The instantiation without the policy references none of the policy's LDS and is the kernel
// it was: about 1.1 KB of static LDS; with the policy about 17 KB.
// kQueue: the scene queue's step -- the slot's own tick (q.ltick) where the
// step reads q.tick (the drawn variates, done), and with q.fresh a slot that took no scene returns
// at once (the masked reset).  The instantiations without it read neither pointer.
template <bool kPlanned, bool kQueue = false>
DEVI void mpc_step_body(const MpcStepParams& q, const MpcVehParams* pv) {
  const MpcScalars& w = q.w;
  const int ep = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if constexpr (kQueue) {
    if (q.fresh && q.fresh[ep] < 0) return;  // the whole workgroup
  }
  __shared__ MpcEgo s_ego;
  __shared__ MpcControl s_ctl;
  __shared__ float s_u[3];
  __shared__ float s_init[6];
  __shared__ float s_veh[kMpcMaxObs][4];
  __shared__ float s_clear;
  __shared__ double s_P[kMpcTrack * 11];
  __shared__ float s_coef[kMpcMaxObs][kVehCoef];
  __shared__ float s_S[kMpcMaxObs][6];
  __shared__ float s_tgt[kMpcMaxObs][2];

  const bool frozen = q.reset || q.done[ep] >= 0;
  const float* cx = q.cx + size_t(ep) * q.s_plan;
  const float* cy = q.cy + size_t(ep) * q.s_plan;

  if constexpr (kPlanned) {  // a
    const int rows = q.x_obs ? kMpcTrack : q.H;
    for (int i = tid; i < rows * 11; i += kMpcThreads) s_P[i] = pv->k.P[i];
    if (!frozen)
      for (int i = kMpcThreads - 1 - tid; i < w.O * kVehCoef; i += kMpcThreads) {
        const int o = i / kVehCoef, j = i - o * kVehCoef;
        const float* veh = q.veh + (size_t(ep) * w.O + o) * 4;
        const float* acc = pv->acc + (size_t(ep) * w.O + o) * 2;
        const float S[6] = {veh[0], veh[1], veh[2], veh[3], acc[0], acc[1]};
        s_coef[o][j] = mpc_veh_coef(pv->k, S, pv->target + (size_t(ep) * w.O + o) * 2, j);
      }
  }

  // 1
  if (tid == 0) {
    MpcEgo e{q.pos[ep * 2], q.pos[ep * 2 + 1], q.vel[ep * 3], q.vel[ep * 3 + 1], q.vel[ep * 3 + 2]};
    MpcControl c{};
    float u[3] = {0.0f, 0.0f, 0.0f};
    if (!q.reset) {  // a reset runs before any solve: the result buffers hold nothing yet
      c = mpc_controller<DevMath>(q.pdot2, q.pddot1, cx, cy);
      if (q.u) for (int k = 0; k < 3; ++k) u[k] = q.u[ep * 3 + k];
      else mpc_draw(w.noise, q.key[ep], q.seed, kQueue ? q.ltick[ep] : q.tick, c.a_c, c.s_c, u);
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
      if constexpr (kPlanned) {  // b
        const size_t vo = size_t(ep) * w.O + lane;
        float* acc = pv->acc + vo * 2;
        float S[6] = {v[0], v[1], v[2], v[3], acc[0], acc[1]};
        if (!frozen) {
          for (int k = 0; k < 6; ++k) S[k] = mpc_veh_advance(pv->k.adv, s_coef[lane], k);
          for (int k = 0; k < 4; ++k) veh[k] = v[k] = S[k];
          acc[0] = S[4], acc[1] = S[5];
        }
        for (int k = 0; k < 6; ++k) s_S[lane][k] = S[k];
        for (int k = 0; k < 2; ++k) s_tgt[lane][k] = pv->target[vo * 2 + k];
        if (pv->log)
          for (int k = 0; k < 6; ++k) pv->log[vo * 6 + k] = S[k];
      } else {
        if (!frozen) {
          v[0] = v[0] + v[2] * w.dt;
          v[1] = v[1] + v[3] * w.dt;
          veh[0] = v[0], veh[1] = v[1];
        }
        for (int k = 0; k < 4; ++k) s_veh[lane][k] = v[k];
      }
      t = mpc_clear_term(w, e, v);
    }
    const bool any_nan = __ballot(t != t) != 0;
    const float m = wave_max(t != t ? -INFINITY : t);
    if (lane == 0) s_clear = any_nan ? canon_nan(NAN) : m;
  }
  __syncthreads();

  if constexpr (kPlanned) {  // c
    for (int i = tid; i < w.O * kVehCoef; i += kMpcThreads) {
      const int o = i / kVehCoef, j = i - o * kVehCoef;
      s_coef[o][j] = mpc_veh_coef(pv->k, s_S[o], s_tgt[o], j);
    }
    __syncthreads();
  }

  // 3
  if (q.obs) {  // obstacle_transpose's layout: [2][O][H]
    float* ob = q.obs + size_t(ep) * 2 * w.O * q.H;
    for (int i = tid; i < w.O * q.H; i += kMpcThreads) {
      const int o = i / q.H, k = i - o * q.H;
      if constexpr (kPlanned) {  // d
        ob[i] = mpc_veh_track(s_P, s_coef[o], k);
        ob[size_t(w.O) * q.H + i] = mpc_veh_track(s_P, s_coef[o] + 11, k);
      } else {
        ob[i] = mpc_track(s_veh[o][0], s_veh[o][2], k);
        ob[size_t(w.O) * q.H + i] = mpc_track(s_veh[o][1], s_veh[o][3], k);
      }
    }
  }
  if (q.x_obs) {
    float* xo = q.x_obs + size_t(ep) * w.O * kMpcTrack;
    float* yo = q.y_obs + size_t(ep) * w.O * kMpcTrack;
    for (int i = tid; i < w.O * kMpcTrack; i += kMpcThreads) {
      const int o = i / kMpcTrack, k = i - o * kMpcTrack;
      if constexpr (kPlanned) {  // d
        xo[i] = mpc_veh_track(s_P, s_coef[o], k);
        yo[i] = mpc_veh_track(s_P, s_coef[o] + 11, k);
      } else {
        xo[i] = mpc_track(s_veh[o][0], s_veh[o][2], k);
        yo[i] = mpc_track(s_veh[o][1], s_veh[o][3], k);
      }
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
    if (!frozen && (collided || goal)) q.done[ep] = kQueue ? q.ltick[ep] : q.tick;
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

__global__ __launch_bounds__(kMpcThreads) void k_mpc_step(const MpcStepParams q) {
  mpc_step_body<false>(q, nullptr);
}

__global__ __launch_bounds__(kMpcThreads) void k_mpc_step_planned(const MpcStepParams q, const MpcVehParams pv) {
  mpc_step_body<true>(q, &pv);
}

__global__ __launch_bounds__(kMpcThreads) void k_mpc_step_queue(const MpcStepParams q) {
  mpc_step_body<false, true>(q, nullptr);
}

__global__ __launch_bounds__(kMpcThreads) void k_mpc_step_planned_queue(const MpcStepParams q, const MpcVehParams pv) {
  mpc_step_body<true, true>(q, &pv);
}

}  // namespace

void launch_mpc_step(const MpcStepParams& q, int episodes, hipStream_t s) {
  hipLaunchKernelGGL(k_mpc_step, dim3(episodes), dim3(kMpcThreads), 0, s, q);
}

void launch_mpc_step_planned(const MpcStepParams& q, const MpcVehParams& pv, int episodes, hipStream_t s) {
  hipLaunchKernelGGL(k_mpc_step_planned, dim3(episodes), dim3(kMpcThreads), 0, s, q, pv);
}

void launch_mpc_step_queue(const MpcStepParams& q, int episodes, hipStream_t s) {
  hipLaunchKernelGGL(k_mpc_step_queue, dim3(episodes), dim3(kMpcThreads), 0, s, q);
}

void launch_mpc_step_planned_queue(const MpcStepParams& q, const MpcVehParams& pv, int episodes, hipStream_t s) {
  hipLaunchKernelGGL(k_mpc_step_planned_queue, dim3(episodes), dim3(kMpcThreads), 0, s, q, pv);
}

}  // namespace mpcmmd
