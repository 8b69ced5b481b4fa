// k_mpc_validate_prep: the inputs of the synthetic closed loop's validation
// stage, one workgroup of 256 threads per episode.  It
// forms on the device what plan_params (validate_api.hip) takes from the host
// after a finished solve, so launch_validate and the k_validate_risk launches
// run on the chained route as mpcmmd_validate / mpcmmd_validate_risk run them:
//   threads 0..21   the plan's cx, cy: the solve's fp32 words widened (exact)
//   thread 64       init_state: x, y rounded to fp32 as k_mpc_step's
//                   mpc_init_state rounds them (a NaN canonical), vx, vy; all
//                   widened; words 4, 5 zero (the validators read 0..3)
//   thread 65       the key tick + key[e]
//   threads 66, 67  the solve's own cost_lane, cost_obs into the tick's log row
//   all threads     the tracks padded to 100 columns (zeros from H on)
// It reads pos and vel, so it runs before the tick's k_mpc_step moves them.
// Conversions and copies only; latency-bound by construction, launched once
// per tick.
#include "common.hpp"
#include "host_constants.hpp"
#include "mpc_step.hpp"
#include "mpc_validate.hpp"

namespace mpcmmd {

namespace {

__global__ __launch_bounds__(kMpcValidateThreads) void k_mpc_validate_prep(const MpcValidateParams q) {
  const int ep = blockIdx.x, tid = threadIdx.x, H = q.H, O = q.O;
  const float* res = q.res + size_t(ep) * q.s_res;

  if (tid < 2 * kNvar) {
    double* dst = tid < kNvar ? q.cx : q.cy;
    dst[size_t(ep) * kNvar + (tid < kNvar ? tid : tid - kNvar)] = double(res[tid]);
  }
  if (tid == 64) {
    double* o = q.init + size_t(ep) * 6;
    o[0] = double(canon_nan(float(q.pos[ep * 2])));
    o[1] = double(canon_nan(float(q.pos[ep * 2 + 1])));
    o[2] = double(q.vel[ep * 3]);
    o[3] = double(q.vel[ep * 3 + 1]);
    o[4] = o[5] = 0.0;
  }
  if (tid == 65) q.keys[ep] = uint32_t(q.tick) + q.key[ep];
  if (tid == 66 || tid == 67) q.est[size_t(ep) * 2 + (tid - 66)] = res[2 * kNvar + (tid - 66)];
  const float* ob = q.obs + size_t(ep) * 2 * O * H;
  float* xo = q.x_obs + size_t(ep) * O * kMpcTrack;
  float* yo = q.y_obs + size_t(ep) * O * kMpcTrack;
  for (int i = tid; i < O * kMpcTrack; i += kMpcValidateThreads) {
    const int o = i / kMpcTrack, h = i - o * kMpcTrack;
    const bool in_h = h < H;
    xo[i] = in_h ? ob[size_t(o) * H + h] : 0.0f;
    yo[i] = in_h ? ob[size_t(O) * H + size_t(o) * H + h] : 0.0f;
  }
}

}  // namespace

void launch_mpc_validate_prep(const MpcValidateParams& q, int episodes, hipStream_t s) {
  hipLaunchKernelGGL(k_mpc_validate_prep, dim3(episodes), dim3(kMpcValidateThreads), 0, s, q);
}

}  // namespace mpcmmd
