// k_world_validate_prep: the inputs of the world context's validation stage
// (DESIGN.md section 20), one workgroup of 256 threads per episode.  It forms
// on the device what carla_plan_params (validate_api.hip) forms on the host
// from a finished solve, so launch_validate_carla and the statistics kernels
// run on the chained route as mpcmmd_validate_carla_risk runs them:
//   1  a thread per plan point: v_best[i] as plan_speed (solve_host.cpp) forms
//      it -- sequential fp64 sums over the 11 columns, each rounded to fp32,
//      then the fp32 norm -- for i <= min(H, 99), into LDS
//   2  a thread per horizon step: plan_controls' acc and steer;
//      thread 64: st0 by carla_velocity_heading's expression (k_tick_setup's);
//      thread 65: the key tick + key[e]; threads 66, 67: the solve's own costs
//      all threads: the path's first P columns, the tracks padded to 100
// Every expression is the host's, operation for operation (-ffp-contract=off),
// so the packed inputs are bit-equal to the host-formed ones.  Latency-bound
// by construction; launched once per tick.
#include "common.hpp"
#include "cr_math.hpp"
#include "host_constants.hpp"
#include "layout.hpp"
#include "world_validate.hpp"

namespace mpcmmd {

namespace {

__global__ __launch_bounds__(kWorldValidateThreads) void k_world_validate_prep(const WorldValidateParams q) {
  const int ep = blockIdx.x, tid = threadIdx.x, H = q.H, O = q.O, P = q.P;
  __shared__ float s_v[kNum];
  const float* res = q.res + size_t(ep) * q.s_res;

  // 1
  const int nv = (H < kNum - 1 ? H : kNum - 1) + 1;  // v[100] = v[99]: the edge is live at H = 100 only
  if (tid < nv) {
    const double* pd = q.pd + tid * kNvar;
    double sx = 0.0, sy = 0.0;
    for (int k = 0; k < kNvar; ++k) {
      sx += pd[k] * double(res[k]);
      sy += pd[k] * double(res[kNvar + k]);
    }
    const float xd = float(sx), yd = float(sy);
    s_v[tid] = sqrtf(xd * xd + yd * yd);
  }
  __syncthreads();

  // 2
  if (tid < H) {
    const float vn = tid + 1 < kNum ? s_v[tid + 1] : s_v[kNum - 1];
    q.acc[size_t(ep) * H + tid] = (vn - s_v[tid]) / 0.15f;
    q.steer[size_t(ep) * H + tid] = q.res_steer[size_t(ep) * q.s_steer + tid];
  }
  if (tid == 64) {
    const float* in = q.in + size_t(ep) * q.s_in;
    float* o = q.st0 + size_t(ep) * 8;
    float s0, c0;
    cr_sincos(in[4], s0, c0);
    const float vx = in[2] * c0, vy = in[2] * s0;
    o[0] = in[0], o[1] = in[1], o[2] = vx, o[3] = vy, o[4] = cr_atan2(vy, vx);
    o[5] = o[6] = o[7] = 0.0f;
  }
  if (tid == 65) q.keys[ep] = uint32_t(q.tick) + q.key[ep];
  if (tid == 66 || tid == 67) q.est[size_t(ep) * 2 + (tid - 66)] = res[2 * kNvar + (tid - 66)];
  {
    const float* pi = q.path_in + size_t(ep) * 6 * kMaxPath;
    float* po = q.path + size_t(ep) * 6 * P;
    for (int i = tid; i < 6 * P; i += kWorldValidateThreads) {
      const int k = i / P, j = i - k * P;
      po[i] = pi[k * kMaxPath + j];
    }
  }
  {
    const float* ob = q.obs + size_t(ep) * 2 * O * H;
    float* xo = q.x_obs + size_t(ep) * O * kNum;
    float* yo = q.y_obs + size_t(ep) * O * kNum;
    for (int i = tid; i < O * kNum; i += kWorldValidateThreads) {
      const int o = i / kNum, h = i - o * kNum;
      const bool in_h = h < H;
      xo[i] = in_h ? ob[size_t(o) * H + h] : 0.0f;
      yo[i] = in_h ? ob[size_t(O) * H + size_t(o) * H + h] : 0.0f;
    }
  }
}

}  // namespace

void launch_world_validate_prep(const WorldValidateParams& q, int episodes, hipStream_t s) {
  hipLaunchKernelGGL(k_world_validate_prep, dim3(episodes), dim3(kWorldValidateThreads), 0, s, q);
}

}  // namespace mpcmmd
