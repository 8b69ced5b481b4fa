// Monte-Carlo validation of saved optima: S/validation.py
// compute_stats (:134-171) for a batch of configurations on the GPU.
//
// One workgroup per configuration.  Threads 0..99 first evaluate the saved
// trajectory's derivatives (xdot = Pdot cx, ... with the fp32 basis, fp64
// sums: validation.py:140-141) and its controls (compute_controls,
// :122-132); then every thread runs noisy rollouts (compute_rollout_complete,
// :42-101) in fp64, the arithmetic NumPy does there, and counts per
// (obstacle, step) and per step the rollouts inside an obstacle ellipse
// (compute_f_bar_temp :103-110, count_nonzero) or across a lane bound
// (compute_lane_bar :112-120).  The counts are integer LDS atomics, so the
// result does not depend on the thread order.  The controls, the noise draw
// and the bicycle step are validate_step.hpp's, shared with k_validate_risk.hip.
#include <hip/hip_runtime.h>

#include "common.hpp"
#include "kernels.hpp"
#include "rng.hpp"
#include "validate_step.hpp"

namespace mpcmmd {
namespace {

__global__ __launch_bounds__(kValThreads) void k_validate(ValidateParams v) {
  __shared__ double sacc[kValMaxH], ssteer[kValMaxH], sv[kValMaxH];
  __shared__ float sxo[kValMaxObs * kValMaxH], syo[kValMaxObs * kValMaxH];
  __shared__ int cnt[kValMaxObs * kValMaxH], clb[kValMaxH], cub[kValMaxH];
  const int k = blockIdx.x, tid = threadIdx.x;
  const int H = v.H, O = v.O, R = v.R;
  const ValNoise vn{v.noise, v.noise_level, v.acc_const, v.steer_const, v.K_steer};
  const double* cx = v.cx + size_t(k) * 11;
  const double* cy = v.cy + size_t(k) * 11;
  for (int i = tid; i < O * H; i += kValThreads) {
    const int o = i / H, h = i - o * H;
    sxo[i] = v.x_obs[(size_t(k) * O + o) * 100 + h];
    syo[i] = v.y_obs[(size_t(k) * O + o) * 100 + h];
    cnt[i] = 0;
  }
  if (tid < H) clb[tid] = cub[tid] = 0;
  val_controls(v.Pdot, v.Pddot, cx, cy, H, tid, sv, sacc, ssteer);
  const double* st = v.init_state + size_t(k) * 6;
  const uint32_t k0 = v.keys[k], k1 = v.seed;
  const double* dr = v.draws ? v.draws + size_t(k) * 3 * R * H : nullptr;
  for (int r = tid; r < R; r += kValThreads) {
    double x = st[0], y = st[1], vx = st[2], vy = st[3], psi = atan2(st[3], st[2]);  // :147
    for (int h = 0; h < H; ++h) {
      // x_roll[:, h] = state before step h (:94-99)
      for (int o = 0; o < O; ++o) {
        const double wc = x - double(sxo[o * H + h]), ws = y - double(syo[o * H + h]);
        const double c = -(wc * wc) / 18.0625 - (ws * ws) / 7.5625 + 1.0;  // :106-109
        if (!(c <= 0.0)) atomicAdd(&cnt[o * H + h], 1);                     // count_nonzero(max(0, c))
      }
      if (!(-y + v.y_lb <= 0.0)) atomicAdd(&clb[h], 1);  // :116-119
      if (!(y - v.y_ub <= 0.0)) atomicAdd(&cub[h], 1);
      if (h == H - 1) break;
      double an, sn;
      val_noisy_controls(vn, dr, R, H, r, h, k0, k1, sacc[h], ssteer[h], an, sn);
      val_bicycle_step(an, sn, x, y, vx, vy, psi);
    }
  }
  __syncthreads();
  // count = max_o max_t #(rollouts in collision); lane = max_t #lb + max_t #ub (:153-169)
  if (tid < 64) {
    int m = 0, mlb = 0, mub = 0;
    for (int i = tid; i < O * H; i += 64) m = max(m, cnt[i]);
    for (int i = tid; i < H; i += 64) {
      mlb = max(mlb, clb[i]);
      mub = max(mub, cub[i]);
    }
    for (int o = 32; o > 0; o >>= 1) {
      m = max(m, __shfl_xor(m, o, 64));
      mlb = max(mlb, __shfl_xor(mlb, o, 64));
      mub = max(mub, __shfl_xor(mub, o, 64));
    }
    if (tid == 0) {
      v.count[k] = m;
      v.count_lane[k] = mlb + mub;
    }
  }
}

}  // namespace

bool validate_shape_ok(int O, int H) { return O >= 1 && O <= kValMaxObs && H >= 2 && H <= kValMaxH; }

void launch_validate(const ValidateParams& v, hipStream_t s) {
  hipLaunchKernelGGL(k_validate, dim3(v.K), dim3(kValThreads), 0, s, v);
}

}  // namespace mpcmmd
