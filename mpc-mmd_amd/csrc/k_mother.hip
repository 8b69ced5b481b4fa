// k_mother and k_mmdfinal: the two rollout kernels around the beta-CEM
// (betacem_common.hpp has the pipeline).
#include "betacem_common.hpp"
#include "rng.hpp"
#include "rollout.hpp"

namespace mpcmmd {

namespace {

// CARLA (the fp64 tan / per-row initial states) and the static rollouts as two
// instantiations: the static one's registers no longer carry the CARLA path
// (166 -> fewer VGPRs, SGPR spills gone: two 512-thread workgroups per CU)
constexpr int kMotherWaves = 1;  // waves per SIMD the static instantiation is allocated for (an experiment edits it)
template <bool CARLA>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(CARLA ? 1 : kMotherWaves))) void k_mother(Params p, int t) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int n = p.n, H = p.H, M = p.M, b = blockIdx.x;
  const Cfg cf = cfg_of(p, b / p.B);
  float* an = reinterpret_cast<float*>(smem);
  float* sn = an + n * H;
  float* tn = sn + n * H;  // CARLA: float(tan(double(steer))) of each control, off the rows' step chains
  // the Bernstein fit rows by step, [H][11] doubles: a step's eleven factors as
  // LDS broadcasts, not a scalar-load latency inside every step of the chain
  double* fitl = reinterpret_cast<double*>(smem + ((size_t(3) * n * H * 4 + 15) & ~size_t(15)));
  for (int idx = tidx(); idx < 11 * H; idx += blockDim.x) {
    const int h = idx / 11, k = idx - h * 11;
    fitl[idx] = p.fit[k * H + h];
  }
  float* gctrl = p.ctrl_n + size_t(b) * 2 * n * H;
  for (int idx = tidx(); idx < n * H; idx += blockDim.x) {
    const int r = idx / H, h = idx % H;
    float a, s;
    noisy_control(p, cf, t, r, h, p.acc[size_t(b) * 100 + h], p.steer[size_t(b) * 100 + h], a, s);
    an[idx] = a;
    sn[idx] = s;
    if constexpr (CARLA) tn[idx] = float(tan(double(s)));
    gctrl[idx] = a;
    gctrl[n * H + idx] = s;
  }
  __syncthreads();
  float* F = p.feat + size_t(b) * kF * M;
  for (int m = tidx(); m < M; m += blockDim.x) {
    // jnp.repeat(acc, n, 0) / jnp.tile(steer, (n, 1)) (cem_helper.py:510-511)
    const float* ar = an + (m / n) * H;
    const float* sr = sn + (m % n) * H;
    const float* tr = tn + (m % n) * H;
    // CARLA: every mother row starts from its own noisy initial state
    // (carla/optimizer/cem.py:251-253, cem_helper.py:846)
    const float* st = CARLA ? p.st0r + (size_t(cf.g) * p.R0 + m) * 8 : cf.st0;
    float x = st[0], y = st[1], vx = st[2], vy = st[3], psi = st[4];
    double cx[11], cy[11];
#pragma unroll
    for (int k = 0; k < 11; ++k) cx[k] = cy[k] = 0.0;
    for (int h = 0; h < H; ++h) {
      const double dx = double(x), dy = double(y);
#pragma unroll
      for (int k = 0; k < 11; ++k) {
        const double f = fitl[h * 11 + k];
        cx[k] = cx[k] + f * dx;
        cy[k] = cy[k] + f * dy;
      }
      if (h == H - 1) break;
      if constexpr (CARLA) bicycle_step_cr_t(x, y, vx, vy, psi, ar[h], tr[h], p.wheel_base);
      else bicycle_step(x, y, vx, vy, psi, ar[h], sr[h]);
    }
    float fr[kFeatStride];
#pragma unroll
    for (int k = 0; k < 11; ++k) {
      fr[k] = float(cx[k]);
      fr[11 + k] = float(cy[k]);
      F[k * M + m] = fr[k];
      F[(11 + k) * M + m] = fr[11 + k];
    }
    fr[22] = fr[23] = 0.0f;
    float4* Fr = reinterpret_cast<float4*>(p.featr + (size_t(b) * M + m) * kFeatStride);
#pragma unroll
    for (int q = 0; q < kFeatStride / 4; ++q) Fr[q] = make_float4(fr[4 * q], fr[4 * q + 1], fr[4 * q + 2], fr[4 * q + 3]);
  }
}

// k_mmdfinal: x_red / y_red of the best reduced set (compute_beta.py:465),
// compute_mmd_obs (costs.py:173-186) and compute_mmd_lane (costs.py:121-135).
// Two phases: the n reduced rollouts a lane each, their states kept in LDS,
// then the n H O obstacle terms over all 64 lanes, a (row, step) pair per
// lane, the row maxima by LDS atomics on the bit patterns (every compared
// value is >= +0 after the max with the initial 0, where unsigned order is
// float order; a maximum is order-free, so the bits are the sequential
// loop's).  The sequential form held 22 of 64 lanes through H x O f_bar
// evaluations and their obstacle loads (62 us per configs[1] step).
__global__ __launch_bounds__(64) void k_mmdfinal(Params p, int t) {
  __shared__ float cb[kMaxReduced], lb[kMaxReduced], ub[kMaxReduced], bt[kMaxReduced];
  __shared__ uint32_t cbits[kMaxReduced], cnan[kMaxReduced];
  __shared__ ReduceScratch rs;
  extern __shared__ __attribute__((aligned(16))) float xy[];  // [2][n][H] rollout states, then [2][n][H] controls
  const int b = blockIdx.x, n = p.n, H = p.H, O = p.O, lane = tidx();
  const Cfg cf = cfg_of(p, b / p.B);
  // the candidate's noisy controls staged by all lanes (coalesced), so the
  // rollouts' per-step reads are LDS reads, not a global load latency per step
  float* ctrl = xy + 2 * n * H;
  for (int i = lane; i < 2 * n * H; i += 64) ctrl[i] = p.ctrl_n[size_t(b) * 2 * n * H + i];
  __syncthreads();
  if (lane < n) {
    const int m = p.bestsel[size_t(b) * n + lane];
    const float* ar = ctrl + (m / n) * H;
    const float* sr = ctrl + n * H + (m % n) * H;
    float x = cf.st0[0], y = cf.st0[1], vx = cf.st0[2], vy = cf.st0[3], psi = cf.st0[4];
    float l = 0.0f, u = 0.0f;
    bool nan = false;
    for (int h = 0; h < H; ++h) {
      xy[lane * H + h] = x;
      xy[(n + lane) * H + h] = y;
      nan |= (y != y);
      l = fmaxf(l, -y + p.y_lb);
      u = fmaxf(u, y - p.y_ub);
      if (h == H - 1) break;
      bicycle_step(x, y, vx, vy, psi, ar[h], sr[h]);
    }
    const float qnan = __int_as_float(0x7fc00000);
    cbits[lane] = 0u;
    cnan[lane] = nan ? 1u : 0u;
    lb[lane] = nan ? qnan : l;
    ub[lane] = nan ? qnan : u;
    bt[lane] = p.beta[size_t(b) * n + lane];
  }
  __syncthreads();
  for (int e = lane; e < n * H; e += 64) {
    const int k = e / H, h = e - k * H;
    const float x = xy[e], y = xy[n * H + e];
    float c = 0.0f;
    bool nan = false;
    for (int o = 0; o < O; ++o) {
      const float f = f_bar(x, y, cf.obs[o * H + h], cf.obs[O * H + o * H + h]);
      nan |= (f != f);
      c = fmaxf(c, f);
    }
    atomicMax(&cbits[k], __float_as_uint(c + 0.0f));  // -0 -> +0 (fmaxf may keep -0): unsigned order = float order
    if (nan) atomicOr(&cnan[k], 1u);
  }
  __syncthreads();
  if (lane < n) cb[lane] = cnan[lane] ? __int_as_float(0x7fc00000) : __uint_as_float(cbits[lane]);
  __syncthreads();
  const float sigma = p.sigma[b];
  const float obs = block_mmd(cb, bt, n, sigma, 1000.0f, rs);
  const float ml = block_mmd(lb, bt, n, sigma, 1000.0f, rs);
  const float mu = block_mmd(ub, bt, n, sigma, 1000.0f, rs);
  if (lane == 0) {
    p.obs_cost[b] = obs;
    p.lane_cost[b] = ml + mu;
  }
}

}  // namespace

void launch_mother(const Params& p, int t, hipStream_t s) {
  const size_t lds = ((size_t(3) * p.n * p.H * 4 + 15) & ~size_t(15)) + size_t(11) * p.H * 8;  // controls, fit rows
  if (p.carla)
    hipLaunchKernelGGL(k_mother<true>, dim3(p.Bt), dim3(kThreads), lds, s, p, t);
  else
    hipLaunchKernelGGL(k_mother<false>, dim3(p.Bt), dim3(kThreads), lds, s, p, t);
}

void launch_mmdfinal(const Params& p, int t, hipStream_t s) {
  hipLaunchKernelGGL(k_mmdfinal, dim3(p.Bt), dim3(64), size_t(4) * p.n * p.H * 4, s, p, t);
}

}  // namespace mpcmmd
