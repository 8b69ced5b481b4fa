// Monte-Carlo validation of CARLA plans: the cvar risk stage of the CARLA
// optimizer (k_carla.hip: k_roll_carla mode 0 -> k_frenet -> the bars of
// k_risk_carla) evaluated with R fresh noise rows per simulator tick and
// reduced to collision counts (S/validation.py:153-169) instead of CVaR.
//
// One launch covers every tick: grid (row blocks, ticks), 64 noise rows and
// 512 threads (256 with the internal streams) per workgroup.  The rollout points never leave the workgroup:
//
//   stage    the tick's path (float2 xy padded to 4 frenet_quarter(P), arc,
//            Fx_dot, Fy_dot: k_frenet's layout), the O x H obstacle tracks and
//            the plan's acc / steer [H] into LDS
//   phase A  all lanes form the rows' (H - 1) noisy controls and tan(steer_n)
//            into an [h][row] table (the fp64 tan off the step chain, as
//            k_roll_carla), then one lane per row runs its chain.  The chain
//            stores the recorded point (x, y) of step h over the table's slot
//            h: slot h is read before it is written and never read again by
//            the chain, so the points alias the controls
//   phase B  a quad of lanes per point: frenet_point_quad over the LDS path,
//            then the collision bar against every obstacle and the lane bars;
//            hits go to integer LDS atomics and a per-row flag
//   epilogue the workgroup's counts are added to the tick's global integer
//            counters (order-independent); k_validate_carla_max takes the maxima
//
// The cost variant (k_validate_carla_costs, mpcmmd_validate_carla_risk) is the
// same body with kCosts set: phase B also keeps, per row, the maximum of each
// of the three cost terms (obs, lane_lb, lane_ub) as an ordered 32-bit key in
// an LDS table [3][64] (integer atomicMax: order-independent), and the epilogue
// stores costs[k][c][r0 + row].  The count kernels compile none of it.
//
// The table's row stride is 65 words: phase A writes it with h fastest across
// lanes (coalesced reads of the [R][H] draws), the chain reads it with the row
// fastest, phase B with h fastest again -- all conflict-free at an odd stride.
#include "frenet.hpp"
#include "kernels.hpp"
#include "rng.hpp"
#include "rollout.hpp"

namespace mpcmmd {
namespace {

// Threads per workgroup (DESIGN.md section 11 has the measurements).  With given draws the kernel needs 67
// VGPRs, and 3 workgroups of 8 waves per CU (the LDS bound at the reference shape) hide the path scan's LDS
// latency better than 3 of 4 waves.  The samplers of the internal streams need 158 (normals) / 187 (Beta)
// VGPRs: 8-wave workgroups would leave one per CU.
constexpr int kVcThreadsGiven = 512;
constexpr int kVcThreadsDrawn = 256;
constexpr int kVcRows = 64;  // one wave runs the chains and counts the row flags
constexpr int kVcStride = kVcRows + 1;
constexpr int kVcMaxObs = 32;

// LDS words: path | obstacle tracks | acc, steer | table (controls, then points) | counters | row flags
// | the cost variant's row maxima [3][kVcRows]
HDI size_t vc_lds_words(int O, int H, int P, bool costs = false) {
  return size_t(8) * frenet_quarter(P) + size_t(3) * P + size_t(2) * O * H + size_t(2) * H +
         size_t(2) * H * kVcStride + size_t(O) * H + size_t(2) * H + kVcRows + (costs ? 3 * kVcRows : 0);
}

// The value rule of a cost term max(0, t) as a key that orders as an unsigned integer: t > 0 -> its bits
// (positive floats and +inf ascend), NaN -> the canonical quiet NaN (above +inf), else +0.  The maximum of
// the keys is the bits of jnp.max(jnp.maximum(0, t)): NaN if any term is NaN.
DEVI uint32_t vc_cost_key(float t) {
  return t > 0.0f ? __float_as_uint(t) : (t != t ? 0x7fc00000u : 0u);
}

// standard normal e of stream (k0, k1, stream), rounded as oracle/rng.py philox_normals
DEVI float vc_normal(uint32_t k0, uint32_t k1, uint32_t stream, uint32_t e) {
  return float(philox_normal(k0, k1, stream, e));
}

// Beta(2|u|, 5|u|) of control u with the CARLA combine (beta_combine_cr), as
// the optimizer's CARLA Beta noise (rollout.hpp: beta_pair)
DEVI float vc_beta(float u, uint32_t k0, uint32_t k1, uint32_t sa, uint32_t sb, uint32_t elem) {
  const float fu = fabsf(u);
  const double a = double(2.0f * fu), b = double(5.0f * fu);
  double ga, ua, gb, ub;
  gamma_direct(a, k0, k1, sa, elem, ga, ua);
  gamma_direct(b, k0, k1, sb, elem, gb, ub);
  return beta_combine_cr(a, b, 2.0, 5.0, ga, ua, gb, ub);
}

// kDraws: 0 = the draws are given, 1 = internal normals (gaussian), 2 = internal Beta variates.  Three
// instantiations, because the fp64 samplers of the internal streams would set the register count (and with
// it the waves per SIMD of the Frenet search, the dominant phase) of the kernel that reads given draws too.
// kCosts: the body of the cost variant (the head comment); false compiles the count kernel as it was.  The
// block is taken by value, as a kernel takes it: by reference the count kernels allocate their registers
// differently (one SGPR spill fewer in the compiler's remarks), and they are to stay what they were.
template <int kDraws, int kVcThreads, bool kCosts>
DEVI void vc_body(const ValidateCarlaParams v) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int P = v.P, H = v.H, O = v.O, R = v.R, k = blockIdx.y, tid = threadIdx.x, Pq = frenet_quarter(P);
  const int r0 = blockIdx.x * kVcRows, rows = min(kVcRows, R - r0);
  float2* pxy = reinterpret_cast<float2*>(smem);
  float* arc = reinterpret_cast<float*>(pxy + 4 * Pq);
  float* Fxd = arc + P;
  float* Fyd = Fxd + P;
  float* xo = Fyd + P;  // [O][H]
  float* yo = xo + O * H;
  float* acc = yo + O * H;  // [H]
  float* steer = acc + H;
  float* ta = steer + H;  // [H][kVcStride]: acc_n, then x
  float* tt = ta + H * kVcStride;  // tan(steer_n), then y
  int* cnt = reinterpret_cast<int*>(tt + H * kVcStride);  // [O][H]
  int* clb = cnt + O * H;  // [H]
  int* cub = clb + H;
  int* flag = cub + H;  // [kVcRows]
  uint32_t* cmax = reinterpret_cast<uint32_t*>(flag + kVcRows);  // [3][kVcRows] cost keys (kCosts only)

  const float* pa = v.path + size_t(k) * 6 * P;
  const float inf = __int_as_float(0x7f800000);
  for (int j = tid; j < 4 * Pq; j += kVcThreads) {
    pxy[j] = j < P ? make_float2(pa[j], pa[P + j]) : make_float2(inf, inf);
    if (j < P) {
      arc[j] = pa[2 * P + j];
      Fxd[j] = pa[3 * P + j];
      Fyd[j] = pa[4 * P + j];
    }
  }
  for (int i = tid; i < O * H; i += kVcThreads) {
    const int o = i / H, h = i - o * H;
    xo[i] = v.x_obs[(size_t(k) * O + o) * 100 + h];
    yo[i] = v.y_obs[(size_t(k) * O + o) * 100 + h];
    cnt[i] = 0;
  }
  for (int h = tid; h < H; h += kVcThreads) {
    acc[h] = v.acc[size_t(k) * H + h];
    steer[h] = v.steer[size_t(k) * H + h];
    clb[h] = cub[h] = 0;
  }
  if (tid < kVcRows) flag[tid] = 0;
  if constexpr (kCosts)
    if (tid < 3 * kVcRows) cmax[tid] = 0u;
  __syncthreads();

  // phase A: noisy controls (helper.inject_noise; rollout.hpp: noisy_from) and tan(steer_n)
  const uint32_t k0 = v.keys[k], k1 = v.seed;
  const size_t RH = size_t(R) * H;
  const float* dr = v.draws ? v.draws + size_t(k) * 3 * RH : nullptr;
  const int Hc = H - 1;
  for (int e = tid; e < rows * Hc; e += kVcThreads) {
    const int rr = e / Hc, h = e - rr * Hc, r = r0 + rr;
    const float a = acc[h], s = steer[h];
    float n0, n1, n2;
    if constexpr (kDraws == 0) {
      const size_t at = size_t(r) * H + h;
      n0 = dr[at];
      n1 = dr[RH + at];
      n2 = dr[2 * RH + at];
    } else {
      const uint32_t el = uint32_t(r) * uint32_t(H) + uint32_t(h);
      n2 = vc_normal(k0, k1, kStreamVcConst, el);
      if constexpr (kDraws == 1) {
        n0 = vc_normal(k0, k1, kStreamVcAcc, el);
        n1 = vc_normal(k0, k1, kStreamVcSteer, el);
      } else {
        n0 = vc_beta(a, k0, k1, kStreamVcGammaAccA, kStreamVcGammaAccB, el);
        n1 = vc_beta(s, k0, k1, kStreamVcGammaSteerA, kStreamVcGammaSteerB, el);
      }
    }
    float an, sn;
    noisy_from(v, a, s, n0, n1, n2, an, sn);
    ta[h * kVcStride + rr] = an;
    tt[h * kVcStride + rr] = float(tan(double(sn)));
  }
  __syncthreads();
  if (tid < rows) {  // the row's chain from its noisy initial state (CarlaCEM.noisy_init)
    const int r = r0 + tid;
    float ex, ey;
    if (v.init_eps) {
      const float* ep = v.init_eps + (size_t(k) * R + r) * 4;
      ex = ep[0];
      ey = ep[1];
    } else {  // elements 4 r, 4 r + 1: block r of the stream
      double z[4];
      philox_normals4(k0, k1, kStreamVcInitEps, 0u, uint32_t(r), z);
      ex = float(z[0]);
      ey = float(z[1]);
    }
    const float* st = v.st0 + size_t(k) * 8;
    float x = st[0] + (ex * v.init_sigma_x + v.init_mu_x);
    float y = st[1] + (ey * v.init_sigma_y + v.init_mu_y);
    float vx = st[2], vy = st[3], psi = st[4];
    for (int h = 0; h < H; ++h) {
      const int at = h * kVcStride + tid;
      const float an = h < Hc ? ta[at] : 0.0f, tn = h < Hc ? tt[at] : 0.0f;
      ta[at] = x;  // the point recorded at h is the state before step h
      tt[at] = y;
      if (h == Hc) break;
      bicycle_step_cr_t(x, y, vx, vy, psi, an, tn, v.wheel_base);
    }
  }
  __syncthreads();

  // phase B: a quad per point, h fastest (the quads of a wave hit different counters)
  const int total = rows * H, q = tid & 3;
  for (int base = 0; base < total; base += kVcThreads / 4) {
    const int e = base + (tid >> 2);  // quad-uniform
    if (e < total) {
      const int rr = e / H, h = e - rr * H;
      float s, d;
      frenet_point_quad(ta[h * kVcStride + rr], tt[h * kVcStride + rr], pxy, arc, Fxd, Fyd, P, Pq, s, d);
      bool any = false;
      uint32_t ko = 0u;
      for (int o = q; o < O; o += 4) {
        const float f = f_bar_ab(s, d, xo[o * H + h], yo[o * H + h], v.obs_a2, v.obs_b2);
        if (!(f <= 0.0f)) {  // k_validate's convention: count_nonzero(max(0, f)), a NaN counts
          atomicAdd(&cnt[o * H + h], 1);
          any = true;
        }
        if constexpr (kCosts) ko = max(ko, vc_cost_key(f));
      }
      if (any) flag[rr] = 1;
      if (q == 0) {
        if (-d + v.y_lb > 0.0f) atomicAdd(&clb[h], 1);
        if (d - v.y_ub > 0.0f) atomicAdd(&cub[h], 1);
      }
      if constexpr (kCosts) {  // the point's three keys into the row's maxima; a zero key changes nothing
        ko = lane_reduce<Scope::Quad, LaneMaxU>(ko);
        if (q == 0) {
          const uint32_t kl = vc_cost_key(-d + v.y_lb), ku = vc_cost_key(d - v.y_ub);
          if (ko) atomicMax(&cmax[rr], ko);
          if (kl) atomicMax(&cmax[kVcRows + rr], kl);
          if (ku) atomicMax(&cmax[2 * kVcRows + rr], ku);
        }
      }
    }
  }
  __syncthreads();

  int* gc = v.cnt_oh + size_t(k) * O * H;
  for (int i = tid; i < O * H; i += kVcThreads) {
    const int c = cnt[i];
    if (c) atomicAdd(&gc[i], c);
  }
  int* gl = v.cnt_lane + size_t(k) * 2 * H;
  for (int h = tid; h < H; h += kVcThreads) {
    if (clb[h]) atomicAdd(&gl[h], clb[h]);
    if (cub[h]) atomicAdd(&gl[H + h], cub[h]);
  }
  if (tid < 64) {
    const bool f = tid < rows && flag[tid] != 0;
    const int n = __popcll(__ballot(f));
    if (tid == 0 && n) atomicAdd(&v.count_rows[k], n);
  }
  if constexpr (kCosts)
    if (tid < rows)  // coalesced per channel
      for (int c = 0; c < 3; ++c)
        v.costs[(size_t(k) * 3 + c) * R + r0 + tid] = __uint_as_float(cmax[c * kVcRows + tid]);
}

template <int kDraws, int kVcThreads>
__global__ __launch_bounds__(kVcThreads) void k_validate_carla(ValidateCarlaParams v) {
  vc_body<kDraws, kVcThreads, false>(v);
}
template <int kDraws, int kVcThreads>
__global__ __launch_bounds__(kVcThreads) void k_validate_carla_costs(ValidateCarlaParams v) {
  vc_body<kDraws, kVcThreads, true>(v);
}

// count = max_{o,h} count_oh, count_lane = max_h #lb + max_h #ub (S/validation.py:153-169)
__global__ __launch_bounds__(64) void k_validate_carla_max(ValidateCarlaParams v) {
  const int k = blockIdx.x, tid = threadIdx.x, O = v.O, H = v.H;
  const int* gc = v.cnt_oh + size_t(k) * O * H;
  const int* gl = v.cnt_lane + size_t(k) * 2 * H;
  int m = 0, mlb = 0, mub = 0;
  for (int i = tid; i < O * H; i += 64) m = max(m, gc[i]);
  for (int i = tid; i < H; i += 64) {
    mlb = max(mlb, gl[i]);
    mub = max(mub, gl[H + i]);
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

}  // namespace

bool validate_carla_shape_ok(int O, int H, int P) {
  return O >= 1 && O <= kVcMaxObs && H >= 2 && H <= kMaxH && P >= 4 && P <= kMaxPath;
}

size_t validate_carla_lds(int O, int H, int P, bool costs) { return vc_lds_words(O, H, P, costs) * 4; }

bool launch_validate_carla(const ValidateCarlaParams& v, size_t lds_limit, hipStream_t s) {
  const bool costs = v.costs != nullptr;
  const size_t lds = validate_carla_lds(v.O, v.H, v.P, costs);
  if (lds > lds_limit) return false;
  const int threads = v.draws ? kVcThreadsGiven : kVcThreadsDrawn;
  auto kern = v.draws ? k_validate_carla<0, kVcThreadsGiven>
                      : (v.noise == 0 ? k_validate_carla<1, kVcThreadsDrawn> : k_validate_carla<2, kVcThreadsDrawn>);
  if (costs)
    kern = v.draws ? k_validate_carla_costs<0, kVcThreadsGiven>
                   : (v.noise == 0 ? k_validate_carla_costs<1, kVcThreadsDrawn>
                                   : k_validate_carla_costs<2, kVcThreadsDrawn>);
  if (lds > 64 * 1024)  // above the default dynamic-LDS cap of a launch
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                              int(lds));
  hipLaunchKernelGGL(kern, dim3((v.R + kVcRows - 1) / kVcRows, v.K), dim3(threads), lds, s, v);
  hipLaunchKernelGGL(k_validate_carla_max, dim3(v.K), dim3(64), 0, s, v);
  return true;
}

}  // namespace mpcmmd
