// Monte-Carlo risk statistics of saved optima (mpcmmd_validate_risk): the
// optimizer's own cost terms at validation sample sizes.
//
//   k_vrisk_roll     k_validate's fp64 rollouts, 1024 per workgroup, reduced to
//                    three running maxima per rollout (max f_bar over (o, h),
//                    max lane_lb, max lane_ub over h), stored as fp32.  No
//                    atomics: a value depends on (k, r) only.
//   k_vrisk_stats    a workgroup per (k, channel): count of !(c <= 0), fp64 sum,
//                    maximum; the two order statistics of the linear quantile by
//                    an exact MSB-first radix selection (11 / 11 / 10 bits, LDS
//                    histograms) on the total-order keys (common.hpp sort_key:
//                    -0 == +0, NaN last); then the CVaR sum and count.
//   k_vrisk_compact  the non-zero values of a channel in index order (prefix
//                    scan), so the MMD's zeros are summed in closed form
//   k_vrisk_mmd      the pair sum of the P non-zero values by 1024-value tiles:
//                    an i-tile sits in registers and walks the j-tiles at or
//                    after it through LDS (broadcast reads), the diagonal once,
//                    the others twice; terms exp2(d (-log2 e / sigma)) on
//                    v_exp_f32, every bandwidth on one |u_p - u_q|
//   k_vrisk_mmd_fin  adds the tile partials in tile order, the single sums and
//                    the zeros' closed form
// Every reduction runs lane -> wave -> workgroup in a fixed order and nothing
// accumulates through floating-point atomics: a call's bits do not depend on
// the launch geometry or on timing.
#include <hip/hip_runtime.h>

#include "common.hpp"
#include "kernels.hpp"
#include "rng.hpp"
#include "validate_step.hpp"

namespace mpcmmd {
namespace {

constexpr int kStatThreads = 1024;
constexpr int kStatWaves = kStatThreads / kWave;
constexpr int kHistBins = 2048;
constexpr int kPairThreads = 256;
constexpr int kPairPerLane = kRiskTile / kPairThreads;  // i-values a lane holds
constexpr float kRiskNegLog2e = -1.44269504088896340736f;
constexpr double kKerWt = 1000.0;  // prob.ker_wt

// ---- rollouts ------------------------------------------------------------------
__global__ __launch_bounds__(kValThreads) void k_vrisk_roll(ValidateRiskParams p) {
  __shared__ double sacc[kValMaxH], ssteer[kValMaxH], sv[kValMaxH];
  __shared__ float sxo[kValMaxObs * kValMaxH], syo[kValMaxObs * kValMaxH];
  const ValidateParams& v = p.roll;
  const int k = blockIdx.y, tid = threadIdx.x;
  const int H = v.H, O = v.O, R = v.R;
  const ValNoise vn{v.noise, v.noise_level, v.acc_const, v.steer_const, v.K_steer};
  const double* cx = v.cx + size_t(k) * 11;
  const double* cy = v.cy + size_t(k) * 11;
  for (int i = tid; i < O * H; i += kValThreads) {
    const int o = i / H, h = i - o * H;
    sxo[i] = v.x_obs[(size_t(k) * O + o) * 100 + h];
    syo[i] = v.y_obs[(size_t(k) * O + o) * 100 + h];
  }
  val_controls(v.Pdot, v.Pddot, cx, cy, H, tid, sv, sacc, ssteer);
  const int r = blockIdx.x * kValThreads + tid;
  if (r >= R) return;
  const double* st = v.init_state + size_t(k) * 6;
  const uint32_t k0 = v.keys[k], k1 = v.seed;
  const double* dr = v.draws ? v.draws + size_t(k) * 3 * R * H : nullptr;
  double x = st[0], y = st[1], vx = st[2], vy = st[3], psi = atan2(st[3], st[2]);
  // running maxima of max(0, .): start at 0, a NaN stays (np.maximum)
  double mo = 0.0, mlb = 0.0, mub = 0.0;
  for (int h = 0; h < H; ++h) {
    for (int o = 0; o < O; ++o) {
      const double wc = x - double(sxo[o * H + h]), ws = y - double(syo[o * H + h]);
      const double c = -(wc * wc) / 18.0625 - (ws * ws) / 7.5625 + 1.0;
      if (c > mo || c != c) mo = c;
    }
    const double lb = -y + v.y_lb, ub = y - v.y_ub;
    if (lb > mlb || lb != lb) mlb = lb;
    if (ub > mub || ub != ub) mub = ub;
    if (h == H - 1) break;
    double an, sn;
    val_noisy_controls(vn, dr, R, H, r, h, k0, k1, sacc[h], ssteer[h], an, sn);
    val_bicycle_step(an, sn, x, y, vx, vy, psi);
  }
  float* out = p.costs + size_t(k) * 3 * R;
  out[r] = float(mo);
  out[size_t(R) + r] = float(mlb);
  out[2 * size_t(R) + r] = float(mub);
}

// ---- workgroup reductions: lane, then wave, then the waves in order ---------------
template <class T>
DEVI T block_total(T v, T* sh) {  // sh [waves of the workgroup]
  v = wave_total(v);
  const int nw = blockDim.x / kWave;
  __syncthreads();  // the previous use of sh
  if ((threadIdx.x & (kWave - 1)) == 0) sh[threadIdx.x / kWave] = v;
  __syncthreads();
  T t = sh[0];
  for (int i = 1; i < nw; ++i) t += sh[i];
  return t;
}

// the value of a total-order key (sort_key's inverse; -0 comes back as +0)
DEVI float key_value(uint32_t key) {
  if (key == 0xFFFFFFFFu) return __uint_as_float(0x7FC00000u);
  return __uint_as_float((key >> 31) ? (key & 0x7FFFFFFFu) : ~key);
}

// one count into an LDS histogram; a wave whose active lanes share a bin (the
// all-zero channel) adds their number once
DEVI void hist_add(uint32_t* hist, uint32_t bin) {
  const unsigned long long act = __ballot(1);
  const uint32_t b0 = __builtin_amdgcn_readfirstlane(bin);
  if (__ballot(bin == b0) == act) {
    if ((threadIdx.x & (kWave - 1)) == uint32_t(__ffsll(act) - 1)) atomicAdd(&hist[b0], uint32_t(__popcll(act)));
  } else {
    atomicAdd(&hist[bin], 1u);
  }
}

// Key of rank q (0-based, ascending) among the R values of c: three histogram
// passes over the key's bits [31:21], [20:10], [9:0].  Uniform result.
DEVI uint32_t select_rank(const float* c, int R, uint32_t q, uint32_t* hist, uint32_t* pick) {
  const int tid = threadIdx.x;
  uint32_t prefix = 0;
  for (int level = 0; level < 3; ++level) {
    const int shift = level == 0 ? 21 : level == 1 ? 10 : 0;
    const int bits = level == 2 ? 10 : 11;
    for (int i = tid; i < kHistBins; i += kStatThreads) hist[i] = 0;
    __syncthreads();
    for (int i = tid; i < R; i += kStatThreads) {
      const uint32_t key = sort_key(c[i]);
      // the bits above this level's equal the prefix (level 0: none above)
      if (level == 0 || (key >> (shift + bits)) == prefix) hist_add(hist, (key >> shift) & ((1u << bits) - 1u));
    }
    __syncthreads();
    if (tid < kWave) {  // wave 0: 32 bins per lane, lane scan, then the owning lane walks its bins
      constexpr int kPer = kHistBins / kWave;
      uint32_t s = 0;
      for (int j = 0; j < kPer; ++j) s += hist[tid * kPer + j];
      uint32_t inc = s;
      for (int o = 1; o < kWave; o <<= 1) {
        const uint32_t t = __shfl_up(inc, o, kWave);
        if (tid >= o) inc += t;
      }
      uint32_t ex = inc - s;
      if (ex <= q && q < inc) {  // exactly one lane: the counts of the level total more than q
        int b = tid * kPer;
        for (int j = 0; j < kPer - 1; ++j) {
          const uint32_t hc = hist[b];
          if (q < ex + hc) break;
          ex += hc;
          ++b;
        }
        pick[0] = uint32_t(b);
        pick[1] = q - ex;
      }
    }
    __syncthreads();
    prefix = (prefix << bits) | pick[0];
    q = pick[1];
    __syncthreads();  // pick and hist are rewritten by the next level
  }
  return prefix;
}

__global__ __launch_bounds__(kStatThreads) void k_vrisk_stats(ValidateRiskParams p) {
  __shared__ uint32_t hist[kHistBins];
  __shared__ uint32_t pick[2];
  __shared__ double shd[kStatWaves];
  __shared__ uint32_t shu[kStatWaves];
  const int kc = blockIdx.x, tid = threadIdx.x, R = p.R;
  const float* c = p.costs + size_t(kc) * R;
  // pass 1: count of !(c <= 0) (a NaN counts), fp64 sum, largest key
  uint32_t npos = 0, kmax = 0;
  double sum = 0.0;
  for (int i = tid; i < R; i += kStatThreads) {
    const float x = c[i];
    npos += !(x <= 0.0f) ? 1u : 0u;
    sum += double(x);
    kmax = max(kmax, sort_key(x));
  }
  npos = block_total(npos, shu);
  sum = block_total(sum, shd);
  kmax = ~wave_min_u32(~kmax);
  __syncthreads();
  if ((tid & (kWave - 1)) == 0) shu[tid / kWave] = kmax;
  __syncthreads();
  for (int i = 0; i < kStatWaves; ++i) kmax = max(kmax, shu[i]);
  // the quantile's two order statistics
  const uint32_t klo = select_rank(c, R, uint32_t(p.lo), hist, pick);
  const uint32_t khi = p.hi == p.lo ? klo : select_rank(c, R, uint32_t(p.hi), hist, pick);
  const float var = key_value(klo) * p.w_lo + key_value(khi) * p.w_hi;  // fp32, no contraction (costs.py quantile_linear)
  // pass 3: mean of the samples >= var (a NaN compares false)
  double cs = 0.0;
  uint32_t cn = 0;
  for (int i = tid; i < R; i += kStatThreads) {
    const float x = c[i];
    if (x >= var) {
      cs += double(x);
      ++cn;
    }
  }
  cn = block_total(cn, shu);
  cs = block_total(cs, shd);
  if (tid == 0) {
    p.count_pos[kc] = int32_t(npos);
    p.mean[kc] = float(sum / double(R));
    p.vmax[kc] = key_value(kmax);
    p.var[kc] = var;
    p.cvar[kc] = cn ? float(cs / double(cn)) : 0.0f;
  }
}

// ---- MMD -----------------------------------------------------------------------
__global__ __launch_bounds__(kStatThreads) void k_vrisk_compact(ValidateRiskParams p) {
  __shared__ uint32_t wtot[kStatWaves];
  const int kc = blockIdx.x, tid = threadIdx.x, R = p.R;
  const int lane = tid & (kWave - 1), w = tid / kWave;
  const float* c = p.costs + size_t(kc) * R;
  float* u = p.u + size_t(kc) * R;
  uint32_t base = 0;
  for (int i0 = 0; i0 < R; i0 += kStatThreads) {  // chunks in index order
    const int i = i0 + tid;
    const float x = i < R ? c[i] : 0.0f;
    const bool nz = !(x == 0.0f);  // either zero; a NaN is kept
    const unsigned long long m = __ballot(nz);
    if (lane == 0) wtot[w] = uint32_t(__popcll(m));
    __syncthreads();
    uint32_t off = base, tot = 0;
    for (int j = 0; j < kStatWaves; ++j) {
      const uint32_t t = wtot[j];
      if (j < w) off += t;
      tot += t;
    }
    if (nz) u[off + uint32_t(__popcll(m & ((1ull << lane) - 1ull)))] = x;  // off + rank < base + tot <= R
    base += tot;
    __syncthreads();
  }
  if (tid == 0) p.np[kc] = int32_t(base);
}

typedef float f2 __attribute__((ext_vector_type(2)));

// Workgroup b sums i-tiles b and nt - 1 - b (nt + 1 tile pairs together,
// whatever b), each against the j-tiles at or after it.  A lane holds four
// i-values as two packed pairs (packed differences and scales); every term is
// converted and added in fp64.
template <int S>
__global__ __launch_bounds__(kPairThreads) void k_vrisk_mmd(ValidateRiskParams p, int T) {
  __shared__ __attribute__((aligned(16))) float uj[kRiskTile];
  __shared__ double shd[kPairThreads / kWave];
  const int blk = blockIdx.x, k = blockIdx.y, kc = k * 3 + blockIdx.z, tid = threadIdx.x;
  const int P = p.np[kc];  // known only here
  const int nt = (P + kRiskTile - 1) / kRiskTile;
  if (2 * blk >= nt) return;
  const float* u = p.u + size_t(kc) * p.R;
  float cs[S];
#pragma unroll
  for (int s = 0; s < S; ++s) cs[s] = kRiskNegLog2e / p.sigma[size_t(k) * S + s];
  for (int half = 0; half < 2; ++half) {
    const int ti = half == 0 ? blk : nt - 1 - blk;
    if (half == 1 && ti == blk) break;  // the middle tile of an odd nt
    // pads: +inf on the i side, -inf on the j side, so every pair with a pad is
    // at distance +inf and adds exp2(-inf) = 0
    f2 ui[kPairPerLane / 2];
#pragma unroll
    for (int a = 0; a < kPairPerLane; ++a) {
      const int i = ti * kRiskTile + a * kPairThreads + tid;
      ui[a / 2][a % 2] = i < P ? u[i] : __builtin_inff();
    }
    double acc[S];
#pragma unroll
    for (int s = 0; s < S; ++s) acc[s] = 0.0;
    for (int tj = ti; tj < nt; ++tj) {
      __syncthreads();
#pragma unroll
      for (int a = 0; a < kPairPerLane; ++a) {
        const int j = tj * kRiskTile + a * kPairThreads + tid;
        uj[a * kPairThreads + tid] = j < P ? u[j] : -__builtin_inff();
      }
      __syncthreads();
      double tacc[S][kPairPerLane];  // a sum per i-value of the lane: independent fp64 chains
#pragma unroll
      for (int s = 0; s < S; ++s)
#pragma unroll
        for (int a = 0; a < kPairPerLane; ++a) tacc[s][a] = 0.0;
      for (int j4 = 0; j4 < kRiskTile / 4; ++j4) {
        const float4 b4 = reinterpret_cast<const float4*>(uj)[j4];
        const float b[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          f2 d[kPairPerLane / 2];
#pragma unroll
          for (int a = 0; a < kPairPerLane / 2; ++a) {
            const f2 df = ui[a] - f2{b[e], b[e]};
            d[a] = f2{fabsf(df.x), fabsf(df.y)};
          }
#pragma unroll
          for (int s = 0; s < S; ++s) {
#pragma unroll
            for (int a = 0; a < kPairPerLane / 2; ++a) {  // every term converted, then added in fp64
              const f2 x = d[a] * cs[s];
              tacc[s][2 * a] += double(__builtin_amdgcn_exp2f(x.x));
              tacc[s][2 * a + 1] += double(__builtin_amdgcn_exp2f(x.y));
            }
          }
        }
      }
      const double wgt = tj == ti ? 1.0 : 2.0;
#pragma unroll
      for (int s = 0; s < S; ++s) {
        double t = tacc[s][0];
#pragma unroll
        for (int a = 1; a < kPairPerLane; ++a) t += tacc[s][a];
        acc[s] += wgt * t;
      }
    }
#pragma unroll
    for (int s = 0; s < S; ++s) {
      const double t = block_total(acc[s], shd);
      if (tid == 0) p.part[(size_t(kc) * T + ti) * S + s] = t;
    }
  }
}

__global__ __launch_bounds__(kPairThreads) void k_vrisk_mmd_fin(ValidateRiskParams p, int T) {
  __shared__ double shd[kPairThreads / kWave];
  const int kc = blockIdx.x, k = kc / 3, tid = threadIdx.x, R = p.R, S = p.S;
  const int P = p.np[kc], nt = (P + kRiskTile - 1) / kRiskTile;
  const float* u = p.u + size_t(kc) * R;
  for (int s = 0; s < S; ++s) {
    const float cs = kRiskNegLog2e / p.sigma[size_t(k) * S + s];
    double a = 0.0;
    for (int i = tid; i < P; i += kPairThreads) a += double(__builtin_amdgcn_exp2f(fabsf(u[i]) * cs));
    const double s1 = block_total(a, shd);
    if (tid == 0) {
      double pp = 0.0;
      for (int t = 0; t < nt; ++t) pp += p.part[(size_t(kc) * T + t) * S + s];
      const double Z = double(R - P), Rd = double(R);
      const double ss = Z * Z + 2.0 * Z * s1 + pp;  // the zeros in closed form
      p.mmd[size_t(kc) * S + s] = float(kKerWt * (ss / (Rd * Rd) - 2.0 * (Z + s1) / Rd));
    }
  }
}

template <int S>
void launch_pairs(const ValidateRiskParams& v, int T, hipStream_t s) {
  hipLaunchKernelGGL(k_vrisk_mmd<S>, dim3((T + 1) / 2, v.K, 3), dim3(kPairThreads), 0, s, v, T);
}

}  // namespace

void launch_vrisk_roll(const ValidateRiskParams& v, hipStream_t s) {
  hipLaunchKernelGGL(k_vrisk_roll, dim3((v.R + kValThreads - 1) / kValThreads, v.K), dim3(kValThreads), 0, s, v);
}

void launch_vrisk_stats(const ValidateRiskParams& v, hipStream_t s) {
  hipLaunchKernelGGL(k_vrisk_stats, dim3(3 * v.K), dim3(kStatThreads), 0, s, v);
}

void launch_vrisk_mmd(const ValidateRiskParams& v, hipStream_t s) {
  if (v.S < 1) return;
  const int T = (v.R + kRiskTile - 1) / kRiskTile;
  hipLaunchKernelGGL(k_vrisk_compact, dim3(3 * v.K), dim3(kStatThreads), 0, s, v);
  switch (v.S) {
    case 1: launch_pairs<1>(v, T, s); break;
    case 2: launch_pairs<2>(v, T, s); break;
    case 3: launch_pairs<3>(v, T, s); break;
    case 4: launch_pairs<4>(v, T, s); break;
    case 5: launch_pairs<5>(v, T, s); break;
    case 6: launch_pairs<6>(v, T, s); break;
    case 7: launch_pairs<7>(v, T, s); break;
    default: launch_pairs<8>(v, T, s); break;
  }
  hipLaunchKernelGGL(k_vrisk_mmd_fin, dim3(3 * v.K), dim3(kPairThreads), 0, s, v, T);
}

}  // namespace mpcmmd
