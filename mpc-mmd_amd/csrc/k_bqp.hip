// k_bqp, k_bqp_wave: the QP of every sample of a beta-iteration
// (betacem_qp.hpp has the quad body).
#include "betacem_qp.hpp"

namespace mpcmmd {

namespace {

template <int NP>
__global__ __launch_bounds__(qp_threads(NP), NP == 24 ? 3 : (NP <= 16 ? 4 : 2)) void k_bqp(Params p, int tb) {
  extern __shared__ __attribute__((aligned(16))) float kl[];
  bqp_quad<NP>(p, tb, kl);
}

// k_bqp_wave: the same QP for 32 < n <= 64, one wave per QP, lane i owns
// row i of C (NP floats in registers).  Right-looking Cholesky with the
// column entries broadcast by v_readlane (entries above the diagonal are
// left stale and zeroed when their column is reached, never read); forward
// solves for g and 1 together; then, since C^-1 = L^-T L^-1,
//   sum x1 = y2.y1, sum x2 = |y2|^2, beta = L^-T (y1 + alpha y2),
// one backward solve (column sums as wave reductions).  fp32 like the quad
// kernel; the cost beta^T K beta - 2 g^T beta in fp64 on the fp32 beta with
// K_red re-read.
template <int NP>
__global__ __launch_bounds__(256) void k_bqp_wave(Params p, int tb) {
  const int lane = tidx() & 63;
  const int n = p.n, M = p.M;
  const int s_lo = first_sample(tb), per = kBetaSamples - s_lo;
  const int gq = blockIdx.x * 4 + (tidx() >> 6);
  if (gq >= p.nb * per) return;  // whole waves
  const int b = p.b0 + gq / per, s = s_lo + gq % per;
  const int ntri = tri_stride(n);
  const float* kr = p.bkred + (size_t(b) * kBetaSamples + s) * ntri;
  const float* br = p.brow + (size_t(b) * kBetaSamples + s) * n;
  const double inv_m = double(1.0f / float(M));
  const float cdiag = 1.0f + 0.05f;
  const bool real = lane < n;
  float A[NP];
  const int ic = min(lane, n - 1);
#pragma unroll
  for (int k = 0; k < NP; ++k) {  // unconditional loads (clamped entry), masked after
    const int e = ic > 0 ? ic * (ic - 1) / 2 + max(min(k, ic - 1), 0) : 0;
    A[k] = kr[e];
  }
  const double gd = real ? double(br[ic]) * inv_m : 0.0;
#pragma unroll
  for (int k = 0; k < NP; ++k) {
    float v = (k < lane && real) ? A[k] : 0.0f;
    if (k == lane) v = real ? cdiag : 1.0f;
    A[k] = v;
  }
  float rdiag = 1.0f;
  // Cholesky, column j
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    const float djj = readlane(A[j], j);
    const float y = rsqrt_nr(djj);
    const float lij = A[j] * y;
    A[j] = lane > j ? lij : (lane == j ? djj * y : 0.0f);
    if (lane == j) rdiag = y;
#pragma unroll
    for (int k = j + 1; k < NP; ++k) A[k] = fmaf(-A[j], readlane(A[j], k), A[k]);
  }
  // forward: L y = (g, 1)
  float y1 = float(gd), y2 = real ? 1.0f : 0.0f;
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    const float t1 = readlane(y1 * rdiag, j), t2 = readlane(y2 * rdiag, j);
    y1 = lane == j ? t1 : fmaf(-A[j], t1, y1);
    y2 = lane == j ? t2 : fmaf(-A[j], t2, y2);
  }
  const float s1 = wave_total(y2 * y1), s2 = wave_total(y2 * y2);
  const float alpha = (1.0f - s1) / s2;
  const float wv = fmaf(alpha, y2, y1);
  // backward: L^T beta = w
  float bet = 0.0f;
#pragma unroll
  for (int j = NP - 1; j >= 0; --j) {
    const float r = wave_total(A[j] * bet);
    if (lane == j) bet = (wv - r) * rdiag;
  }
  const float bf = real ? bet : 0.0f;
  const double bd = double(bf);
  // cost = bd^T K bd - 2 g^T bd, K = K_red (unit diagonal)
  double kb = bd;
#pragma unroll 8
  for (int k = 0; k < NP; ++k) {
    const double bk = double(readlane(bf, k));
    if (k != lane && real && k < n) {
      const int e = k < lane ? lane * (lane - 1) / 2 + k : k * (k - 1) / 2 + lane;
      kb = fma(double(kr[e]), bk, kb);
    }
  }
  const double c1 = wave_total(bd * kb), c3 = wave_total(gd * bd);
  float* bt = p.btop + (size_t(b) * kBetaSamples + s) * n;
  if (real) bt[lane] = bf;
  if (lane == 0) p.bcost[size_t(b) * kBetaSamples + s] = float(c1 - 2.0 * c3);
}

}  // namespace

template <int NP>
void launch_bqp_quad(const Params& p, int tb, int qps, hipStream_t s) {
  // threads per workgroup: qp_threads, or 64 (16 QPs) where the launch
  // would give the CUs barely one workgroup each (Params::qp_small)
  const int T = p.qp_small && (qps + 31) / 32 < 2 * kCUs ? 64 : qp_threads(NP);
  const size_t lds = (size_t(T / 4) * tri_stride(p.n) + kQpZeros) * 4;
  hipLaunchKernelGGL((k_bqp<NP>), dim3((qps * 4 + T - 1) / T), dim3(T), lds, s, p, tb);
}

void launch_bqp(const Params& p, int tb, hipStream_t s) {
  const int qps = p.nb * (kBetaSamples - first_sample(tb));
  const dim3 grid_wave((qps + 3) / 4);
  switch (qp_np(p.n)) {
    case 8:
      return launch_bqp_quad<8>(p, tb, qps, s);
    case 12:
      return launch_bqp_quad<12>(p, tb, qps, s);
    case 16:
      return launch_bqp_quad<16>(p, tb, qps, s);
    case 24:
      return launch_bqp_quad<24>(p, tb, qps, s);
    case 32:
      return launch_bqp_quad<32>(p, tb, qps, s);
    case 48:
      hipLaunchKernelGGL((k_bqp_wave<48>), grid_wave, dim3(256), 0, s, p, tb);
      return;
    default:
      hipLaunchKernelGGL((k_bqp_wave<64>), grid_wave, dim3(256), 0, s, p, tb);
      return;
  }
}

}  // namespace mpcmmd
