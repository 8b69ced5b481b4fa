// k_belite, k_bgen, k_bgen_wave, k_bsigma: elites, the next generators and
// sigma_best (betacem_elite.hpp has the bodies).
#include "betacem_elite.hpp"

namespace mpcmmd {

namespace {

__global__ __launch_bounds__(kThreads) void k_belite(Params p, int tb) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  belite_body(p, tb, p.b0 + blockIdx.x, smem);
}

// k_bgen: level 2 of the generators, one quad (4 lanes) per (candidate,
// block of 16 positions).  The block prefix Phi_b (k_belite) is inverted
// once, A = Phi_b^-1; then, position by position through the block,
//   v_j = A u_j,  L_jj = sqrt(0.05 + u_j . v_j),  w_j = v_j / L_jj,
//   A <- A - w_j w_j^T      (= Phi_{j+1}^-1: Sherman-Morrison, since
//                            Phi_{j+1} = Phi_j + u_j u_j^T / 0.05)
// -- at most 15 rank-1 steps from an exactly inverted start, so the error
// stays at the level of one fp64 inversion.  Lane q of the quad owns rows
// q, q + 4, q + 8 of A (full rows, so A stays symmetric without a packed
// layout); the inverse is an in-place Gauss-Jordan sweep (Phi_b is SPD: no
// pivoting), its pivot rows and the w_j of each step quad broadcasts (DPP),
// so the chain per position is one 11-term dot product deep instead of the
// whole matrix-vector product, and the ~32 blocks x 4 lanes of a candidate
// give ~2 waves per SIMD at B = 1024 (one lane per block gave < 1).
// the generators of 16-position block blk of candidate b on the calling quad
// (lane q = tidx() & 3), after k_belite of beta-iteration tb; live = false:
// compute, store nothing.  st: the quad's kGenStage floats of LDS.
//
// u_j is formed from the elite rows and the mean (gen_u).  The rows are M + 1
// floats apart, so a position's 11 values lie in 11 cache lines that the
// block's other 15 positions need as well: read position by position, a wave
// (16 blocks) keeps ~100 lines live for the whole launch, more than L1 and L2
// hold for the resident waves (measured: twice the U plane's bytes from HBM,
// 54 against 38 us).  So the quad reads its block's 11 x 16 floats once, every
// line in one go -- lane q its own rows q, q + 4, q + 8 as four float4 each --
// and stages them by position in LDS, [16 positions][12] (slot 11 zero).
constexpr int kGenStage = 16 * 12 + 4;  // + 4: 16 quads' float4 reads tile the 64 banks
DEVI void bgen_quad(const Params& p, int tb, int b, int blk, bool live, float* st) {
  const int M = p.M, M1 = M + 1, nblk = (M1 + 15) / 16;
  const int q = tidx() & 3;
  double* gen = p.gen + size_t(b) * pos_pad(M) * kGenStride;
  const int j0 = blk * 16, j1 = min(M1, j0 + 16);
  {
    // raw buffer loads over the launch's elite rows: what lies past the
    // launch's last row is out of range (0); positions past M of the other
    // rows read the next row and are never used (j < j1 below)
    typedef float v4f __attribute__((ext_vector_type(4)));
    const __amdgpu_buffer_rsrc_t er = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(gen_elites(p, tb + 1, p.b0)), short(0), p.nb * kBetaElite * M1 * 4, 0x00020000);
    const int vb = ((b - p.b0) * kBetaElite * M1 + j0) * 4;
    v4f f[3][4];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int k = 0; k < 4; ++k)
        f[i][k] = __builtin_bit_cast(
            v4f, __builtin_amdgcn_raw_buffer_load_b128(er, vb + (min(q + 4 * i, 10) * M1 + 4 * k) * 4, 0, 0));
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int w = 0; w < 4; ++w) st[(4 * k + w) * 12 + q + 4 * i] = q + 4 * i < 11 ? f[i][k][w] : 0.0f;
    wave_sync();
  }
  const double* Gb = p.phib + (size_t(b) * nblk + blk) * 66;
  // own rows a = q + 4 i; row 11 (q = 3, i = 2) is padding: an identity row
  // that no other row reads (column 11 does not exist)
  double A[3][11];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int a = q + 4 * i;
#pragma unroll
    for (int c = 0; c < 11; ++c) A[i][c] = a < 11 ? Gb[sym11i(a, c)] : 0.0;
  }
  // in-place Gauss-Jordan inversion
#pragma unroll
  for (int k = 0; k < 11; ++k) {
    const int ik = k >> 2, ok = k & 3;
    const double ip = 1.0 / quad_bcast(A[ik][k], ok);  // the pivot, from its owner lane
    double f[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) f[i] = A[i][k];
    // column by column: entry c of pivot row k (broadcast before its owner
    // overwrites it), scaled, then every own row's update
#pragma unroll
    for (int c = 0; c < 11; ++c) {
      const double rc = c == k ? ip : quad_bcast(A[ik][c], ok) * ip;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const bool pivot_row = q + 4 * i == k;
        A[i][c] = pivot_row ? rc : (c == k ? -f[i] * ip : fma(-f[i], rc, A[i][c]));
      }
    }
  }
  // The quad's four lanes read a position's 11 floats (three float4) and its
  // mean; the next position's in flight, as fp32, while one is processed; and
  // the lane's own components q + 4 i again (slot 11 is zero and masked at
  // use), so the dot u . v needs no lane-dependent register selects
  typedef float v4f __attribute__((ext_vector_type(4)));
  const double* mrow = gen_mean_row(p, b);
  float en[12], eon[3];
  double mn = mrow[j0];
  auto stage_ld = [&](int jj) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const v4f f = *reinterpret_cast<const v4f*>(st + jj * 12 + 4 * k);
#pragma unroll
      for (int w = 0; w < 4; ++w) en[4 * k + w] = f[w];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) eon[i] = st[jj * 12 + q + 4 * i];
  };
  stage_ld(0);
  for (int j = j0; j < j1; ++j) {
    double u[11], uo[3];
#pragma unroll
    for (int c = 0; c < 11; ++c) u[c] = gen_u(en[c], mn);
#pragma unroll
    for (int i = 0; i < 3; ++i) uo[i] = gen_u(eon[i], mn);
    const int jn = min(j + 1, j1 - 1);
    mn = mrow[jn];
    stage_ld(jn - j0);
    double v[3], part = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      double s = 0.0;
#pragma unroll
      for (int c = 0; c < 11; ++c) s = fma(A[i][c], u[c], s);
      v[i] = s;
      const int a = q + 4 * i;
      part = fma(i < 2 || a < 11 ? uo[i] : 0.0, s, part);
    }
    const double uv = quad_sum(part);
    const double ljj = sqrt(kRidge + uv);
    const double rl = 1.0 / ljj;
    double w[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) w[i] = v[i] * rl;
    double* g = gen + size_t(j) * kGenRow;
    if (live) {
#pragma unroll
      for (int i = 0; i < 3; ++i) g[kGenW + q + 4 * i] = q + 4 * i < 11 ? w[i] : 0.0;  // whole rows: slot 11 is 0
      if (q == 0) p.genm[size_t(b) * pos_pad(M) + j] = ljj;
    }
#pragma unroll
    for (int c = 0; c < 11; ++c) {
      const double wc = quad_bcast(w[c >> 2], c & 3);
#pragma unroll
      for (int i = 0; i < 3; ++i) A[i][c] = fma(-w[i], wc, A[i][c]);
    }
  }
}

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void k_bgen(Params p, int tb) {
  const int nblk = (p.M + 1 + 15) / 16;
  const int gq = (blockIdx.x * blockDim.x + tidx()) >> 2;
  const bool live = gq < p.nb * nblk;  // quads stay whole: dead ones compute on a clamped block, store nothing
  const int gqc = live ? gq : p.nb * nblk - 1;
  __shared__ __attribute__((aligned(16))) float stage[64 * kGenStage];
  bgen_quad(p, tb, p.b0 + gqc / nblk, gqc % nblk, live, stage + (tidx() >> 2) * kGenStage);
}

constexpr int kGenWaveWaves = 4;
__global__ __launch_bounds__(64 * kGenWaveWaves) void k_bgen_wave(Params p, int tb) {
  __shared__ double xl[kGenWaveWaves][32];
  const int nblk = (p.M + 1 + 15) / 16;
  const int w = tidx() >> 6, gw = blockIdx.x * kGenWaveWaves + w;
  if (gw >= p.nb * nblk) return;  // whole waves; no workgroup barrier below
  bgen_wave(p, tb, p.b0 + gw / nblk, gw % nblk, xl[w]);
}

__global__ __launch_bounds__(kThreads) void k_bsigma(Params p, int tb) {
  __shared__ double red[(kThreads / 64) * 11];
  const int b = p.b0 + blockIdx.x;
  if (p.bimin[b] < kBetaElite) return;  // k_belite wrote it
  bsigma_body(p, tb, b, red);
}

}  // namespace

void launch_belite(const Params& p, int tb, hipStream_t s) {
  const EliteLds e = elite_lds(p.M + 1);
  hipLaunchKernelGGL(k_belite, dim3(p.nb), dim3(kThreads), e.total, s, p, tb);
}

// (k_bcem_small's generators are bgen_wave's: handles with gen_wave only)
void launch_bgen(const Params& p, int tb, hipStream_t s) {
  const int nblk = (p.M + 1 + 15) / 16;
  if (p.gen_wave)
    hipLaunchKernelGGL(k_bgen_wave, dim3((p.nb * nblk + kGenWaveWaves - 1) / kGenWaveWaves), dim3(64 * kGenWaveWaves), 0,
                       s, p, tb);
  else
    hipLaunchKernelGGL(k_bgen, dim3((p.nb * nblk * 4 + 255) / 256), dim3(256), 0, s, p, tb);
  if (tb == kBetaIters - 1) hipLaunchKernelGGL(k_bsigma, dim3(p.nb), dim3(kThreads), 0, s, p, tb);
}

}  // namespace mpcmmd
