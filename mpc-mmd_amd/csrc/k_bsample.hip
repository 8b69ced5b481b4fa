// k_bsample_chunks, k_bsel0, k_bselect: a beta-iteration's new samples in
// small launches and the top-n selection (betacem_common.hpp has the
// pipeline; k_bsample_walk.hip has the one-wave sampler of large launches).
#include <algorithm>

#include "betacem_sample.hpp"
#include "betacem_select.hpp"

namespace mpcmmd {

namespace {

// The first beta-iteration's selection from the handle's table (Params::sel0,
// sig0: k_bselect's output for the shared initial samples, computed once per
// table) into every candidate's bsel / bsig.
__global__ __launch_bounds__(256) void k_bsel0(Params p) {
  const int n = p.n, per = kBetaSamples * n + kBetaSamples;
  for (size_t x = size_t(blockIdx.x) * 256 + tidx(); x < size_t(p.nb) * per; x += size_t(gridDim.x) * 256) {
    const int c = int(x / per), e = int(x - size_t(c) * per), b = p.b0 + c;
    if (e < kBetaSamples * n)
      p.bsel[size_t(b) * kBetaSamples * n + e] = p.sel0[e];
    else
      p.bsig[size_t(b) * kBetaSamples + e - kBetaSamples * n] = p.sig0[e - kBetaSamples * n];
  }
}

// k_bsample_chunks: the samples of k_bsample for small batches, workgroup =
// (candidate, tile of 16 samples), one wave per chunk of blocks.  Phase 1:
// each wave but the last sums W^T Z over its chunk (the MFMAs of the walker's
// S_loc, from zero) into LDS; phase 2: S_pre = the earlier chunks' sums in
// order (the walker's folds), then the chunk's blocks as in k_bsample.
__global__ __launch_bounds__(64 * kChunkWavesMax) void k_bsample_chunks(Params p, int tb) {
  __shared__ double dS[kChunkWavesMax - 1][3][64];
  const int b = p.b0 + blockIdx.x, M = p.M, Pp = pos_pad(M), nblk = Pp >> 4;
  const int lane = tidx() & 63, k = tidx() >> 6, P = blockDim.x >> 6;
  const int r = lane & 15, h = lane >> 4, s0 = blockIdx.y * 16;
  const int cl = sample_chunk(nblk), c0 = k * cl, c1 = min(nblk, c0 + cl);
  MPCMMD_STAMP(p, 0);
  const double* G = p.gen + size_t(b) * Pp * kGenStride;
  const double* gm = p.genm + size_t(b) * Pp;
  const float* z = p.beta_z + size_t(tb - 1) * Pp * kBzCols;
  const int ys = ygen_stride(M);
  float* plane = p.ygen + size_t(b) * kBzCols * ys;
  if (k < P - 1) {
    // operands of W^T Z for block c: W[p0 + 4 kk + h][r], Z[p0 + 4 kk + h][s0 + r]
    auto ld = [&](double (&wa)[4], double (&zz)[4], int c) {
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        const size_t pos = size_t(c) * 16 + 4 * kk + h;
        wa[kk] = G[pos * kGenRow + kGenW + r];
        zz[kk] = double(z[bz_index(int(pos), s0 + r)]);
      }
    };
    d4 Sl = d4{0.0, 0.0, 0.0, 0.0};
    double wa[4], zz[4], wn[4], zn[4];
    ld(wa, zz, c0);
    for (int c = c0; c < c1; ++c) {
      ld(wn, zn, min(c + 1, c1 - 1));
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) Sl = mfma64(wa[kk], zz[kk], Sl);
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        wa[kk] = wn[kk];
        zz[kk] = zn[kk];
      }
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) dS[k][i][lane] = Sl[i];
  }
  __syncthreads();
  d4 S[1] = {d4{0.0, 0.0, 0.0, 0.0}}, Sp[1] = {d4{0.0, 0.0, 0.0, 0.0}};
  Sp[0][2] = h == 3 ? 1.0 : 0.0;  // row 11 of S_pre: the mean's coefficient (the chunks' row 11 sums are 0)
  for (int j = 0; j < k; ++j)
#pragma unroll
    for (int i = 0; i < 3; ++i) Sp[0][i] = Sp[0][i] + dS[j][i][lane];
  const float* E = gen_elites(p, tb, b);
  const double* mrow = gen_mean_row(p, b);
  // the last chunk ends with the last block that holds a position (the walker's bound)
  walk_blocks<1, true>(
      c0, min(sample_blocks(M), c1), M, r, h, S, Sp,
      [&](SampleBlock<1>& q, int q0) { load_block(q, G, E, mrow, gm, z, M, q0, s0, r, h); },
      [&](const d4* Yv, int q0, auto) { block_store<1>(Yv, plane, q0, M, ys, s0, r, h); }, [](int) {});
  MPCMMD_STAMP(p, 1);
}

template <int NQ, int R, int G>
__global__ __launch_bounds__(64) void k_bselect(Params p, int tb) {
  __shared__ __attribute__((aligned(16))) unsigned long long cand[64 * R + 8];
  __shared__ __attribute__((aligned(16))) uint32_t lm[64];
  __shared__ int scratch[128];
  // this beta-iteration's direct-pair list starts empty (k_bkernel appends)
  if (blockIdx.y == 0 && tidx() == 0) p.bdlcount[size_t(p.b0 + blockIdx.x) * kBetaIters + tb] = 0;
  bselect_wave<NQ, R, G>(p, tb, p.b0 + blockIdx.x, blockIdx.y, gridDim.y, cand, lm, scratch);
}

}  // namespace

// one wave per (candidate, tile, chunk): launch_bsample's small batches
void launch_bsample_chunks(const Params& p, int tb, hipStream_t s) {
  const int nblk = pos_pad(p.M) >> 4, cl = sample_chunk(nblk);
  hipLaunchKernelGGL(k_bsample_chunks, dim3(p.nb, kSampleTiles), dim3(64 * ((nblk + cl - 1) / cl)), 0, s, p, tb);
}

void launch_bsel0(const Params& p, hipStream_t s) {
  const size_t total = size_t(p.nb) * (kBetaSamples * p.n + kBetaSamples);
  hipLaunchKernelGGL(k_bsel0, dim3(unsigned(std::min<size_t>((total + 255) / 256, 4096))), dim3(256), 0, s, p);
}

// waves per candidate: ~16 single-wave workgroups per SIMD over the launch,
// at most 16 per candidate (B = 1024: 8 -> 16 measured -8.5%; the 512-candidate
// groups of the two-stream split: 25 -> 16 +1%); small launches (nb <= 128:
// up to Params::sel_cap waves per candidate -- CARLA n = 22, B = 100: 16 -> 64
// took 1.5 ms off a 49.5 ms solve)
int sel_waves(int nb, int cap) { return std::max(4, std::min(nb <= 128 ? cap : 16, 16384 / std::max(1, nb))); }

template <int NQ, int R, int G>
void launch_bselect_i(const Params& p, int tb, hipStream_t s) {
  hipLaunchKernelGGL((k_bselect<NQ, R, G>), dim3(p.nb, sel_waves(p.nb, p.sel_cap)), dim3(64), 0, s, p, tb);
}

// k_bselect<NQ, R, G> by n (betacem_select.hpp): NQ the instantiated keys per
// lane that cover ceil(n^2 / 64); (R, G) = (1, 32) for n <= 24, (2, 64) for
// n <= 48, else (2, 0).  The two follow n together, so these 13 instances are
// all a supported size (n <= 64) reaches.
void launch_bselect(const Params& p, int tb, hipStream_t s) {
  const int n = p.n;
  if (n <= 8) return launch_bselect_i<1, 1, 32>(p, tb, s);
  if (n <= 11) return launch_bselect_i<2, 1, 32>(p, tb, s);
  if (n <= 16) return launch_bselect_i<4, 1, 32>(p, tb, s);
  if (n <= 22) return launch_bselect_i<8, 1, 32>(p, tb, s);
  if (n <= 24) return launch_bselect_i<12, 1, 32>(p, tb, s);
  if (n <= 27) return launch_bselect_i<12, 2, 64>(p, tb, s);
  if (n <= 32) return launch_bselect_i<16, 2, 64>(p, tb, s);
  if (n <= 39) return launch_bselect_i<24, 2, 64>(p, tb, s);
  if (n <= 45) return launch_bselect_i<32, 2, 64>(p, tb, s);
  if (n <= 48) return launch_bselect_i<40, 2, 64>(p, tb, s);
  if (n <= 50) return launch_bselect_i<40, 2, 0>(p, tb, s);
  if (n <= 55) return launch_bselect_i<48, 2, 0>(p, tb, s);
  return launch_bselect_i<64, 2, 0>(p, tb, s);
}

}  // namespace mpcmmd
