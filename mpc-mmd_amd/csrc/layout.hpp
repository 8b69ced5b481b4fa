// Sizes and index functions of the device buffers that host-only code needs
// as well (solve_host.cpp): no HIP include.  kernels.hpp includes this.
#pragma once
#include <cstddef>

#ifdef __HIPCC__
#define HDI_CONST __host__ __device__ __forceinline__ constexpr
#else
#define HDI_CONST inline constexpr
#endif

namespace mpcmmd {

constexpr int kMaxH = 100;
constexpr int kMaxReduced = 64;        // n for mmd_opt (M = n^2 <= 4096) -- see DESIGN.md
constexpr int kBetaSamples = 100;      // compute_beta.py:14
constexpr int kBetaIters = 20;         // compute_beta.py:15
constexpr int kBetaElite = 11;         // compute_beta.py:26
constexpr int kEliteCost = 20;         // cem.py:140
constexpr int kCnormStride = 12;       // doubles per candidate of Params::cnorm (11 norms)
constexpr int kElite = 5;              // cem.py:138
constexpr int kResultStride = 11 + 11 + 2 + 1 + 20 + kMaxReduced;  // cx, cy, lane, obs, sigma, res_beta, beta
// generators per candidate: a W plane of pos_pad(M) rows x kGenRow doubles
// (features 0..10, slot 11 zero), L_jj in Params::genm, and the U rows
// (features u_0..u_10, the position's fp32-rounded elite mean in slot 11).
// The U rows are not stored: u_e of a position is the elite row E_e
// (Params::belite, fp32, row stride M + 1) re-encoded against the position's
// fp64 elite mean m, and every user forms it with gen_u / gen_mean_slot below
// (one expression, so one set of bits).  k_belite writes the means to the
// first pos_pad(M) doubles after the W plane (gen_means; padding positions
// keep the allocation's 0).  The rest of that second plane of the candidate's
// kGenStride doubles per position -- it held the U rows -- is neither written
// nor read: the allocation keeps its size only because the buffer sizes are
// pinned.  The sampler feeds slot 11 through the 16x16x4 MFMA
// operands unmasked: W's zero slot keeps the mean out of W U^T, and row 11 of
// its S_pre is 1, so U S adds the mean.
constexpr int kGenRow = 12;
constexpr int kGenStride = 2 * kGenRow;  // doubles per position and candidate
constexpr int kGenW = 0, kGenMean = 11;
HDI_CONST size_t gen_means(int Pp) { return size_t(Pp) * kGenRow; }  // offset of the means: [pos_pad(M)] fp64
constexpr double kRsqrt10 = 0x1.43d136248490fp-2;  // 1.0 / sqrt(10.0) in fp64 arithmetic (jnp.cov's 1 / (11 - 1))
// u_e of a position from its elite value and mean; slot 11 of the U row
HDI_CONST double gen_u(float e, double m) { return (double(e) - m) * kRsqrt10; }
HDI_CONST double gen_mean_slot(double m) { return double(float(m)); }
HDI_CONST int ygen_stride(int M) { return ((M + 1) + 31) & ~31; }
// beta-CEM sample generation works on pairs of blocks of 16 positions and
// tiles of 16 samples: generators (gen, genm) and the device normals (beta_z)
// are padded with zeros to pos_pad(M) positions, beta_z rows and ygen to
// kBzCols samples
constexpr int kBzCols = 96;
// beta_z device layout per iteration: blocks of 16 positions x kBzCols
// samples, each block the sampler's lane image [6 chunks][64 lanes][4 floats]:
// lane r + 16 h holds positions p0 + 4 k + h (k < 4) of samples 32 u + 2 r + e
// (u < 3, e < 2) at index 6 k + 2 u + e, so a wave reads a block's normals in
// six fully coalesced float4 loads
HDI_CONST size_t bz_index(int j, int s) {
  const int jj = j & 15, lane = ((s & 31) >> 1) + 16 * (jj & 3), idx = 6 * (jj >> 2) + 2 * (s >> 5) + (s & 1);
  return size_t(j >> 4) * (16 * kBzCols) + (idx >> 2) * 256 + lane * 4 + (idx & 3);
}
HDI_CONST int pos_pad(int M) { return ((M + 1) + 31) & ~31; }  // whole pairs of 16-blocks
// row stride (floats) of the mother distance matrix: whole 256-column blocks
// (k_bkernel: a wave holds a row as one float4 per lane and block); pad
// columns hold +inf
HDI_CONST int dist_stride(int M) { return (M + 255) & ~255; }
// floats per sample of Params::bkred: the n (n - 1) / 2 strict lower triangle
// rounded to whole 16-byte groups (the QP kernel stages rows as float4)
HDI_CONST int tri_stride(int n) { return ((n * (n - 1) / 2) + 3) & ~3; }
// floats per mother row of Params::featr (22 features, 2 zero pads: six float4)
constexpr int kFeatStride = 24;
// series record of a distance row (Params::bmom, k_bmoment): P_0..P_11, R, pad
constexpr int kMom = 12;
constexpr int kMomStride = 16;
constexpr int kMomR = 12;
// doubles per configuration of Params::gtab
HDI_CONST size_t gtab_stride(int S, int H) { return size_t(4) * 4 * 4 * S * H; }  // == gamma_tab_size (rng.hpp)
constexpr int kMaxSplit = 8;  // workgroups per candidate of the row-sum kernels
constexpr int kMaxPath = 2048;  // CARLA path points (the reference's num_path = 600)
constexpr int kMaxDetObs = 32;  // obstacles of compute_cem_det (k_front's per-lane non-finite mask: 2 bits each)

}  // namespace mpcmmd
