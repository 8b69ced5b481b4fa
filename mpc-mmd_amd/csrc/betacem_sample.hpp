// The beta-CEM sampler's device code (k_bsample_walk.hip, k_bsample.hip,
// k_bcem_small.hip).
//
// k_bsample: the new samples of beta-CEM iteration tb >= 1 (rows 11..99,
// mean + L z, compute_beta.py:51-68) with the structured factor of
// betacem_common.hpp's header, as fp64 MFMA (v_mfma_f64_16x16x4_f64) over
// blocks of 16 positions:
//
//   Y_c = m_c + T_c Z_c + U_c S_c,   S_{c+1} = S_c + W_c^T Z_c
//
// Z_c [16 positions x 16 samples] the normals, S_c [11 x 16] the prefix
// sum_{j < 16c} w_j z_j, U_c / W_c [16 x 11] the generators u_j / w_j and
// T_c [16 x 16] = strict_lower(U_c W_c^T) + diag(L_jj) (itself one MFMA
// product, masked).  A wave owns kTilesPerWave tiles of 16 samples and walks
// the blocks in order; S stays in the registers its MFMAs accumulate in and
// is, by the 16x16x4 f64 layouts, directly the B operand of U_c S_c.  All in
// fp64 (the oracle's dense fp64 Cholesky agrees to ~1e-15 before the fp32
// rounding).
//
// f64 16x16x4 layouts (lane l, r = l & 15, h = l >> 4):
//   A: A[r][h]   B: B[h][r]   C/D register i: C[h + 4 i][r]
#pragma once
#include <type_traits>

#include "betacem_common.hpp"

namespace mpcmmd {

namespace {

constexpr int kSampleTiles = kBzCols / 16;  // 6 tiles of 16 sample columns (89 used)
static_assert(kBzCols >= kNew, "sample tiles");
// TPW = sample tiles per wave: 6 (one wave per candidate: the generator
// operands loaded once) when the batch fills the chip; small batches -- the
// reference's num_batch = 100 -- take k_bsample_chunks (one tile per wave,
// the blocks split into chunks walked in parallel).
//
// The prefix is kept as S = S_pre + S_loc: S_loc accumulates W^T Z from zero
// within a chunk of sample_chunk(nblk) blocks and is folded into S_pre at the
// chunk's end.  The chunking depends only on M, so one wave walking every
// chunk (k_bsample) and one wave per chunk (k_bsample_chunks, S_pre from the
// earlier chunks' sums) compute the same bits: a configuration's samples do
// not depend on the batch it is solved in.
constexpr int kChunkWavesMax = 12;
HDI int sample_chunk(int nblk) {
  int cl = nblk <= 8 ? 4 : 8;  // two chunks at M = 100 (k_bcem_small walks them in parallel)
  while ((nblk + cl - 1) / cl > kChunkWavesMax) cl <<= 1;
  return cl;
}
// The blocks every sampler walks: those that hold a position 0..M.  The
// chunking stays that of the padded count pos_pad(M) / 16 (a pair of blocks
// more at most, pure padding: W^T Z of zeros into sums nothing reads).
HDI int sample_blocks(int M) { return (M + 1 + 15) >> 4; }
template <int TPW>
constexpr int sample_waves() {
  static_assert(kSampleTiles % TPW == 0, "tiles per wave");
  return kSampleTiles / TPW;
}

// Operands of one block, loaded unconditionally (generators and normals are
// zero padded to whole blocks and tiles), so the loop has no branches and the
// compiler can count outstanding loads exactly.  Generators (k_belite,
// k_bgen; layout.hpp): W plane = w_0..w_10 and a zero slot 11, genm = L_jj,
// and the U row u_0..u_10 with the position's mean in slot 11, which
// block_u forms from the elite rows' fp32 values and the fp64 mean.  With
// row 11 of S_pre held at 1 (and row 11 of S_loc exactly 0, W's slot 11 being
// 0), U S carries the mean as its twelfth term: no mean operand, no
// accumulator initialisation.
template <int TPW>
struct SampleBlock {
  double wA[4];  // W[p0 + 4k + h][r]        (A of W^T Z; r = feature)
  double wX[3];  // W[p0 + r][4i + h]        (A of W U^T; 4i + h = feature)
  float eX[3];   // E[4i + h][p0 + r]        (the elite value of U[p0 + r][4i + h]; feature 11: unused)
  double m;      // elite mean of position p0 + r (0 at padding positions)
  double L;      // L_jj of position p0 + r
  float z[TPW][4];   // Z[p0 + 4k + h][sample of (tile t, lane r)] (sample_of); fp32 normals, widened at use
};

// U[p0 + r][4i + h] of a loaded block (B of W U^T, A of U S; feature 11 =
// the mean).  TAIL: the block may hold positions past the sigma coordinate
// (valid = p0 + r <= M), whose u is 0 as their mean is: the elite rows are
// not padded, so there eX holds some other value.
template <bool TAIL, int TPW>
DEVI void block_u(const SampleBlock<TPW>& q, double (&uX)[3], int h, bool valid) {
#pragma unroll
  for (int i = 0; i < 3; ++i) uX[i] = gen_u(TAIL && !valid ? 0.0f : q.eX[i], q.m);
  uX[2] = h == 3 ? gen_mean_slot(q.m) : uX[2];
}

// E: the candidate's elite rows (gen_elites), mrow its means (gen_mean_row)
template <int TPW>
DEVI void load_block(SampleBlock<TPW>& q, const double* G, const float* E, const double* mrow, const double* gm,
                     const float* z, int M, int p0, int s0, int r, int h) {
#pragma unroll
  for (int k = 0; k < 4; ++k) q.wA[k] = G[size_t(p0 + 4 * k + h) * kGenRow + kGenW + r];  // rows > 11 of S unused
  const double* g = G + size_t(p0 + r) * kGenRow;
  const float* e = E + min(p0 + r, M);  // clamped into the rows, as the feature below (block_u masks both)
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    q.wX[i] = g[kGenW + 4 * i + h];  // W's zero slot 11 times U's mean: X gets no mean term
    q.eX[i] = e[size_t(min(4 * i + h, kBetaElite - 1)) * (M + 1)];
  }
  q.m = mrow[p0 + r];
  q.L = gm[p0 + r];
  // tiles in pairs: lane r of tiles 2u, 2u + 1 takes samples 32u + 2r, 32u +
  // 2r + 1 -- the lane image of bz_index, six float4 loads per block (one
  // tile per wave: lane r takes sample s0 + r, scalar loads)
  static_assert(TPW == 1 || TPW == kSampleTiles, "tile pairing of the normals' layout");
  if constexpr (TPW == 1) {
#pragma unroll
    for (int k = 0; k < 4; ++k) q.z[0][k] = z[bz_index(p0 + 4 * k + h, s0 + r)];
  } else {
    const float4* zb = reinterpret_cast<const float4*>(z + size_t(p0 >> 4) * (16 * kBzCols)) + r + 16 * h;
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      const float4 f = zb[64 * c];
      const float fv[4] = {f.x, f.y, f.z, f.w};
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const int idx = 4 * c + w, k = idx / 6, t = idx % 6;  // t = 2 u + e
        q.z[t][k] = fv[w];
      }
    }
  }
}

// load_block<kSampleTiles> as raw buffer loads: the lane parts of the offsets
// are fixed for the launch (four VGPRs), the block part p0 goes in SGPRs, so
// a block's 17 loads need no per-lane address arithmetic and no 64-bit
// address registers (the walker runs at 1 wave per SIMD, where every VALU
// instruction and register counts).  Same addresses as load_block.
// The elite rows' buffer ends with row 10: feature 11's load (lanes h = 3 of
// i = 2) and a padding position's in row 10 are out of range and return 0; a
// padding position's in the rows before reads the next row (block_u's mask).
struct SampleRsrc {
  __amdgpu_buffer_rsrc_t gen, genm, z, el;
  int vA, vX, vL, vZ, vE;  // lane offsets (bytes): W^T rows, W rows, L_jj / mean, normals, elite values
  int means;               // bytes from the W plane to the means
  int erow;                // bytes of four elite rows (features 4i + h -> 4(i + 1) + h)
};
DEVI SampleRsrc sample_rsrc(const double* G, const float* E, const double* gm, const float* z, int M, int r, int h) {
  SampleRsrc s;
  const int Pp = pos_pad(M);
  s.gen = __builtin_amdgcn_make_buffer_rsrc(const_cast<double*>(G), short(0), Pp * kGenStride * 8, 0x00020000);
  s.el = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(E), short(0), kBetaElite * (M + 1) * 4, 0x00020000);
  s.genm = __builtin_amdgcn_make_buffer_rsrc(const_cast<double*>(gm), short(0), Pp * 8, 0x00020000);
  s.z = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(z), short(0), Pp * kBzCols * 4, 0x00020000);
  s.vA = (h * kGenRow + kGenW + r) * 8;
  s.vX = (r * kGenRow + h) * 8;
  s.vL = r * 8;
  s.vZ = (r + 16 * h) * 16;
  s.vE = (h * (M + 1) + r) * 4;
  s.means = int(gen_means(Pp)) * 8;
  s.erow = 4 * (M + 1) * 4;
  return s;
}
DEVI void load_block_buf(SampleBlock<kSampleTiles>& q, const SampleRsrc& s, int p0) {
  const int sg = p0 * kGenRow * 8;
#pragma unroll
  for (int k = 0; k < 4; ++k) q.wA[k] = buf_ld_d(s.gen, s.vA + k * 4 * kGenRow * 8, sg);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    q.wX[i] = buf_ld_d(s.gen, s.vX + 32 * i, sg);
    q.eX[i] = buf_ld_f(s.el, s.vE, p0 * 4 + i * s.erow);
  }
  q.m = buf_ld_d(s.gen, s.vL, p0 * 8 + s.means);
  q.L = buf_ld_d(s.genm, s.vL, p0 * 8);
  const int szz = (p0 >> 4) * (16 * kBzCols * 4);
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    typedef float v4f __attribute__((ext_vector_type(4)));
    const v4f f = __builtin_bit_cast(v4f, __builtin_amdgcn_raw_buffer_load_b128(s.z, s.vZ + 1024 * (c % 3), szz + 3072 * (c / 3), 0));
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int idx = 4 * c + w, k = idx / 6, t = idx % 6;
      q.z[t][k] = f[w];
    }
  }
}

// One block's MFMAs for the wave's tiles, all accumulating in place:
//   Y  = U S              (3 per tile from a zero C operand; the mean is
//                          U's feature 11 times row 11 of S_pre, which is 1)
//   S += W^T Z            (4 per tile; after U S has read S)
//   Y += T Z              (4 per tile; T from X = W U^T, built meanwhile)
// The Y products are formed transposed, Y^T = S^T U^T + Z^T T^T (the same
// operand registers with A and B exchanged), so register i of lane (r, h)
// holds sample row h + 4i of the tile at position p0 + r: a store covers
// four sample rows x 16 consecutive positions, no transpose before it.
// Tiles are interleaved, so every accumulator chain has 6 MFMAs between
// dependent steps.  No VALU work on the accumulators: the pipe never waits
// for a vector add between blocks.
template <bool TAIL = false, int TPW>
DEVI void block_mfma(const SampleBlock<TPW>& cur, d4* S, const d4* Sp, d4* Y, int r, int h, bool valid = true) {
  double uX[3];
  block_u<TAIL>(cur, uX, h, valid);
  double zd[TPW][4];  // the fp32 normals widened once (exact), used by two MFMA chains
#pragma unroll
  for (int t = 0; t < TPW; ++t)
#pragma unroll
    for (int k = 0; k < 4; ++k) zd[t][k] = double(cur.z[t][k]);
  d4 X = d4{0.0, 0.0, 0.0, 0.0};  // X = W_c U_c^T: register i holds w_{h+4i} . u_r = T[row r][col h + 4i]
#pragma unroll
  for (int i = 0; i < 3; ++i) X = mfma64(cur.wX[i], uX[i], X);
  const d4 zero = d4{0.0, 0.0, 0.0, 0.0};
  // B operand of U S: S_pre + S_loc (rows 0..11 of S: registers 0..2)
  double St[TPW][3];
#pragma unroll
  for (int t = 0; t < TPW; ++t)
#pragma unroll
    for (int k = 0; k < 3; ++k) St[t][k] = Sp[t][k] + S[t][k];
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int t = 0; t < TPW; ++t) Y[t] = mfma64(St[t][k], uX[k], k == 0 ? zero : Y[t]);
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int t = 0; t < TPW; ++t) S[t] = mfma64(cur.wA[k], zd[t][k], S[t]);
  double T[4];  // B operand of (T Z)^T, k-step i: T[r][4i + h]
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int k = h + 4 * i;
    T[i] = k < r ? X[i] : (k == r ? cur.L : 0.0);
  }
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int t = 0; t < TPW; ++t) Y[t] = mfma64(zd[t][k], T[k], Y[t]);
}

// the finished block's samples to fp32 (the sigma coordinate M clipped).
// Lane (r, h), register i of tile t: sample row rho = h + 4i of the tile
// (sample s0 + rho for one tile per wave; 32 (t / 2) + 2 rho + t % 2 for the
// paired tiles of the one-wave walker), position p0 + r; per store, four
// sample rows x 64 contiguous bytes.  Blocks wholly past the sigma coordinate
// and the padding samples >= kNew are not stored (k_bselect never reads them).
HDI_CONST int tile_sample(int TPW, int s0, int t, int rho) { return TPW == 1 ? s0 + rho : 32 * (t >> 1) + 2 * rho + (t & 1); }
template <int TPW>
DEVI void block_store(const d4* Yv, float* plane, int p0, int M, int ys, int s0, int r, int h) {
  if (p0 > M) return;
#pragma unroll
  for (int t = 0; t < TPW; ++t)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int s = tile_sample(TPW, s0, t, h + 4 * i);
      const float v = float(Yv[t][i]);
      if (s < kNew) plane[size_t(s) * ys + p0 + r] = p0 + r == M ? fmaxf(v, 0.01f) : v;
    }
}

// k_bsample's store of a finished block that does not hold the sigma
// coordinate M: block_store<kSampleTiles> without the clip's selects and
// without per-block address arithmetic (on gfx950 a wave's VALU work does not
// run in the shadow of its fp64 MFMAs -- tools/mfma_overlap.hip: +6..8
// clocks per VALU instruction between MFMAs).  Raw buffer stores over the
// candidate's sample plane: the lane part of the offset (vl = row 2h,
// position r) is fixed for the launch, the block, tile and register parts go
// in an SGPR.  Tiles 0-3 hold real samples only; in tiles 4 and 5 register 3
// holds samples 88 + 2h + t % 2 >= kNew but for (t = 4, h = 0) -- that store
// takes v43, out of range (dropped by the buffer unit) for h > 0, and tile
// 5's register 3 is not stored.
// The stores are non-temporal (kStoreNt, the buffer instructions' nt bit): a
// launch streams 89 rows x M + 1 floats per candidate (177 MB at B = 1024,
// n = 22) that nothing reads before k_bselect, so their lines are marked for
// early eviction and do not displace what the sampler itself and the other
// candidate group's kernels, which run beside it, keep in L2.  A cache policy
// only: the bytes written are the same.
constexpr int kStoreNt = 2;
DEVI __amdgpu_buffer_rsrc_t ygen_rsrc(float* plane, int ys) {
  return __builtin_amdgcn_make_buffer_rsrc(plane, short(0), kBzCols * ys * 4, 0x00020000);
}
constexpr int kDropOffset = 0x7FFFFF00;  // out of range for any plane
static_assert(kNew == 89, "tile 4 / 5 register 3 validity below");
DEVI void block_store_rows(const d4* Yv, __amdgpu_buffer_rsrc_t yr, int p0, int ys, int vl, int v43) {
#pragma unroll
  for (int t = 0; t < kSampleTiles; ++t)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (t == 5 && i == 3) continue;
      const int soff = ((32 * (t >> 1) + (t & 1) + 8 * i) * ys + p0) * 4;
      __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(float(Yv[t][i])), yr, t == 4 && i == 3 ? v43 : vl, soff, kStoreNt);
    }
}

// S_pre += S_loc, S_loc = 0 (a chunk's end)
DEVI void fold_chunk(d4& Sp, d4& S) {
#pragma unroll
  for (int k = 0; k < 3; ++k) Sp[k] = Sp[k] + S[k];
  S = d4{0.0, 0.0, 0.0, 0.0};
}

// Blocks [c0, c1) (c1 > c0) in order on the calling wave, c1 - 1 the last
// block a caller walks before its sums are dropped.  Blocks in pairs with the
// operands ping-ponged, so the next block's loads are in flight during a
// block's MFMAs (sched barriers keep that order).
// HOLD: a finished block's samples are converted and stored after the next
// block's MFMAs are issued (outputs ping-ponged too), so the wave does not
// wait for its last MFMAs -- k_bsample_chunks, whose one tile per wave makes
// that wait long and the second Y cheap.  The one-wave walker stores a block
// right after its MFMAs, from one Y: with six tiles the wait is short, a
// wave's VALU work does not run in the shadow of its own fp64 MFMAs on gfx950
// anyway (tools/mfma_overlap.hip), and the second Y's 48 registers are the
// difference between a loop with AccVGPR spill moves and one without.
// The pairs stop short of block c1 - 1, which may hold positions past the
// sigma coordinate M: it is peeled, alone or after its unpaired predecessor,
// with block_u's mask.  pair_end(c) follows the second block of the pair that
// starts at c (the walker's chunk folds: chunk lengths are even, so no chunk
// ends inside the peeled blocks but with the walk).
// store(Y, p0, tag) gets a compile-time tag.  InteriorBlock for the blocks
// c < c1 - 1 <= sample_blocks(M) - 1, which lie wholly before the sigma
// coordinate: 16 (sample_blocks(M) - 1) <= M gives p0 + 15 = 16 c + 15 <=
// 16 (sample_blocks(M) - 1) - 1 < M.  EdgeBlock for block c1 - 1, which may
// hold M or positions past it.
using InteriorBlock = std::true_type;
using EdgeBlock = std::false_type;
template <int TPW, bool HOLD, class Load, class Store, class PairEnd>
DEVI void walk_blocks(int c0, int c1, int M, int r, int h, d4* S, const d4* Sp, Load&& load, Store&& store,
                      PairEnd&& pair_end) {
  d4 Y[HOLD ? 2 : 1][TPW];
  d4 *const Ya = Y[0], *const Yb = Y[HOLD ? 1 : 0];
  SampleBlock<TPW> qa, qb;
  const int last = c1 - 1;
  const bool valid = (last << 4) + r <= M;
  // block q0 / 16 < last is finished in Yc: its store, or with HOLD that of the block before it (in Yp)
  auto finished = [&](const d4* Yc, int q0, const d4* Yp, bool prev) {
    if constexpr (!HOLD)
      store(Yc, q0, InteriorBlock{});
    else if (prev)
      store(Yp, q0 - 16, InteriorBlock{});
  };
  load(qa, c0 << 4);
  int c = c0;
  for (; c + 2 <= last; c += 2) {
    const int p0 = c << 4;
    load(qb, p0 + 16);
    __builtin_amdgcn_sched_barrier(0);
    block_mfma(qa, S, Sp, Ya, r, h);
    __builtin_amdgcn_sched_barrier(0);
    finished(Ya, p0, Yb, c > c0);
    __builtin_amdgcn_sched_barrier(0);
    load(qa, p0 + 32);  // <= last
    __builtin_amdgcn_sched_barrier(0);
    block_mfma(qb, S, Sp, Yb, r, h);
    pair_end(c);
    __builtin_amdgcn_sched_barrier(0);
    finished(Yb, p0 + 16, Ya, true);
    __builtin_amdgcn_sched_barrier(0);
  }
  const int p0 = c << 4;
  if (c < last) {  // two blocks left (wave-uniform)
    load(qb, p0 + 16);
    __builtin_amdgcn_sched_barrier(0);
    block_mfma(qa, S, Sp, Ya, r, h);
    __builtin_amdgcn_sched_barrier(0);
    finished(Ya, p0, Yb, c > c0);
    __builtin_amdgcn_sched_barrier(0);
    block_mfma<true>(qb, S, Sp, Yb, r, h, valid);
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (HOLD) store(Ya, p0, InteriorBlock{});
    store(Yb, p0 + 16, EdgeBlock{});
  } else {  // block c1 - 1 alone (a copy of qa into a shared tail costs the walker's loop six spilled registers)
    block_mfma<true>(qa, S, Sp, Ya, r, h, valid);
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (HOLD)
      if (c > c0) store(Yb, p0 - 16, InteriorBlock{});
    store(Ya, p0, EdgeBlock{});
  }
}

// k_bcem_small's sampler, from an LDS copy of the candidate's generators (lg:
// W plane, the U rows' image, genm; its workgroup just wrote them).
// Two passes:
//   bsample_tblocks  every block's T = strict_lower(W U^T) + diag(L_jj) (the
//                    X MFMAs of block_mfma), once per block into LDS (Tl)
//                    instead of once per tile
//   bsample_unit_lds one (tile of 16 samples, chunk of blocks) per wave: the
//                    earlier chunks' W^T Z sums first (S_pre, folded chunk by
//                    chunk as the walker folds), then the chunk's blocks --
//                    so the chunks of a tile run on separate waves
// Per block the operands and MFMAs of block_mfma in its order, so the samples
// are the per-iteration kernels' bits.  The normals (global, shared by every
// candidate) come kZAhead blocks ahead in registers.
constexpr int kZAhead = 4;

DEVI void bsample_tblocks(const Params& p, const double* lg, double* Tl, int w, int W) {
  const int M = p.M, Pp = pos_pad(M), nblk = sample_blocks(M);
  const int lane = tidx() & 63, r = lane & 15, h = lane >> 4;
  for (int blk = w; blk < nblk; blk += W) {
    const int p0 = blk * 16;
    const double* g = lg + size_t(p0 + r) * kGenRow;
    const double* gu = lg + lds_uplane(Pp) + size_t(p0 + r) * kGenRow;
    double wX[3], uX[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      wX[i] = g[kGenW + 4 * i + h];
      uX[i] = gu[4 * i + h];
    }
    const double L = lg[2 * lds_uplane(Pp) + p0 + r];
    d4 X = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int i = 0; i < 3; ++i) X = mfma64(wX[i], uX[i], X);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int k = h + 4 * i;
      Tl[(size_t(blk) * 4 + i) * 64 + lane] = k < r ? X[i] : (k == r ? L : 0.0);
    }
  }
}

DEVI void bsample_unit_lds(const Params& p, int tb, int b, int tile, int chunk, const double* lg, const double* Tl) {
  const int M = p.M, Pp = pos_pad(M), cl = sample_chunk(Pp >> 4);
  const int c0 = chunk * cl, c1 = min(sample_blocks(M), c0 + cl);  // the walker's bound
  const int lane = tidx() & 63, r = lane & 15, h = lane >> 4, s0 = tile * 16;
  const double* LW = lg;
  const double* LU = lg + lds_uplane(Pp);
  const float* z = p.beta_z + size_t(tb - 1) * Pp * kBzCols;
  const int ys = ygen_stride(M);
  float* plane = p.ygen + size_t(b) * kBzCols * ys;
  d4 S = d4{0.0, 0.0, 0.0, 0.0}, Sp = d4{0.0, 0.0, 0.0, 0.0};
  Sp[2] = h == 3 ? 1.0 : 0.0;  // row 11 of S_pre: the mean's coefficient
  auto zload = [&](float (&zz)[4], int c) {
#pragma unroll
    for (int k = 0; k < 4; ++k) zz[k] = z[bz_index(c * 16 + 4 * k + h, s0 + r)];
  };
  float zr[kZAhead][4];
#pragma unroll
  for (int u = 0; u < kZAhead; ++u) zload(zr[u], min(u, c1 - 1));
  const d4 zero = d4{0.0, 0.0, 0.0, 0.0};
  for (int c = 0; c < c1; c += kZAhead) {
#pragma unroll
    for (int u = 0; u < kZAhead; ++u) {
      const int cb = c + u;
      if (cb < c1) {  // wave-uniform
        const int p0 = cb * 16;
        double zd[4], wA[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          zd[k] = double(zr[u][k]);
          wA[k] = LW[size_t(p0 + 4 * k + h) * kGenRow + kGenW + r];
        }
        zload(zr[u], min(cb + kZAhead, c1 - 1));
        if (cb >= c0) {  // the chunk's block: Y = U S + T Z (block_mfma)
          double uX[3], T[4];
#pragma unroll
          for (int i = 0; i < 3; ++i) uX[i] = LU[size_t(p0 + r) * kGenRow + 4 * i + h];
#pragma unroll
          for (int i = 0; i < 4; ++i) T[i] = Tl[(size_t(cb) * 4 + i) * 64 + lane];
          double St[3];
#pragma unroll
          for (int k = 0; k < 3; ++k) St[k] = Sp[k] + S[k];
          d4 Y = zero;
#pragma unroll
          for (int k = 0; k < 3; ++k) Y = mfma64(St[k], uX[k], k == 0 ? zero : Y);
#pragma unroll
          for (int k = 0; k < 4; ++k) S = mfma64(wA[k], zd[k], S);
#pragma unroll
          for (int k = 0; k < 4; ++k) Y = mfma64(zd[k], T[k], Y);
          block_store<1>(&Y, plane, p0, M, ys, s0, r, h);
        } else {  // an earlier chunk's block: its W^T Z into S_loc only
#pragma unroll
          for (int k = 0; k < 4; ++k) S = mfma64(wA[k], zd[k], S);
        }
        if ((cb + 1) % cl == 0) fold_chunk(Sp, S);  // the walker's fold after a chunk's last block
      }
    }
  }
}

}  // namespace

}  // namespace mpcmmd
