// Stage "risk" for cost = mmd_opt: the mother rollouts, their Bernstein fit
// and the nested beta-CEM that picks the reduced set and the MMD weights,
// then the reduced-set MMD.  Per outer iteration:
//
//   k_mother    noisy control rows, n^2 mother rollouts (Cartesian product,
//               cem_helper.py:469-530) with the ridge fit folded into the scan
//               (compute_coeff, cem_helper.py:553-564) -> 22 features per row
//   k_bdist     the M x M L1 distance matrix of the features (once)
//   20 x { k_bsample  new samples of the beta-CEM (compute_beta.py:51-68)
//          k_bselect  top-n |beta| rows and sigma per sample (compute_beta.py:41-49, 117-118)
//          k_bkernel  Laplace-kernel row sums over the mother set and K_red
//                     (kernel_computation.py:19-65, compute_beta.py:120-127)
//          k_bqp      the equality-constrained QP and its cost per sample
//                     (compute_beta.py:70-91, 129)
//          k_belite   elite 11, mean, structured Cholesky of
//                     cov = D D^T / 10 + 0.05 I, next generators (compute_beta.py:51-68, 133-145) }
//   k_mmdfinal  reduced-set rollouts, collision residual, MMD obs / lane
//               (costs.py:121-135, 173-186)
//
// The beta-iteration kernels work on a candidate range [p.b0, p.b0 + p.nb):
// the host splits the batch into groups, each on its own stream, so the
// kernels of different groups (bound by different units: MFMA, exp, fp64
// FMA latency, LDS) run side by side.  Every supported size n <= 64
// (M = n^2 <= 4096) takes these per-iteration kernels, their LDS-resident
// pieces sized at launch (ker_lds, dir_lds, elite_lds) -- except handles of
// <= 512 candidates at n <= 16 (M <= 256), whose 20 beta-iterations run in one
// launch of the fused k_bcem_small (bcem_small_ok), the same phase bodies.
//
// The covariance of the beta-CEM is rank <= 10 plus 0.05 I
// (jnp.cov of 11 elites, compute_beta.py:61).  Its Cholesky factor is never
// formed: with U = (E - mean)^T / sqrt(10), Phi_j = I + U_{<j}^T U_{<j} / d,
// v_j = Phi_j^-1 u_j, L_jj = sqrt(d + u_j.v_j), w_j = v_j / L_jj, one has
// L_ij = u_i . w_j (i > j), so (L z)_i = L_ii z_i + u_i . sum_{j<i} w_j z_j.
// Same factor as chol(cov) in exact arithmetic, O(M r^2) instead of O(M^3).
//
// This header: what every beta-CEM file shares (the thread index, sizes,
// launch sizing, the LDS layouts; the wave / quad helpers are lanes.hpp's).
// The phase bodies that both the per-iteration kernels and the fused
// k_bcem_small run are in betacem_{sample,select,kernel,qp,elite}.hpp; the
// kernels and their
// launchers in k_mother, k_bdist, k_bsample, k_bkernel, k_bqp, k_belite and
// k_bcem_small.hip.
#pragma once
#include <type_traits>

#include "block.hpp"
#include "kernels.hpp"

namespace mpcmmd {

namespace {

// The thread's index.  The small-batch fused kernel (k_bcem_small.hip, which
// alone defines MPCMMD_OPAQUE_TIDX before its includes) runs every phase
// inside one loop over the beta-iterations; there each read is opaque, so
// nothing computed from the index is hoisted out of the loop and held in
// registers across the other phases (spills).  The per-iteration kernels read
// threadIdx.x.  This is the one thing that differs between the phase bodies
// as the fused kernel and as the per-iteration kernels compile them.
#ifdef MPCMMD_OPAQUE_TIDX
DEVI unsigned tidx() {
  unsigned t = threadIdx.x;
  asm volatile("" : "+v"(t));
  return t;
}
#else
DEVI unsigned tidx() { return threadIdx.x; }
#endif

constexpr int kF = 22;                               // features: cx (11) | cy (11)
constexpr int kNew = kBetaSamples - kBetaElite;      // 89 resampled rows per iteration
constexpr int kThreads = 512;
constexpr double kSqrt20 = 4.47213595499957927704;   // chol(20 I) (compute_beta.py:24)
constexpr double kRidge = 0.05;                      // cov jitter (compute_beta.py:61)
constexpr double kInvRidge = 20.0;

// first sample a beta-iteration processes: from the second iteration on,
// samples 0..10 are the previous iteration's elites, unchanged, and k_belite
// carries their top-n rows, sigma, QP solution and cost
HDI int first_sample(int tb) { return tb > 0 ? kBetaElite : 0; }

// The elite rows [11][M + 1] (fp32) and position means [pos_pad(M)] (fp64)
// that candidate b's generators re-encode (layout.hpp: gen_u): k_belite of
// beta-iteration t writes half (t + 1) & 1 of Params::belite, which k_bgen /
// k_bsigma of iteration t and the sampler of iteration t + 1 read -- `half`
// is t + 1 for all three.
DEVI const float* gen_elites(const Params& p, int half, int b) {
  return p.belite + (size_t(half & 1) * p.Bt + b) * kBetaElite * (p.M + 1);
}
DEVI const double* gen_mean_row(const Params& p, int b) {
  return p.gen + size_t(b) * pos_pad(p.M) * kGenStride + gen_means(pos_pad(p.M));
}

// raw buffer loads: lane offset (bytes) in a VGPR, wave-uniform offset in an
// SGPR; out of range returns 0
DEVI float buf_ld_f(__amdgpu_buffer_rsrc_t rs, int voff, int soff) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, voff, soff, 0));
}
DEVI double buf_ld_d(__amdgpu_buffer_rsrc_t rs, int voff, int soff) {
  return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(rs, voff, soff, 0));
}

#define kconst __attribute__((address_space(4)))
typedef float f2 __attribute__((ext_vector_type(2)));

// fp64 MFMA (v_mfma_f64_16x16x4_f64; layouts: betacem_sample.hpp)
typedef double d4 __attribute__((ext_vector_type(4)));
DEVI d4 mfma64(double a, double b, d4 c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }

// launch sizing
constexpr int kXcds = 8;   // workgroups are dealt round-robin to the 8 XCDs by linear id
constexpr int kCUs = 256;  // MI355X compute units (launch sizing only)
constexpr int kKerWaves = 16;  // waves per k_bkernel workgroup (and of k_bcem_small, which runs its body)
constexpr int kDirWaves = 4;   // waves per k_bdirect / k_bdirect_pairs workgroup
constexpr int kLptBins = 128;  // pair counts per distinct row (<= 100 samples)
// the series of a K_mixed row sum (k_bmoment's records, summed by k_bkernel)
// covers a = R / sigma <= kSeriesAMax: k_bmoment's error bound holds for a <= 1
constexpr double kSeriesAMax = 1.0;
constexpr float kNegLog2e = -1.44269504088896340736f;
constexpr size_t kLdsBudget = 160 * 1024 - 1024;

// Host dispatch on the float4s a lane holds of a distance row, V =
// dist_stride(M) / 256 (one per 256-column block): calls f with
// std::integral_constant<int, V>, V = 1..16, so a launcher picks its kernel
// instance by f's argument type.  M <= 4096 (kMaxReduced^2) keeps V <= 16;
// anything else takes 16.
template <int V = 1, class F>
void with_dist_blocks(int M, F&& f) {
  if constexpr (V == 16) {
    f(std::integral_constant<int, 16>{});
  } else {
    if ((dist_stride(M) >> 8) == V) f(std::integral_constant<int, V>{});
    else with_dist_blocks<V + 1>(M, f);
  }
}

struct LdsTake {  // consecutive 16-byte aligned LDS pieces
  size_t o = 0;
  HDI size_t operator()(size_t bytes) {
    const size_t at = o;
    o = (o + bytes + 15) & ~size_t(15);
    return at;
  }
};

// k_bkernel LDS.  persistent: sel (short; union ranks once the records are
// staged), -log2 e / sigma, 1 / sigma, the entry table (k | kk << 8), union
// rank of a row, row of a rank; scratch (`scratch` bytes, chosen at launch):
// the union flags, then the union's series records, then the distance table
// and the union's feature rows, or the waves' per-sample feature rows (or
// the union's feature rows alone: MPCMMD_KER_PATH=1)
struct KerLds {
  size_t sel, csg, csd, tri, urank, urow, misc, scratch, total;
};
HDI KerLds ker_lds(int M, int n, size_t scratch) {
  KerLds L{};
  LdsTake take;
  L.sel = take(size_t(kBetaSamples) * n * 2);
  L.csg = take(size_t(kBetaSamples) * 4);
  L.csd = take(size_t(kBetaSamples) * 8);
  L.tri = take(size_t(n) * (n - 1));
  L.urank = take(size_t(M) * 2);
  L.urow = take(size_t(M) * 2);
  L.misc = take(32 * 4);  // [0] union rows, [1] series pairs, [2] direct pairs, [16..] wave totals
  L.scratch = take(scratch);
  L.total = take.o;
  return L;
}
// floats per feature row staged for K_red outside the table (the waves'
// per-sample slices, the union image): 7 float4s, not kFeatStride's 6.  A
// ds_read_b128 is served per 16-lane group from sixteen 16-byte bank slots; the
// lanes of a group read rows kk, kk + 1, .. of the slice, and at an odd pitch
// those start in distinct slots (at 6 float4s rows kk and kk + 8 share one: every
// second-row read ran 2-way conflicted)
constexpr int kKerRowPitch = 28;
HDI size_t ker_sample_bytes(int n) { return size_t(kKerWaves) * n * kKerRowPitch * 4; }
HDI size_t ker_tab_bytes(int U) { return ((size_t(U) * (U - 1) / 2 * 4 + 15) & ~size_t(15)) + size_t(U) * kFeatStride * 4; }
// the union table's LDS budget: what two workgroups per CU (160 KB, less
// allocation slack) leave after the persistent pieces, between 55 KB (unions
// of <= 144 rows; every size gets it, as before) and 71 KB (<= 165 rows: n = 22,
// where 64% of the candidates of beta-iteration 4 have 145..165 rows)
constexpr size_t kKerTabBytes = 55 * 1024, kKerTabMax = 71 * 1024, kKerHalfLds = 79 * 1024;
HDI size_t ker_tab_budget(int M, int n) {
  const size_t fixed = ker_lds(M, n, 0).total;
  const size_t left = kKerHalfLds > fixed ? (kKerHalfLds - fixed) & ~size_t(15) : 0;
  return left < kKerTabBytes ? kKerTabBytes : (left > kKerTabMax ? kKerTabMax : left);
}
// scratch: the series records of every mother row (up to kKerRecBytes;
// larger unions read them from global memory), and the union table (its
// budget) from the second beta-iteration on (the first one's 100 fresh
// samples select nearly every mother row).  MPCMMD_KER_PATH=1 launches the
// first iteration with that size too, for the image of its union.  `tab`:
// k_bkernel passes ker_tab_budget; k_bcem_small keeps the 55 KB (the larger
// budget cost CARLA n = 10 1% in three of three alternated runs)
constexpr size_t kKerRecBytes = 64 * 1024;
HDI size_t ker_scratch(int M, int n, int tb, size_t tab = kKerTabBytes) {
  size_t sc = ker_sample_bytes(n);
  size_t rec = size_t(M) * kMomStride * 4;
  if (rec > kKerRecBytes) rec = kKerRecBytes;
  if (rec > sc) sc = rec;
  if (tb > 0 && tab > sc) sc = tab;
  return sc;
}

// k_bdirect LDS.  persistent: sel (short), -log2 e / sigma, the direct pairs
// sorted by row, the distinct direct rows and their first pair, the grab
// order; scratch: the setup's counts / fill / scan (10 M bytes)
struct DirLds {
  size_t sel, csg, pairs, ulist, ustart, order, bins, misc, scratch, total;
};
HDI DirLds dir_lds(int M, int n) {
  DirLds L{};
  LdsTake take;
  L.sel = take(size_t(kBetaSamples) * n * 2);
  L.csg = take(size_t(kBetaSamples) * 4);
  L.pairs = take(size_t(kBetaSamples) * n * 2);
  L.ulist = take(size_t(M) * 2);
  L.ustart = take(size_t(M + 1) * 2);
  L.order = take(size_t(M) * 2);
  L.bins = take(kLptBins * 4);
  L.misc = take(32 * 4);  // [0] next row, [1] distinct rows, [16..] wave totals
  L.scratch = take(size_t(M) * 10);
  L.total = take.o;
  return L;
}

// k_belite LDS: the block sums (nblk x 66 fp64), small bookkeeping, the
// carried elite rows and a 16-position u staging per wave
struct EliteLds {
  size_t Gb, misc, carry, ublk, total;
};
constexpr int kUPitch = 12;  // doubles per position row of the per-wave u staging
HDI EliteLds elite_lds(int M1, int waves = kThreads / 64) {
  EliteLds L{};
  const int nblk = (M1 + 15) / 16;
  L.Gb = 0;
  L.misc = (size_t(nblk) * 66 * 8 + 15) & ~size_t(15);
  L.carry = L.misc + 1024;
  L.ublk = (L.carry + size_t(kBetaElite) * (2 * kMaxReduced + 2) * 4 + 15) & ~size_t(15);
  L.total = L.ublk + size_t(waves) * 16 * kUPitch * 8;  // one 16-position block per wave
  return L;
}

// the fused kernel's sampler: an LDS copy of the candidate's generators
// ([W plane][U rows: pos_pad(M) x kGenRow, formed in place][genm]) and every
// block's T (betacem_sample.hpp: bsample_tblocks)
HDI size_t lds_uplane(int Pp) { return size_t(Pp) * kGenRow; }  // doubles from the W plane to the U rows
HDI size_t gen_lds_bytes(int M) { return size_t(pos_pad(M)) * (2 * kGenRow + 1) * 8 + 16 * 8; }  // + wA's overreach
HDI size_t tblk_lds_bytes(int M) { return size_t(pos_pad(M) >> 4) * 4 * 64 * 8; }

}  // namespace

}  // namespace mpcmmd
