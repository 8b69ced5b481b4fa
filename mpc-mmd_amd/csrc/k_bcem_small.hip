// k_bcem_small, the small-batch fused beta-CEM kernel: the 20 beta-iterations
// of a candidate in one workgroup.  The phase bodies are the per-iteration
// kernels' (the betacem_*.hpp headers), compiled here with the thread index
// read opaquely (tidx, betacem_common.hpp) so that the loop over
// beta-iterations does not keep index arithmetic of every phase live across
// the others.
#define MPCMMD_OPAQUE_TIDX 1
#include "betacem_elite.hpp"
#include "betacem_kernel.hpp"
#include "betacem_qp.hpp"
#include "betacem_sample.hpp"
#include "betacem_select.hpp"

namespace mpcmmd {

namespace {

// k_bcem_small: the 20 beta-iterations of one candidate in one workgroup
// (small batches: the reference's num_batch = 100, BASELINE configs[4]'s
// CARLA solves).  At B = 100 the seven per-iteration kernels run as
// one latency-bound launch each (10-27 us for a few microseconds of work per
// candidate, 140 launches per outer iteration); here the same phases follow
// each other inside one launch, separated by workgroup barriers, with the
// candidate's intermediates (samples, selections, K_red, generators) in
// global memory that this workgroup alone touches -- L2-resident at this
// size.  Every phase is the body of its multi-kernel counterpart (same
// operations, so the same bits): samples by bsample_unit_lds (a wave per tile
// and chunk), selection by bselect_wave, kernel sums / K_red by bkernel_body,
// direct row sums by bdirect_body, the QPs by bqp_solve (a quad each), elites by
// belite_body, generators by bgen_wave, sigma_best by bsigma_body.
// Only for n <= 16 (M <= 256, bcem_small_ok), where every phase fits 128
// VGPRs (the QPs of n > 16 need up to 256): kSmallWaves = kKerWaves = 16 waves
// (1024 threads), and the selection is k_bselect's (R, G) = (1, 32) of n <= 24.
constexpr int kSmallWaves = kKerWaves, kSmallThreads = 64 * kSmallWaves;
constexpr int kSmallSelR = 1, kSmallSelG = 32;
constexpr size_t kSmallCandBytes = size_t(64 * kSmallSelR + 8) * 8;     // select_walk's cand
constexpr size_t kSmallSelBytes = kSmallCandBytes + 64 * 4 + 128 * 4;  // one wave's select LDS: cand, lm, scratch
HDI size_t small_lds(int M, int n) {
  size_t b = kSmallWaves * kSmallSelBytes + size_t(kNew) * ygen_stride(M) * 4;  // + the staged sample rows
  const size_t k = ker_lds(M, n, ker_scratch(M, n, 1)).total;  // (>= kKerTabBytes: covers bgen_wave's pivot columns)
  const size_t d = dir_lds(M, n).total, e = elite_lds(M + 1, kSmallWaves).total;
  const size_t q = (size_t(kBetaSamples) * tri_stride(n) + kQpZeros) * 4;  // the QPs' K_red and zeros
  const size_t gl = ((gen_lds_bytes(M) + 15) & ~size_t(15)) + tblk_lds_bytes(M);  // the sampler's copy + T blocks
  b = b > q ? b : q;
  b = b > gl ? b : gl;
  b = b > k ? b : k;
  b = b > d ? b : d;
  b = b > e ? b : e;
  return b;
}

// the persistent LDS copies (k_bcem_small's persist): after the phases' space
HDI size_t small_persist_off(int M, int n) { return (small_lds(M, n) + 15) & ~size_t(15); }
HDI size_t small_persist_bytes(int M) { return size_t(M) * (kMomStride + kFeatStride) * 4; }

// phase stamps of beta-iteration 5 (MPCMMD_STAMPW; rows 32768 + workgroup,
// apart from the kernel-sum body's own stamps): tools/stamp_small.py
#define SMALL_STAMP(p, slot)                                                             \
  do {                                                                                   \
    if (tidx() == 0 && (p).dbgw)                                                    \
      (p).dbgw[size_t(32768 + blockIdx.x) * 8 + (slot)] = __builtin_amdgcn_s_memrealtime(); \
  } while (0)

// NQ: select_walk's keys per lane (M <= 64 NQ); NP: bqp_solve's padded size
template <int NQ, int NP>
__global__ __launch_bounds__(kSmallThreads) void k_bcem_small(Params p0, int persist) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int cand = blockIdx.x;
  const int tid = tidx();
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  // persist: the candidate's series records and feature rows (fixed for the
  // outer iteration) copied once into LDS past the phases' space, for the
  // kernel-sum phase of every beta-iteration
  const float4* mom_l = nullptr;
  const float4* feat_l = nullptr;
  if (persist) {
    const int M = p0.M, b = p0.b0 + cand;
    float4* pm = reinterpret_cast<float4*>(smem + small_persist_off(M, p0.n));
    float4* pf = pm + M * (kMomStride / 4);
    const float4* gm = reinterpret_cast<const float4*>(p0.bmom + size_t(b) * M * kMomStride);
    const float4* gf = reinterpret_cast<const float4*>(p0.featr + size_t(b) * M * kFeatStride);
    for (int i = tid; i < M * (kMomStride / 4); i += kSmallThreads) pm[i] = gm[i];
    for (int i = tid; i < M * (kFeatStride / 4); i += kSmallThreads) pf[i] = gf[i];
    mom_l = pm;
    feat_l = pf;
    __syncthreads();
  }
  for (int tb = 0; tb < kBetaIters; ++tb) {
    // the launch's Params read through a pointer laundered per iteration: no
    // field (nor anything computed from one) is hoisted out of the loop
    typedef const Params __attribute__((address_space(4)))* KParams;
    KParams pk = (KParams)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(pk));
    const Params& p = *(const Params*)pk;
    const int b = p.b0 + cand, M = p.M, n = p.n;
    const int ntri = tri_stride(n);
    // samples of this iteration (compute_beta.py:51-68); the first ones are
    // the shared initial draws (Q3), taken from the handle's selection table
    if (tb > 0) {
      if (tb == 5) SMALL_STAMP(p, 0);
      {  // the generators into LDS (the W plane, an image of the U rows formed
         // here from the elite rows and means, genm), then the walkers
        const int Pp = pos_pad(M), M1 = M + 1;
        const double2* gsrc = reinterpret_cast<const double2*>(p.gen + size_t(b) * Pp * kGenStride);
        const double2* msrc = reinterpret_cast<const double2*>(p.genm + size_t(b) * Pp);
        double2* dst = reinterpret_cast<double2*>(smem);
        const int nw = Pp * (kGenRow / 2), ng = 2 * nw, nm = Pp >> 1;  // double2 counts: W plane, both, genm
        for (int i = tid; i < nw + nm; i += kSmallThreads) dst[i < nw ? i : i + nw] = i < nw ? gsrc[i] : msrc[i - nw];
        const float* E = gen_elites(p, tb, b);
        const double* mrow = gen_mean_row(p, b);
        double* ul = reinterpret_cast<double*>(smem) + lds_uplane(Pp);
        for (int i = tid; i < Pp * kGenRow; i += kSmallThreads) {
          const int pos = i / kGenRow, q = i - pos * kGenRow;
          const double m = mrow[pos];  // 0 at padding positions, whose u is 0
          const float e = pos < M1 ? E[min(q, kBetaElite - 1) * M1 + pos] : 0.0f;
          ul[i] = q < kBetaElite ? gen_u(e, m) : gen_mean_slot(m);
        }
        if (tid < 8) dst[ng + nm + tid] = double2{0.0, 0.0};
      }
      __syncthreads();
      {
        const double* lg = reinterpret_cast<const double*>(smem);
        double* Tl = reinterpret_cast<double*>(smem + ((gen_lds_bytes(M) + 15) & ~size_t(15)));
        bsample_tblocks(p, lg, Tl, w, kSmallWaves);
        __syncthreads();
        const int nblk = pos_pad(M) >> 4, units = kSampleTiles * ((nblk + sample_chunk(nblk) - 1) / sample_chunk(nblk));
        for (int u = w; u < units; u += kSmallWaves) bsample_unit_lds(p, tb, b, u % kSampleTiles, u / kSampleTiles, lg, Tl);
      }
      __syncthreads();
      if (tb == 5) SMALL_STAMP(p, 1);
      // the new samples' rows into LDS (after the waves' select scratch), so
      // each wave's top-n walk reads its keys at LDS latency: a wave's chain of
      // samples otherwise waits on one L2 round trip per sample.  Then
      // bselect_wave's walk (samples first_sample(tb) = 11 .. 99: the elites'
      // selections were carried) on the staged rows
      const int ys = ygen_stride(M);
      const float* Yl = reinterpret_cast<const float*>(smem + kSmallWaves * kSmallSelBytes);
      {
        const float4* src = reinterpret_cast<const float4*>(p.ygen + size_t(b) * kBzCols * ys);
        float4* dst = reinterpret_cast<float4*>(smem + kSmallWaves * kSmallSelBytes);
        for (int i = tid; i < kNew * (ys >> 2); i += kSmallThreads) dst[i] = src[i];
      }
      __syncthreads();
      char* sw = smem + size_t(w) * kSmallSelBytes;
      unsigned long long* cand_l = reinterpret_cast<unsigned long long*>(sw);
      uint32_t* lm = reinterpret_cast<uint32_t*>(sw + kSmallCandBytes);
      int* scr = reinterpret_cast<int*>(sw + kSmallCandBytes + 64 * 4);
      {
        int32_t* sel = p.bsel + size_t(b) * kBetaSamples * n;
        float* sig = p.bsig + size_t(b) * kBetaSamples;
        auto row = [&](int s) {
          const float* r = Yl + size_t(s - kBetaElite) * ys;
          return [=](int j) { return r[j]; };
        };
        const int s_lo = first_sample(tb), lane = tid & 63;
        if (s_lo + w < kBetaSamples) {
          select_walk<NQ, kSmallSelR, kSmallSelG>(row, [&](int s) { return sel + s * n; }, s_lo + w, kBetaSamples,
                                                  kSmallWaves, M, n, cand_l, lm, scr);
          for (int s2 = s_lo + w + lane * kSmallWaves; lane < 16 && s2 < kBetaSamples; s2 += 16 * kSmallWaves)
            sig[s2] = row(s2)(M);  // tb >= 1: rows are clipped when written
        }
      }
    } else {
      for (int e = tid; e < kBetaSamples * n; e += kSmallThreads) p.bsel[size_t(b) * kBetaSamples * n + e] = p.sel0[e];
      for (int e = tid; e < kBetaSamples; e += kSmallThreads) p.bsig[size_t(b) * kBetaSamples + e] = p.sig0[e];
    }
    __syncthreads();
    if (tb == 5) SMALL_STAMP(p, 2);
    // K_mixed row sums and K_red (compute_beta.py:120-127).  The direct sums
    // by rows (bdirect_body): a candidate's direct pairs share its M rows
    // several times over, and the pair-list form (direct_pairs_wave) measured
    // no faster here (CARLA n = 10: 24.2 vs 24.3 ms per solve)
    bkernel_body<false, true>(p, tb, cand, 0, 1, int(ker_scratch(M, n, tb)), smem, mom_l, feat_l);
    __syncthreads();
    if (tb == 5) SMALL_STAMP(p, 3);
    if (tb > 0) {
      const int total = bdirect_total(p, b, 1);  // block-uniform
      if (total > 0) {
        bdirect_body<1, kSmallWaves>(p, tb, 1, 1, cand, 0, total, smem);  // M <= 256: one float4 per lane
        __syncthreads();
      }
    }
    if (tb == 5) SMALL_STAMP(p, 4);
    // the QPs (compute_beta.py:70-91), a quad each, the samples' K_red staged
    // in LDS (one contiguous copy: the candidate's triangles are consecutive)
    {
      const int s_lo = first_sample(tb), per = kBetaSamples - s_lo;
      const float4* src = reinterpret_cast<const float4*>(p.bkred + (size_t(b) * kBetaSamples + s_lo) * ntri);
      float4* kl4 = reinterpret_cast<float4*>(smem);
      for (int i = tid; i < per * (ntri >> 2); i += kSmallThreads) kl4[i] = src[i];
      if (tid < kQpZeros) reinterpret_cast<float*>(smem)[per * ntri + tid] = 0.0f;
      __syncthreads();
      static_assert(kSmallThreads / 4 >= kBetaSamples, "one quad per QP");
      const int g = tid >> 2;
      const bool ok = g < per;
      const int gc = ok ? g : 0;
      bqp_solve<NP>(p, b, s_lo + gc, ok, reinterpret_cast<const float*>(smem) + size_t(gc) * ntri,
                    reinterpret_cast<const float*>(smem) + size_t(per) * ntri);
    }
    __syncthreads();
    if (tb == 5) SMALL_STAMP(p, 5);
    // elites, mean, generator level 1 (compute_beta.py:51-68, 133-157)
    belite_body(p, tb, b, smem);
    __syncthreads();
    if (tb == 5) SMALL_STAMP(p, 6);
    // generator level 2, a wave per 16-position block
    {
      const int nblk = (M + 1 + 15) / 16;
      double* xl = reinterpret_cast<double*>(smem) + 32 * w;
      for (int blk = w; blk < nblk; blk += kSmallWaves) bgen_wave(p, tb, b, blk, xl);
    }
    __syncthreads();
    if (tb == 5) SMALL_STAMP(p, 7);
    if (tb == kBetaIters - 1 && p.bimin[b] >= kBetaElite) {  // block-uniform
      bsigma_body(p, tb, b, reinterpret_cast<double*>(smem));
      __syncthreads();
    }
  }
}

}  // namespace

// M <= 256 (n <= 16): at n = 22 the per-iteration kernels, which spread each
// phase over the whole chip, measured faster (CARLA n = 22: 63.0 vs 70.9 ms
// per tick), and the kernel is built for no larger size
bool bcem_small_ok(const Params& p) {
  return p.gen_wave && p.M <= 256 && p.nb <= 512 && small_lds(p.M, p.n) <= kLdsBudget;
}

void launch_bcem_small(const Params& p, hipStream_t s) {
  const int n = p.n, M = p.M;
  const dim3 grid(p.nb), block(kSmallThreads);
  const size_t lp = small_persist_off(M, n) + small_persist_bytes(M);
  const int persist = lp <= kLdsBudget;  // the records and features stay in LDS when they fit
  const size_t lds = persist ? lp : small_lds(M, n);
  if (M <= 64)
    hipLaunchKernelGGL((k_bcem_small<1, 8>), grid, block, lds, s, p, persist);
  else if (M <= 128)
    hipLaunchKernelGGL((k_bcem_small<2, 12>), grid, block, lds, s, p, persist);
  else
    hipLaunchKernelGGL((k_bcem_small<4, 16>), grid, block, lds, s, p, persist);
}

}  // namespace mpcmmd
