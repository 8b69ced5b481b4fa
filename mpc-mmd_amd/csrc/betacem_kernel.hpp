// The beta-CEM kernel-sum phase's device code (k_bkernel.hip, k_bcem_small.hip).
//
// k_bkernel + k_bdirect: kernel_computation.py:19-65 / compute_beta.py:120-127
// for every sample of the iteration: the K_mixed row sums and K_red.
//
// k_bkernel, workgroup = (candidate, part of its samples):
//   union    the distinct mother rows the iteration's samples select (LDS
//            flags, scan): their rank and their series records (k_bmoment),
//            staged in LDS
//   series   every (sample s, reduced position k) pair whose a = R_r / sigma_s
//            is <= 1: row sum = exp(-a) * a 12-term Horner sum over the row's
//            moments, fp64, one thread per pair; the other pairs are flagged
//            for k_bdirect (Params::bdflag, a count per part in bdcount)
//   K_red    exp(-D[sel_k][sel_kk] / sigma_s), kk < k, the distances
//            recomputed from the feature rows (Params::featr) in k_bdist's
//            sequential feature order (bit-equal to D's entries), consecutive
//            entries stored by consecutive lanes.  When the pairwise distances
//            of the union fit the LDS budget (after the first few
//            beta-iterations the samples concentrate: ~40-150 distinct rows
//            of 484 at n = 22) they are computed once (a lane per row a, the
//            rows b < a as LDS broadcasts) and each sample's entries are
//            exponentials of table lookups (a wave per sample, the lookups of
//            all its entries in flight together); otherwise a wave per sample
//            stages its n feature rows in LDS (rows kKerRowPitch floats apart:
//            conflict-free reads) and forms its n (n - 1) / 2 distances, one
//            lane per entry.  Params::ker_path (MPCMMD_KER_PATH; tests, A/B
//            timing) forces the gather, or a third path: the union's feature
//            rows staged once per workgroup, each entry from two of them.
// k_bdirect, workgroup = (candidate, part of its rows), only when a candidate
// has flagged pairs (a > 1: mostly the first beta-iteration, whose samples
// clipped to sigma = 0.01 have a ~ 100): the flagged pairs counting-sorted by
// mother row r (LDS); a wave takes the next distinct row (LDS counter,
// heaviest first) and holds its distance row (k_bdist) in registers (lane L:
// float4s L + 64 t; for short rows the next row's loads are issued before the
// current one is summed).  The row's pairs are summed 8 at a time: per lane
// and pair the lane's terms exp2(D[r][j] * (-log2 e / sigma_s)) (v_exp_f32,
// packed scale / add), then one transposing cross-lane reduction (permlane32
// / permlane16 swaps, DPP) leaves pair j's row sum in lane 8 j + 4.
// From the second beta-iteration on, samples 0..10 are the previous elites:
// their selection, kernels and QP are unchanged, k_belite carried them, and
// only samples 11..99 are processed here.
#pragma once
#include "betacem_common.hpp"

namespace mpcmmd {

namespace {

// 1 / (k + 1) for the Horner steps of the series
__constant__ double kInvK[kMom] = {1.0,       1.0 / 2,  1.0 / 3,  1.0 / 4,  1.0 / 5,  1.0 / 6,
                                   1.0 / 7,   1.0 / 8,  1.0 / 9,  1.0 / 10, 1.0 / 11, 1.0 / 12};

// row sum of one pair by the series: q = the row's record, na = -a.  The
// Horner sum in fp64; exp(-a) by v_exp_f32 (~1 ulp: the sum is rounded to
// fp32 anyway, as the reference's fp32 terms are)
DEVI float series_sum(const float4 (&q)[3], double na) {
  const double P[kMom] = {q[0].x, q[0].y, q[0].z, q[0].w, q[1].x, q[1].y,
                          q[1].z, q[1].w, q[2].x, q[2].y, q[2].z, q[2].w};
  double h = P[kMom - 1];
#pragma unroll
  for (int k = kMom - 2; k >= 0; --k) h = fma(h, na * kInvK[k], P[k]);  // P_k + (-a / (k + 1)) h
  constexpr double kLog2e = 1.44269504088896340736;
  return float(double(__builtin_amdgcn_exp2f(float(na * kLog2e))) * h);
}
static_assert(kMomR == 12 && kMom == 12, "record layout: P_0..P_11 in float4s 0..2, R in float4 3");

// L1 distance of two feature rows (LDS) in k_bdist's order: features 0..21,
// one sequential fp32 sum (22, 23 are padding)
DEVI float feat_l1(const float4* A, const float4* Bv) {
  constexpr int Q = kFeatStride / 4;
  float dd = 0.0f;
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const float4 x = A[q], y = Bv[q];
    dd = q == 0 ? fabsf(x.x - y.x) : dd + fabsf(x.x - y.x);
    dd = dd + fabsf(x.y - y.y);
    if (q < Q - 1) {
      dd = dd + fabsf(x.z - y.z);
      dd = dd + fabsf(x.w - y.w);
    }
  }
  return dd;
}

// The body of k_bkernel for part `part` of candidate `cand` (of `split`),
// kKerWaves waves (k_bkernel and the small-batch fused kernel k_bcem_small).
// mom_l / feat_l: LDS copies of the candidate's series records and feature
// rows (k_bcem_small, which keeps them for its 20 beta-iterations), else null
// (read from global memory).  kList: also append the flagged pairs to the
// candidate's list (k_bdirect_pairs).  kFlat: the K_red table lookups spread
// over every thread (k_bcem_small) instead of a wave per sample (k_bkernel)
template <bool kList, bool kFlat>
DEVI void bkernel_body(const Params& p, int tb, int cand, int part, int split, int scratch, char* smem,
                       const float4* mom_l = nullptr, const float4* feat_l = nullptr) {
  constexpr int NT = 64 * kKerWaves, Q = kFeatStride / 4;
  const int b = p.b0 + cand, M = p.M, n = p.n;
  const int tid = tidx(), lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const KerLds C = ker_lds(M, n, size_t(scratch));
  short* sl = reinterpret_cast<short*>(smem + C.sel);
  float* csg = reinterpret_cast<float*>(smem + C.csg);
  double* csd = reinterpret_cast<double*>(smem + C.csd);
  unsigned short* tri = reinterpret_cast<unsigned short*>(smem + C.tri);
  unsigned short* urank = reinterpret_cast<unsigned short*>(smem + C.urank);
  unsigned short* urow = reinterpret_cast<unsigned short*>(smem + C.urow);
  int* misc = reinterpret_cast<int*>(smem + C.misc);
  unsigned char* uflag = reinterpret_cast<unsigned char*>(smem + C.scratch);  // setup only
  const int ntri = tri_stride(n), nent = n * (n - 1) / 2;
  const int s_lo = first_sample(tb);
  const int i_lo = s_lo * n, i_hi = kBetaSamples * n;
  MPCMMD_STAMP(p, 16);
  MPCMMD_STAMPW(p, 0);
  const int32_t* gsel = p.bsel + size_t(b) * kBetaSamples * n;
  for (int i = i_lo + tid; i < i_hi; i += NT) sl[i] = short(gsel[i]);
  for (int s = s_lo + tid; s < kBetaSamples; s += NT) {
    const float sg = p.bsig[size_t(b) * kBetaSamples + s];
    csg[s] = kNegLog2e / sg;
    csd[s] = 1.0 / double(sg);
  }
  for (int k = 1 + w; k < n; k += kKerWaves)  // entry k (k - 1) / 2 + kk of the strict lower triangle
    for (int kk = lane; kk < k; kk += 64) tri[k * (k - 1) / 2 + kk] = (unsigned short)(k | kk << 8);
  for (int r = tid; r < M; r += NT) uflag[r] = 0;
  if (tid < 3) misc[tid] = 0;
  __syncthreads();
  for (int i = i_lo + tid; i < i_hi; i += NT) uflag[sl[i]] = 1;
  __syncthreads();
  {  // union ranks: exclusive scan of the flags (thread runs, wave scans, wave totals)
    const int per = (M + NT - 1) / NT, a = tid * per, e = min(M, a + per);
    int sq = 0;
    for (int r = a; r < e; ++r) sq += uflag[r];
    int y = sq;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int yo = __shfl_up(y, o, 64);
      if (lane >= o) y += yo;
    }
    if (lane == 63) misc[16 + w] = y;
    __syncthreads();
    int base = 0;
    for (int v = 0; v < w; ++v) base += misc[16 + v];
    y += base - sq;
    if (tid == NT - 1) misc[0] = y + sq;
    for (int r = a; r < e; ++r) {
      if (uflag[r]) {
        urank[r] = (unsigned short)y;
        urow[y] = (unsigned short)r;
        ++y;
      }
    }
  }
  __syncthreads();  // the flags are dead: the scratch now holds the union's records
  MPCMMD_STAMPW(p, 1);
  const int Uu = misc[0];
  {
    // the union's records: staged in LDS when they fit, else read in place
    const float4* mom = mom_l ? mom_l : reinterpret_cast<const float4*>(p.bmom + size_t(b) * M * kMomStride);
    const bool staged = !mom_l && size_t(Uu) * kMomStride * 4 <= size_t(scratch);  // block-uniform
    float4* lrec = reinterpret_cast<float4*>(smem + C.scratch);
    if (staged)
      for (int i = tid; i < Uu * 4; i += NT) lrec[i] = mom[size_t(urow[i >> 2]) * 4 + (i & 3)];
    for (int i = i_lo + tid; i < i_hi; i += NT) sl[i] = short(urank[sl[i]]);  // rows -> union ranks
    __syncthreads();
    const float4* rec = staged ? lrec : mom;
    // series pairs of this part's samples; the others flagged for k_bdirect
    float* rowsum = p.brow + size_t(b) * kBetaSamples * n;
    unsigned char* dflag = p.bdflag + size_t(b) * kBetaSamples * n;
    int nd = 0;
    const int ns = (kBetaSamples - s_lo - part + split - 1) / split;
    for (int j = tid; j < ns * n; j += NT) {
      const int sj = j / n, s = s_lo + part + split * sj, i = s * n + (j - sj * n);
      const float4* q = rec + 4 * (staged ? int(sl[i]) : int(urow[sl[i]]));
      const double na = -double(q[3].x) * csd[s];  // -a, a = R / sigma
      const bool series = -na <= kSeriesAMax;     // NaN sigma: direct (NaN sum, as the reference)
      if (series) {
        const float4 qq[3] = {q[0], q[1], q[2]};
        rowsum[i] = series_sum(qq, na);
      }
      const bool direct = !series && tb > 0;  // first iteration: k_bmoment summed them
      dflag[i] = direct ? 1 : 0;
      nd += direct ? 1 : 0;
      if (kList) {  // the direct-pair list (its order is free: every pair's sum is its own)
        const unsigned long long m = __ballot(direct);  // one atomic per wave
        if (m) {
          const int ld = __builtin_ctzll(m);
          int at = 0;
          if (lane == ld) at = atomicAdd(&p.bdlcount[size_t(b) * kBetaIters + tb], __popcll(m));
          at = __shfl(at, ld, 64) + __builtin_amdgcn_mbcnt_hi(unsigned(m >> 32), __builtin_amdgcn_mbcnt_lo(unsigned(m), 0u));
          if (direct && at < kBetaSamples * n) p.bdlist[size_t(b) * kBetaSamples * n + at] = i;
        }
      }
    }
    nd = wave_total(nd);
    if (lane == 0) atomicAdd(&misc[2], nd);
    __syncthreads();  // the records are dead
    if (tid == 0) {
      p.bdcount[size_t(b) * kMaxSplit + part] = misc[2];
      atomicAdd(&p.stats[2], static_cast<unsigned long long>(ns * n - misc[2]));
      if (part == 0) atomicAdd(&p.stats[3], static_cast<unsigned long long>((kBetaSamples - s_lo) * nent));
    }
  }
  MPCMMD_STAMP(p, 17);
  MPCMMD_STAMPW(p, 2);
  const float4* fg = feat_l ? feat_l : reinterpret_cast<const float4*>(p.featr + size_t(b) * M * kFeatStride);
  float* kbase = p.bkred + size_t(b) * kBetaSamples * ntri;
  // block-uniform.  Params::ker_path 0: the table when it fits, else the
  // per-sample gather; 1: the union image when it fits, else the gather (never
  // the table); 2: the gather.  The image is not a default path: at n = 22 its
  // two random rows per entry conflict in the LDS banks more than the gather's
  // compact slice and it measured slower; it is kept as the
  // third way to the same bits that tests/test_gpu_kred_paths.py compares
  constexpr int Qr = kKerRowPitch / 4;
  const bool table = p.ker_path == 0 && ker_tab_bytes(Uu) <= size_t(scratch);
  const bool image = p.ker_path == 1 && size_t(Uu) * kKerRowPitch * 4 <= size_t(scratch);
  if (table) {
    float* T = reinterpret_cast<float*>(smem + C.scratch);
    float4* Fu = reinterpret_cast<float4*>(smem + C.scratch + ((size_t(Uu) * (Uu - 1) / 2 * 4 + 15) & ~size_t(15)));
    for (int i = tid; i < Uu * Q; i += NT) {
      const int u = i / Q;
      Fu[i] = fg[size_t(urow[u]) * Q + (i - u * Q)];
    }
    __syncthreads();
    // work items: (block of 64 rows a, chunk of 16 rows b below the block's last row)
    const int nab = (Uu + 63) >> 6;
    auto chunks = [&](int ab) { return (min(64 * ab + 63, Uu - 1) + 15) >> 4; };
    int items = 0;
    for (int ab = 0; ab < nab; ++ab) items += chunks(ab);
    for (int it = w; it < items; it += kKerWaves) {
      int ab = 0, c = it;
      while (c >= chunks(ab)) c -= chunks(ab++);
      const int a = 64 * ab + lane;
      float fa[kF];
      {
        const float4* src = Fu + min(a, Uu - 1) * Q;
#pragma unroll
        for (int q = 0; q < Q; ++q) {
          const float4 v = src[q];
          fa[4 * q] = v.x;
          fa[4 * q + 1] = v.y;
          if (q < Q - 1) {
            fa[4 * q + 2] = v.z;
            fa[4 * q + 3] = v.w;
          }
        }
      }
      const int b_end = min(16 * c + 16, min(64 * ab + 63, Uu - 1));
      float* Ta = T + a * (a - 1) / 2;
#pragma unroll 2
      for (int bb = 16 * c; bb < b_end; ++bb) {
        const float4* fb = Fu + bb * Q;  // wave-uniform: LDS broadcast
        float dd = 0.0f;
#pragma unroll
        for (int q = 0; q < Q; ++q) {  // differences as packed pairs, the sum in feature order
          const float4 y = fb[q];
          const f2 d0 = f2{fa[4 * q], fa[4 * q + 1]} - f2{y.x, y.y};
          dd = q == 0 ? fabsf(d0.x) : dd + fabsf(d0.x);
          dd = dd + fabsf(d0.y);
          if (q < Q - 1) {
            const f2 d1 = f2{fa[4 * q + 2], fa[4 * q + 3]} - f2{y.z, y.w};
            dd = dd + fabsf(d1.x);
            dd = dd + fabsf(d1.y);
          }
        }
        if (bb < a && a < Uu) Ta[bb] = dd;
      }
    }
    __syncthreads();
    MPCMMD_STAMPW(p, 3);
    if constexpr (kFlat) {
      // k_bcem_small: the (sample, entry) items spread over every thread, kJ
      // items per thread in flight together (a wave per sample leaves most
      // lanes idle at small n: 45 entries at n = 10)
      constexpr int kJ = 4;
      const int ns = (kBetaSamples - s_lo - part + split - 1) / split, nitems = ns * nent;
      for (int i0 = tid; i0 < nitems; i0 += NT * kJ) {
        int s[kJ], e[kJ], t[kJ];
#pragma unroll
        for (int j = 0; j < kJ; ++j) {
          const int i = min(i0 + NT * j, nitems - 1), sj = i / nent;
          s[j] = s_lo + part + split * sj;
          e[j] = i - sj * nent;
          t[j] = tri[e[j]];
        }
        int u0[kJ], u1[kJ];
#pragma unroll
        for (int j = 0; j < kJ; ++j) {
          u0[j] = sl[s[j] * n + (t[j] & 0xFF)];
          u1[j] = sl[s[j] * n + (t[j] >> 8)];
        }
        float dv[kJ];
#pragma unroll
        for (int j = 0; j < kJ; ++j) {
          const int hi = max(u0[j], u1[j]), lo = min(u0[j], u1[j]);
          dv[j] = T[hi * (hi - 1) / 2 + lo];
        }
#pragma unroll
        for (int j = 0; j < kJ; ++j)
          if (i0 + NT * j < nitems)
            kbase[size_t(s[j]) * ntri + e[j]] = __builtin_amdgcn_exp2f(dv[j] * csg[s[j]]);
      }
    } else {
      // a wave per sample of this part, all its lookups in flight together
      // (entries lane + 64 j, j < kJ covers n <= 23; larger n loop)
      constexpr int kJ = 4;
      for (int s = s_lo + part + split * w; s < kBetaSamples; s += split * kKerWaves) {
        const short* su = sl + s * n;
        const float cs = csg[s];
        float* kr = kbase + size_t(s) * ntri;
        for (int e0 = 0; e0 < nent; e0 += 64 * kJ) {
          int t[kJ];
#pragma unroll
          for (int j = 0; j < kJ; ++j) t[j] = tri[min(e0 + lane + 64 * j, nent - 1)];
          int u0[kJ], u1[kJ];
#pragma unroll
          for (int j = 0; j < kJ; ++j) {
            u0[j] = su[t[j] & 0xFF];
            u1[j] = su[t[j] >> 8];
          }
          float dv[kJ];
#pragma unroll
          for (int j = 0; j < kJ; ++j) {
            const int hi = max(u0[j], u1[j]), lo = min(u0[j], u1[j]);
            dv[j] = T[hi * (hi - 1) / 2 + lo];
          }
#pragma unroll
          for (int j = 0; j < kJ; ++j)
            if (e0 + lane + 64 * j < nent)
              kr[e0 + lane + 64 * j] = __builtin_amdgcn_exp2f(dv[j] * cs);
        }
      }
    }
  } else if (image) {
    // the union's feature rows once per workgroup (the union records are
    // dead); sl holds union ranks, so entry (k, kk) of sample s reads rows
    // sl[s n + k] and sl[s n + kk] of the image.  A wave's samples are
    // independent: nothing is staged per sample, no wave_sync between them
    float4* Fu = reinterpret_cast<float4*>(smem + C.scratch);
    constexpr int kJ = 3;  // 478 rows (n = 22, first beta-iteration): 2868 float4s, 3 per thread in flight
    for (int i0 = tid; i0 < Uu * Q; i0 += NT * kJ) {
      float4 v[kJ];
#pragma unroll
      for (int j = 0; j < kJ; ++j) {
        const int i = min(i0 + NT * j, Uu * Q - 1), u = i / Q;
        v[j] = fg[size_t(urow[u]) * Q + (i - u * Q)];
      }
#pragma unroll
      for (int j = 0; j < kJ; ++j)
        if (i0 + NT * j < Uu * Q) {
          const int i = i0 + NT * j, u = i / Q;
          Fu[u * Qr + (i - u * Q)] = v[j];
        }
    }
    __syncthreads();
    MPCMMD_STAMPW(p, 3);
    for (int s = s_lo + part + split * w; s < kBetaSamples; s += split * kKerWaves) {
      const short* su = sl + s * n;
      const float cs = csg[s];
      float* kr = kbase + size_t(s) * ntri;
      for (int e = lane; e < nent; e += 64) {
        const int kk2 = tri[e];
        const float dd = feat_l1(Fu + su[kk2 & 0xFF] * Qr, Fu + su[kk2 >> 8] * Qr);
        kr[e] = __builtin_amdgcn_exp2f(dd * cs);
      }
    }
  } else {
    // per-sample: the union records are dead, sl holds union ranks (urow maps back)
    float4* Fw = reinterpret_cast<float4*>(smem + C.scratch) + size_t(w) * n * Qr;
    for (int s = s_lo + part + split * w; s < kBetaSamples; s += split * kKerWaves) {
      for (int k = lane; k < n; k += 64) {
        const float4* src = fg + size_t(urow[sl[s * n + k]]) * Q;
#pragma unroll
        for (int q = 0; q < Q; ++q) Fw[k * Qr + q] = src[q];
      }
      wave_sync();  // one wave's LDS operations run in order
      const float cs = csg[s];
      float* kr = kbase + size_t(s) * ntri;
      for (int e = lane; e < nent; e += 64) {
        const int kk2 = tri[e];
        const float dd = feat_l1(Fw + (kk2 & 0xFF) * Qr, Fw + (kk2 >> 8) * Qr);
        kr[e] = __builtin_amdgcn_exp2f(dd * cs);
      }
      wave_sync();  // the reads are done before the next sample's rows overwrite them
    }
  }
  MPCMMD_STAMP(p, 18);
  MPCMMD_STAMPW(p, 4);
}

// The per-lane part of a direct row sum: the lane's columns x (float4s
// lane + 64 t of the distance row) as exp2(D * cs), cs = -log2 e / sigma
// (packed scale, v_exp_f32; pad columns: +inf * cs = -inf -> 0), summed in
// two packed accumulators (the float4's column pairs) that are added at the
// end.  k_bdirect (do_row) and k_bdirect_pairs (direct_pairs_wave) both take
// their terms from here and reduce them by transpose_sum8: the same bits.
template <int NV4>
DEVI float pair_terms(const float4 (&x)[NV4], float cs) {
  const f2 c2 = {cs, cs};
  f2 a0, a1;
#pragma unroll
  for (int t = 0; t < NV4; ++t) {
    const f2 t0 = f2{x[t].x, x[t].y} * c2, t1 = f2{x[t].z, x[t].w} * c2;
    const f2 e0 = {__builtin_amdgcn_exp2f(t0.x), __builtin_amdgcn_exp2f(t0.y)};
    const f2 e1 = {__builtin_amdgcn_exp2f(t1.x), __builtin_amdgcn_exp2f(t1.y)};
    a0 = t == 0 ? e0 : a0 + e0;
    a1 = t == 0 ? e1 : a1 + e1;
  }
  a0 += a1;
  return a0.x + a0.y;
}

// flagged pairs of candidate b (k_bkernel's parts): k_bdirect's work
DEVI int bdirect_total(const Params& p, int b, int kparts) {
  int total = 0;
  for (int k = 0; k < kparts; ++k) total += p.bdcount[size_t(b) * kMaxSplit + k];
  return total;
}

// The body of k_bdirect for part `part` of candidate `cand` with `total` > 0
// flagged pairs, NW waves (k_bdirect: kDirWaves = 4; k_bcem_small: 16)
template <int NV4, int NW>
DEVI void bdirect_body(const Params& p, int tb, int split, int lpt, int cand, int part, int total, char* smem) {
  constexpr int kDirWaves = NW;
  constexpr bool kPrefetch = NV4 <= 4;
  constexpr int NT = 64 * kDirWaves;
  const int b = p.b0 + cand, M = p.M, n = p.n, Md = dist_stride(M);
  const int tid = tidx(), lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const DirLds C = dir_lds(M, n);
  short* sl = reinterpret_cast<short*>(smem + C.sel);
  float* csg = reinterpret_cast<float*>(smem + C.csg);
  unsigned short* pairs = reinterpret_cast<unsigned short*>(smem + C.pairs);
  unsigned short* ulist = reinterpret_cast<unsigned short*>(smem + C.ulist);
  unsigned short* ustart = reinterpret_cast<unsigned short*>(smem + C.ustart);
  unsigned short* order = reinterpret_cast<unsigned short*>(smem + C.order);
  int* bins = reinterpret_cast<int*>(smem + C.bins);
  int* misc = reinterpret_cast<int*>(smem + C.misc);
  int* cnt = reinterpret_cast<int*>(smem + C.scratch);  // setup only
  int* fill = cnt + M;
  unsigned short* start = reinterpret_cast<unsigned short*>(fill + M);
  float* rowsum = p.brow + size_t(b) * kBetaSamples * n;
  const unsigned char* dflag = p.bdflag + size_t(b) * kBetaSamples * n;
  const int s_lo = first_sample(tb);
  const int i_lo = s_lo * n, i_hi = kBetaSamples * n;
  const int32_t* gsel = p.bsel + size_t(b) * kBetaSamples * n;
  MPCMMD_STAMPW(p, 5);
  // direct pairs keep their row; the others get row -1
  for (int i = i_lo + tid; i < i_hi; i += NT) sl[i] = dflag[i] ? short(gsel[i]) : short(-1);
  for (int s = s_lo + tid; s < kBetaSamples; s += NT) csg[s] = kNegLog2e / p.bsig[size_t(b) * kBetaSamples + s];
  for (int r = tid; r < M; r += NT) {
    cnt[r] = 0;
    fill[r] = 0;
  }
  if (tid == 0) misc[0] = 0;
  for (int c = tid; c < kLptBins; c += NT) bins[c] = 0;
  __syncthreads();
  for (int i = i_lo + tid; i < i_hi; i += NT)
    if (sl[i] >= 0) atomicAdd(&cnt[sl[i]], 1);
  __syncthreads();
  {  // exclusive scans of cnt and (cnt > 0), packed as cnt | (cnt > 0) << 16
     // (totals <= 6400 pairs, <= 4096 rows): thread runs, wave scans, wave totals
    const int per = (M + NT - 1) / NT, a = tid * per, e = min(M, a + per);
    int sp = 0;
    for (int r = a; r < e; ++r) {
      const int c = cnt[r];
      sp += c | (c > 0) << 16;
    }
    int x = sp;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int y = __shfl_up(x, o, 64);
      if (lane >= o) x += y;
    }
    if (lane == 63) misc[16 + w] = x;
    __syncthreads();
    int base = 0;
    for (int v = 0; v < w; ++v) base += misc[16 + v];
    x += base - sp;  // exclusive prefix of this thread's run
    if (tid == NT - 1) {
      const int tot = x + sp;
      misc[1] = tot >> 16;
      ustart[tot >> 16] = (unsigned short)(tot & 0xFFFF);
    }
    for (int r = a; r < e; ++r) {
      const int c = cnt[r], x1 = x & 0xFFFF, x2 = x >> 16;
      start[r] = (unsigned short)x1;
      if (c > 0) {
        ulist[x2] = (unsigned short)r;
        ustart[x2] = (unsigned short)x1;
      }
      x += c | (c > 0) << 16;
    }
  }
  __syncthreads();
  const int U = misc[1];
  if (tid == 0 && part == 0) {
    atomicAdd(&p.stats[0], static_cast<unsigned long long>(U));
    atomicAdd(&p.stats[1], static_cast<unsigned long long>(total));
  }
  for (int i = i_lo + tid; i < i_hi; i += NT) {
    const int r = sl[i];
    if (r >= 0) pairs[start[r] + atomicAdd(&fill[r], 1)] = (unsigned short)i;
  }
  // grab order: heaviest rows (most pairs) first, so no wave starts a long
  // row while the others run dry (bucket sort by pair count; the order within
  // a bucket is arbitrary -- every row's outputs are independent of it -- so
  // only for a candidate in one workgroup: parts of a split candidate must
  // agree on the order)
  if (lpt && split == 1) {
    for (int u = tid; u < U; u += NT) atomicAdd(&bins[kLptBins - 1 - min(ustart[u + 1] - ustart[u], kLptBins - 1)], 1);
    __syncthreads();
    if (tid < 64) {  // exclusive scan of the 128 bins, two per lane
      const int a = bins[2 * tid], c = bins[2 * tid + 1];
      int x = a + c;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(x, o, 64);
        if (tid >= o) x += y;
      }
      bins[2 * tid] = x - a - c;
      bins[2 * tid + 1] = x - c;
    }
    __syncthreads();
    for (int u = tid; u < U; u += NT)
      order[atomicAdd(&bins[kLptBins - 1 - min(ustart[u + 1] - ustart[u], kLptBins - 1)], 1)] = (unsigned short)u;
  } else {
    for (int u = tid; u < U; u += NT) order[u] = (unsigned short)u;
  }
  __syncthreads();
  MPCMMD_STAMP(p, 19);
  MPCMMD_STAMPW(p, 6);
  const float4* Dg = reinterpret_cast<const float4*>(p.bdist + size_t(b) * M * Md);
  // this part's rows order[part + split q], q from the workgroup's counter
  // (U: past the end)
  auto grab = [&]() {
    int q = 0;
    if (lane == 0) q = atomicAdd(&misc[0], 1);
    const int i = part + split * __builtin_amdgcn_readfirstlane(q);
    return i < U ? int(order[i]) : U;
  };
  auto load = [&](float4 (&x)[NV4], int u) {
    const float4* src = Dg + size_t(ulist[u]) * (Md >> 2) + lane;
#pragma unroll
    for (int t = 0; t < NV4; ++t) x[t] = src[64 * t];
  };
  // one distinct row u held in x: its pairs 8 at a time
  auto do_row = [&](const float4 (&x)[NV4], int u) {
    const int pb = ustart[u], pc = ustart[u + 1] - pb;
    for (int c0 = 0; c0 < pc; c0 += 64) {  // (rows with more than 64 pairs: chunks)
      // lane l holds pair c0 + l and its scale; batches broadcast them by readlane
      const int cc = min(64, pc - c0);
      const int pl = pairs[pb + c0 + min(lane, cc - 1)];
      const float cl = csg[pl / n];
      for (int j0 = 0; j0 < cc; j0 += 8) {
        float v[8];
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) {
          v[jj] = 0.0f;
          if (j0 + jj < cc) v[jj] = pair_terms<NV4>(x, readlane(cl, j0 + jj));
        }
        const float sum = transpose_sum8(v, tidx() & 63);
        // lane group j = lane >> 3 takes pair j0 + j
        const int jg = j0 + (lane >> 3);
        const int pj = __shfl(pl, jg, 64);
        if ((lane & 7) == 4 && jg < cc) rowsum[pj] = sum;
      }
    }
  };
  float4 d[NV4];
  int u = grab();
  if (kPrefetch) {
    // ping-pong: the next row's loads are issued (unconditionally, a past-the-
    // end index clamped to the current row) before the current row is summed,
    // so the memory-counter waits are exact and the loads overlap the exps
    float4 dn[NV4];
    if (u < U) load(d, u);
    while (u < U) {
      const int un = grab();
      load(dn, un < U ? un : u);
      do_row(d, u);
      if (un >= U) break;
      const int unn = grab();
      load(d, unn < U ? unn : un);
      do_row(dn, un);
      u = unn;
    }
  } else {
    for (; u < U; u = grab()) {
      load(d, u);
      do_row(d, u);
    }
  }
  MPCMMD_STAMP(p, 20);
  MPCMMD_STAMPW(p, 7);
}

// Direct row sums from k_bkernel's list of flagged pairs (k_bdirect_pairs),
// no per-candidate setup (bdirect_body counting-sorts the
// pairs by mother row in LDS first, which at the reference's num_batch = 100
// -- CARLA, where about half of all pairs are direct at every beta-iteration
// -- costs more than the sums).  A wave takes PJ listed pairs, issues all
// their distance-row loads (lane L: float4s L + 64 t of row sel[i]) before the
// first exponential, forms each pair's per-lane terms by pair_terms, as
// bdirect_body's do_row does, and reduces the PJ slots by one transpose_sum8,
// whose tree is the same for every slot: the bits of bdirect_body.
// Groups g0, g0 + gs, .. of PJ listed pairs of candidate b (cnt pairs) on the
// calling wave.
template <int NV4, int PJ>
DEVI void direct_pairs_wave(const Params& p, int b, int cnt, int g0, int gs) {
  static_assert(PJ >= 1 && PJ <= 8, "pairs per wave");
  const int M = p.M, n = p.n, Md = dist_stride(M);
  const int lane = tidx() & 63;
  const int groups = (cnt + PJ - 1) / PJ;
  const int32_t* list = p.bdlist + size_t(b) * kBetaSamples * n;
  const int32_t* gsel = p.bsel + size_t(b) * kBetaSamples * n;
  const float* gsig = p.bsig + size_t(b) * kBetaSamples;
  float* rowsum = p.brow + size_t(b) * kBetaSamples * n;
  const float4* Dg = reinterpret_cast<const float4*>(p.bdist + size_t(b) * M * Md);
  for (int g = g0; g < groups; g += gs) {
    int pi[PJ];
    float cs[PJ];
    float4 x[PJ][NV4];
#pragma unroll
    for (int j = 0; j < PJ; ++j) {  // a past-the-end slot repeats the group's first pair (not stored)
      const int k = g * PJ + j < cnt ? g * PJ + j : g * PJ;
      pi[j] = list[k];
    }
#pragma unroll
    for (int j = 0; j < PJ; ++j) {
      const float4* src = Dg + size_t(gsel[pi[j]]) * (Md >> 2) + lane;
#pragma unroll
      for (int t = 0; t < NV4; ++t) x[j][t] = src[64 * t];
      cs[j] = kNegLog2e / gsig[pi[j] / n];
    }
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = 0.0f;
#pragma unroll
    for (int j = 0; j < PJ; ++j) v[j] = pair_terms<NV4>(x[j], cs[j]);
    const float sum = transpose_sum8(v, tidx() & 63);  // slot j's total in lanes 8 j + 4..7
    const int j = lane >> 3;
    int pj = pi[0];
#pragma unroll
    for (int q = 1; q < PJ; ++q) pj = j == q ? pi[q] : pj;
    if ((lane & 7) == 4 && j < PJ && g * PJ + j < cnt) rowsum[pj] = sum;
  }
}

// pairs per wave of the pair-list direct sums: as many distance rows in flight
// as fit ~64 VGPRs of operands (NV4 float4s per lane and row)
HDI_CONST int direct_pj(int nv4) { return nv4 <= 2 ? 8 : (nv4 <= 4 ? 4 : (nv4 <= 8 ? 2 : 1)); }

}  // namespace

}  // namespace mpcmmd
