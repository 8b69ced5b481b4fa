// The beta-CEM elite / generator phase's device code (k_belite.hip,
// k_bcem_small.hip).
//
// k_belite: elites, mean, next generators; on the last iteration the outputs
// (beta_best, sigma_best with the post-update quirk Q4, the reduced set).
// Positions are thread-strided (lane = position), so a wave covers four
// whole 16-position blocks: mean and u_j stay in the thread's registers and
// the block sums of u u^T are row-of-16 DPP reductions.  LDS holds only the
// block sums (nblk x 66 fp64) and small bookkeeping.
#pragma once
#include "betacem_common.hpp"

namespace mpcmmd {

namespace {

// packed upper index of (a <= c) in an 11 x 11 symmetric matrix
HDI int sym11(int a, int c) { return a * 11 - a * (a - 1) / 2 + (c - a); }
HDI int sym11i(int a, int c) { return a <= c ? sym11(a, c) : sym11(c, a); }

// The body of k_belite for candidate b (any whole number of waves)
DEVI void belite_body(const Params& p, int tb, int b, char* smem) {
  const int M = p.M, M1 = M + 1, n = p.n, tid = tidx();
  const EliteLds C = elite_lds(M1, blockDim.x >> 6);
  double* Gb = reinterpret_cast<double*>(smem + C.Gb);
  int* elite = reinterpret_cast<int*>(smem + C.misc);    // [11]
  int* info = elite + 16;                                 // [0] imin, [1] any NaN
  float* cst = reinterpret_cast<float*>(info + 16);       // [100]
  float* sig_new = cst + kBetaSamples;                    // [11] sigma of the new elite rows
  uint32_t* ckey = reinterpret_cast<uint32_t*>(sig_new + 12);  // [100] sort keys of the costs (16-byte aligned)
  const float* costs = p.bcost + size_t(b) * kBetaSamples;
  if (tid < kBetaSamples) {
    const float c = costs[tid];
    cst[tid] = c;
    ckey[tid] = sort_key(c);
  }
  if (tid == 0) {
    info[0] = -1;
    info[1] = 0;
  }
  __syncthreads();
  if (tid < kBetaSamples) {
    // stable rank: 25 broadcast reads of four keys each, all in flight
    const uint32_t ks = ckey[tid];
    const uint4* k4 = reinterpret_cast<const uint4*>(ckey);
    int r = 0;
#pragma unroll
    for (int k = 0; k < kBetaSamples / 4; ++k) {
      const uint4 v = k4[k];
      r += int(v.x < ks || (v.x == ks && 4 * k < tid)) + int(v.y < ks || (v.y == ks && 4 * k + 1 < tid)) +
           int(v.z < ks || (v.z == ks && 4 * k + 2 < tid)) + int(v.w < ks || (v.w == ks && 4 * k + 3 < tid));
    }
    if (r < kBetaElite) elite[r] = tid;
    if (cst[tid] != cst[tid]) {
      atomicOr(&info[1], 1);
      atomicMin(reinterpret_cast<unsigned*>(&info[0]), unsigned(tid));  // first NaN (-1 == max)
    }
  }
  __syncthreads();
  const int imin = info[1] ? info[0] : elite[0];  // jnp.argmin: first NaN, else first minimum
  if (tid == 0) {
    p.res_beta[size_t(b) * kBetaIters + tb] = info[1] ? __int_as_float(0x7fc00000) : cst[elite[0]];
    double es = 0.0;  // elite costs in rank order (the parity trace; tests/parity.py)
    for (int q = 0; q < kBetaElite; ++q) es += double(cst[elite[q]]);
    p.btrace[size_t(b) * kBetaIters + tb] = float(es);
  }
  // the elites are samples 0..10 of the next iteration, unchanged: carry
  // their top-n rows, sigma, QP solution and cost there (first_sample)
  if (tb < kBetaIters - 1) {
    int* csel = reinterpret_cast<int*>(smem + C.carry);
    float* ctop = reinterpret_cast<float*>(csel + kBetaElite * n);
    float* csig = ctop + kBetaElite * n;
    float* ccost = csig + kBetaElite;
    const size_t rb = size_t(b) * kBetaSamples;
    for (int i = tid; i < kBetaElite * n; i += blockDim.x) {
      const int q = i / n, k = i - q * n;
      const size_t src = (rb + elite[q]) * n + k;
      csel[i] = p.bsel[src];
      ctop[i] = p.btop[src];
    }
    if (tid < kBetaElite) {
      csig[tid] = p.bsig[rb + elite[tid]];
      ccost[tid] = cst[elite[tid]];
    }
    __syncthreads();
    for (int i = tid; i < kBetaElite * n; i += blockDim.x) {
      p.bsel[rb * n + i] = csel[i];
      p.btop[rb * n + i] = ctop[i];
    }
    if (tid < kBetaElite) {
      p.bsig[rb + tid] = csig[tid];
      p.bcost[rb + tid] = ccost[tid];
    }
  }
  // ---- per position j: E_new column (the 11 elite sample values: previous
  // elites, this iteration's new samples (ygen) or, at tb = 0, the initial
  // samples), mean, u = (E - mean) / sqrt(10), block sums of u u^T
  const float* Eold = p.belite + (size_t(tb & 1) * p.Bt + b) * kBetaElite * M1;
  float* Enew = p.belite + (size_t((tb + 1) & 1) * p.Bt + b) * kBetaElite * M1;
  const int ys = ygen_stride(M);
  const float* Y = p.ygen + size_t(b) * kBzCols * ys;
  double* gmean = p.gen + size_t(b) * pos_pad(M) * kGenStride + gen_means(pos_pad(M));
  const int nblk = (M1 + 15) / 16;
  const int span = ((nblk * 16 + 63) / 64) * 64;  // whole waves
  for (int j = tid; j < span; j += blockDim.x) {
    const bool valid = j < M1;
    double u[kBetaElite];
    {
      float v[kBetaElite];
      double s = 0.0;
      const int jc = min(j, M);
      // the 11 loads are unconditional (clamped position, source row chosen
      // by pointer) so they are in flight together
#pragma unroll
      for (int q = 0; q < kBetaElite; ++q) {
        const int e = elite[q];
        const float* src = tb == 0 ? p.beta_z0 + size_t(e) * M1
                                   : (e < kBetaElite ? Eold + size_t(e) * M1 : Y + size_t(e - kBetaElite) * ys);
        v[q] = src[jc];
      }
#pragma unroll
      for (int q = 0; q < kBetaElite; ++q) {
        float x = v[q];
        if (tb == 0) {
          x = float(kSqrt20 * double(x));
          if (j == M) x = fmaxf(x, 0.01f);
        }
        x = valid ? x : 0.0f;
        if (valid) {
          Enew[size_t(q) * M1 + j] = x;
          if (j == M) sig_new[q] = x;
        }
        v[q] = x;
        s = s + double(x);
      }
      const double m = s / double(kBetaElite);
#pragma unroll
      for (int q = 0; q < kBetaElite; ++q) u[q] = valid ? gen_u(v[q], m) : 0.0;
      // the generators' readers re-form u from Enew and this mean (layout.hpp)
      if (valid) gmean[j] = m;
    }
    // level 1: block sums G = U^T U of u u^T over each 16-position block (66
    // packed entries) on fp64 MFMA: the wave's four blocks one at a time, the
    // block's u rows staged in the wave's LDS slice, then 4 x
    // v_mfma_f64_16x16x4 with A = B = U (lane (r, h) of step s: feature r of
    // position 4 s + h; features 11..15 zero)
    double* ub = reinterpret_cast<double*>(smem + C.ublk) + (tid >> 6) * 16 * kUPitch;
    const int lane = tid & 63, r = lane & 15, h = lane >> 4;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int blk = (j >> 6) * 4 + k;  // wave-uniform
      if ((lane >> 4) == k) {
#pragma unroll
        for (int q = 0; q < kBetaElite; ++q) ub[(lane & 15) * kUPitch + q] = u[q];
      }
      wave_sync();
      d4 G = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int st = 0; st < 4; ++st) {
        const double x = r < 11 ? ub[(4 * st + h) * kUPitch + r] : 0.0;
        G = mfma64(x, x, G);
      }
      wave_sync();
      // register i: G[h + 4 i][r]; the packed upper triangle a <= c
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int a = h + 4 * i;
        if (blk < nblk && a <= r && r < 11) Gb[blk * 66 + sym11(a, r)] = G[i];
      }
    }
  }
  __syncthreads();
  // block prefix: phib[blk] <- Phi at the start of blk = I + sum_{<blk} / d
  if (tid < 66) {
    int a = 0, c = tid;
    while (c >= 11 - a) {
      c -= 11 - a;
      ++a;
    }
    c += a;
    double acc = a == c ? 1.0 : 0.0;
    double* ph = p.phib + size_t(b) * nblk * 66;
#pragma unroll 8
    for (int blk = 0; blk < nblk; ++blk) {  // the LDS reads of several blocks in flight
      const double g = Gb[blk * 66 + tid];
      ph[blk * 66 + tid] = acc;
      acc = fma(g, kInvRidge, acc);
    }
  }
  // last iteration: beta_best / reduced set of argmin (pre-update) and, when
  // argmin is a carried elite, sigma_best (Q4); k_bsigma handles a new sample
  if (tb == kBetaIters - 1) {
    const int* bsel = p.bsel + (size_t(b) * kBetaSamples + imin) * n;
    for (int i = tid; i < n; i += blockDim.x) {
      p.bestsel[size_t(b) * n + i] = bsel[i];
      p.beta[size_t(b) * n + i] = p.btop[(size_t(b) * kBetaSamples + imin) * n + i];
    }
    if (tid == 0) {
      p.bimin[b] = imin;
      if (imin < kBetaElite) p.sigma[b] = sig_new[imin];
    }
  }
}

// The generators of block blk of candidate b on one wave (Params::gen_wave:
// small batches, where k_bgen's chain of 11 pivots + 16 positions x (an
// 11-term dot product, sqrt, divide, 11 broadcasts) on one quad is the whole
// latency).  The same quantities in block form:
//   A = Phi_b^-1                    symmetric sweep of Phi_b (11 pivots, a
//                                   lane per matrix entry; -A after the sweep)
//   V = A U,  G = 0.05 I + U^T V    fp64 MFMA (3 + 3 of 16x16x4; U = the
//                                   block's 16 u_j as columns, features 11..
//                                   15 zero)
//   G = L L^T,  W = V L^-T          right-looking Cholesky of the 16 x 16 G,
//                                   V updated alongside (16 pivots)
// -- L_jj and w_j are k_bgen's (G_jj - sum_{i<j} L_ji^2 = 0.05 + u_j . A_j u_j
// with A_j = A - sum_{i<j} w_i w_i^T; w_j = (A u_j - sum_{i<j} w_i L_ji) /
// L_jj = A_j u_j / L_jj), summed in another order (fp64; ~1e-16 apart).
// Every matrix is in the f64 MFMA accumulator layout (lane (r, h), register
// i: row h + 4 i, column r); a pivot step publishes column k through the
// wave's 32 doubles of LDS (xl) and every lane updates its entries.  The
// sweep keeps A exactly symmetric (mirrored entries see the same products),
// so register s of A is also the A operand of step s of A U.
// 1 / d and 1 / sqrt(d) for d > 0: the hardware estimate and two Newton
// steps (a few ulp; the pivots' chain is these few dependent operations, not
// the IEEE divide and square root sequences)
DEVI double rcp_nr(double d) {
  double y = __builtin_amdgcn_rcp(d);
  y = fma(y, fma(-d, y, 1.0), y);
  return fma(y, fma(-d, y, 1.0), y);
}
DEVI double rsq_nr(double d) {
  double y = __builtin_amdgcn_rsq(d);
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const double e = fma(-(d * y), y, 1.0);
    y = fma(0.5 * y, e, y);
  }
  return y;
}

// Block blk (< nblk) of candidate b on the calling wave, after k_belite of
// beta-iteration tb.  xl: the wave's 32 doubles of LDS.
DEVI void bgen_wave(const Params& p, int tb, int b, int blk, double* xl) {
  const int M = p.M, M1 = M + 1, nblk = (M1 + 15) / 16, Pp = pos_pad(M);
  const int lane = tidx() & 63, r = lane & 15, h = lane >> 4;
  double* gen = p.gen + size_t(b) * Pp * kGenStride;
  double* gm = p.genm + size_t(b) * Pp;
  const int j0 = blk * 16;
  d4 A;
  double U[3];
  const double* Gb = p.phib + (size_t(b) * nblk + blk) * 66;
  const float* E = gen_elites(p, tb + 1, b);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int a = h + 4 * i;
    A[i] = a < 11 && r < 11 ? Gb[sym11i(min(a, 10), min(r, 10))] : 0.0;
  }
  const int jr = min(j0 + r, M);  // clamped: the loads unconditional
  const double mr = gen_mean_row(p, b)[jr];
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    const int f = 4 * s + h;  // feature 11 is the mean's slot: zero here
    const float e = E[size_t(min(f, 10)) * M1 + jr];
    U[s] = f < 11 && j0 + r < M1 ? gen_u(e, mr) : 0.0;
  }
  // sweep: A_kk <- -1/d, A_ik = A_ki <- A_ik / d, A_ij <- A_ij - A_ik A_kj / d
#pragma unroll
  for (int k = 0; k < 11; ++k) {
    if (r == k) {
#pragma unroll
      for (int i = 0; i < 4; ++i) xl[h + 4 * i] = A[i];
    }
    wave_sync();
    const double d = xl[k], cr = xl[r];
    double ci[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) ci[i] = xl[h + 4 * i];
    wave_sync();
    const double id = rcp_nr(d);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int a = h + 4 * i;
      A[i] = a == k ? (r == k ? -id : cr * id) : (r == k ? ci[i] * id : A[i] - (ci[i] * cr) * id);
    }
  }
  const d4 zero = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int i = 0; i < 4; ++i) A[i] = -A[i];
  d4 V = zero, G = zero;
#pragma unroll
  for (int s = 0; s < 3; ++s) V = mfma64(A[s], U[s], V);
#pragma unroll
  for (int s = 0; s < 3; ++s) G = mfma64(U[s], V[s], G);
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (h + 4 * i == r) G[i] = G[i] + kRidge;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    if (r == k) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        xl[h + 4 * i] = G[i];
        xl[16 + h + 4 * i] = V[i];
      }
    }
    wave_sync();
    const double d = xl[k], gr = xl[r];
    double gi[4], vi[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      gi[i] = xl[h + 4 * i];
      vi[i] = xl[16 + h + 4 * i];
    }
    wave_sync();
    const double rl = rsq_nr(d);
    const double lr = r > k ? gr * rl : 0.0;
    double wk[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const double li = h + 4 * i > k ? gi[i] * rl : 0.0;
      wk[i] = vi[i] * rl;
      G[i] = G[i] - li * lr;
      V[i] = V[i] - wk[i] * lr;
    }
    const int j = j0 + k;  // the pivot's position
    if (r == k && j < M1) {
      double* g = gen + size_t(j) * kGenRow + kGenW;
#pragma unroll
      for (int i = 0; i < 3; ++i) g[h + 4 * i] = h + 4 * i < 11 ? wk[i] : 0.0;  // whole rows: slot 11 is 0
      if (h == 0) gm[j] = d * rl;  // L_jj
    }
  }
}

// k_bsigma (last beta-iteration only): sigma_best when argmin is a new
// sample -- its sigma coordinate drawn with the NEW generators (Q4,
// compute_beta.py:133-145): y_M = mean_M + L_MM z_M + u_M . sum_{j<M} w_j z_j
// the body of k_bsigma for candidate b when its argmin is a new sample;
// red: (kThreads / 64) * 11 doubles of LDS.  The sums are split over
// kThreads threads whatever the workgroup size (the threads beyond add
// nothing), so every caller forms the same bits.
DEVI void bsigma_body(const Params& p, int tb, int b, double* red) {
  const int M = p.M, tid = tidx();
  const int imin = p.bimin[b];
  const double* gen = p.gen + size_t(b) * pos_pad(M) * kGenStride;
  {
    const float* z = p.beta_z + size_t(tb) * pos_pad(M) * kBzCols;
    const int si = imin - kBetaElite;
    double part[11];
#pragma unroll
    for (int a = 0; a < 11; ++a) part[a] = 0.0;
    for (int j = tid; j < M && tid < kThreads; j += kThreads) {
      const double zj = double(z[bz_index(j, si)]);
#pragma unroll
      for (int a = 0; a < 11; ++a) part[a] += gen[size_t(j) * kGenRow + kGenW + a] * zj;
    }
#pragma unroll
    for (int a = 0; a < 11; ++a) {
      part[a] = wave_total(part[a]);
    }
    __syncthreads();
    if ((tid & 63) == 0 && tid < kThreads)
#pragma unroll
      for (int a = 0; a < 11; ++a) red[(tid >> 6) * 11 + a] = part[a];
    __syncthreads();
    if (tid == 0) {
      // u_M and the mean's slot of the NEW generators (this iteration's k_belite)
      const float* EM = gen_elites(p, tb + 1, b) + M;
      const double mM = gen_mean_row(p, b)[M];
      double d = 0.0;
      for (int a = 0; a < 11; ++a) {
        double sa = 0.0;
        for (int w2 = 0; w2 < kThreads / 64; ++w2) sa += red[w2 * 11 + a];
        d += gen_u(EM[size_t(a) * (M + 1)], mM) * sa;
      }
      const double zM = z[bz_index(M, si)];
      const float yM = float((gen_mean_slot(mM) + p.genm[size_t(b) * pos_pad(M) + M] * zM) + d);
      p.sigma[b] = fmaxf(yM, 0.01f);
    }
  }
}

}  // namespace

}  // namespace mpcmmd
