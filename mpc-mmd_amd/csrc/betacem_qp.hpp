// The beta-CEM QP's device code (k_bqp.hip, k_bcem_small.hip).
//
// k_bqp: compute_beta_reduced (compute_beta.py:70-91) for every sample:
// C = K_red + 0.05 I, C x1 = g, C x2 = 1, beta = x1 + ((1 - sum x1) / sum x2) x2
// (the (n+1) KKT system).  The factorisation and the solves are fp32, the
// reference's precision (jnp.linalg.solve on fp32, compute_beta.py:79); the
// cost beta^T K beta - 2 g^T beta is accumulated in fp64 from the fp32 beta
// and the re-read K_red, so it carries no factorisation error.
//
// A quad (4 lanes) per QP, 16 QPs per wave: lane q owns rows i = 4t + q of
// the (padded to NP) matrix, in registers.  Right-looking Cholesky; the
// column entries every lane needs are quad broadcasts (DPP quad_perm, no
// LDS, no barriers); the triangular solves are a row sweep (forward, quad
// broadcast of y_j) and a column sweep (backward, quad sum of partials).
// Entries above the diagonal are kept at exactly 0, padding rows are
// identity with zero right-hand sides.
#pragma once
#include "betacem_common.hpp"

namespace mpcmmd {

namespace {

// 1 / sqrt(x): v_rsq_f32 and one Newton step
DEVI float rsqrt_nr(float x) {
  const float y = __builtin_amdgcn_rsqf(x);
  return y * fmaf(-0.5f * x, y * y, 1.5f);
}

// zero floats after the staged triangles (bqp_solve's padding rows and
// reads past a row end: at most NP - 1 <= 31 floats past a triangle)
constexpr int kQpZeros = 64;

// K_red of the workgroup's QPs is staged in LDS first (consecutive
// threads copy consecutive entries of one QP's triangle: coalesced), so the
// per-lane row gathers of the factorisation and the cost read LDS, not
// scattered global lines.
DEVI void bqp_stage(const Params& p, int tb, float* kl) {
  const int n = p.n;
  const int s_lo = first_sample(tb), per = kBetaSamples - s_lo;
  const int ntri = tri_stride(n), n4 = ntri >> 2;
  const int nq = blockDim.x >> 2, q0 = blockIdx.x * nq, total = p.nb * per;
  {  // the workgroup's K_red rows as float4s, consecutive threads on consecutive
     // float4s, every thread's loads issued before its first LDS store (one
     // memory latency, not one per four rows).  QP g = q0 + j (clamped to the
     // last) is sample s0 + j of candidate c0 while s0 + j < per, else sample
     // s0 + j - per of candidate c0 + 1 (nq < per): its triangle is the
     // (j + (j >= jw ? s_lo : 0))-th past the first one's.  Float4 (j, r) of
     // the staging advances by (T / n4, T % n4) per round of T threads.
    const int c0 = q0 / per, s0 = q0 - c0 * per, jw = per - s0, jmax = min(nq, total - q0) - 1;
    const float4* src = reinterpret_cast<const float4*>(p.bkred + (size_t(p.b0 + c0) * kBetaSamples + s_lo + s0) * ntri);
    float4* kl4 = reinterpret_cast<float4*>(kl);
    const int T = blockDim.x, dj = T / n4, dr = T - dj * n4;
    int j = int(tidx()) / n4, r = int(tidx()) - j * n4;
    constexpr int kU = 16;  // float4s per thread and round: 32 QPs x 58 float4s fit one round at n = 22
    for (int i0 = 0; i0 < nq * n4; i0 += kU * T) {
      float4 v[kU];
      int jj[kU], rr[kU];
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        jj[u] = j;
        rr[u] = r;
        const int jc = min(j, jmax);
        v[u] = src[(jc + (jc >= jw ? s_lo : 0)) * n4 + r];
        j += dj;
        r += dr;
        if (r >= n4) {
          r -= n4;
          ++j;
        }
      }
#pragma unroll
      for (int u = 0; u < kU; ++u)
        if (jj[u] < nq) kl4[jj[u] * n4 + rr[u]] = v[u];
    }
    if (int(tidx()) < kQpZeros) kl[nq * ntri + tidx()] = 0.0f;  // the padding rows' zeros
    __syncthreads();
  }
}

// QP of sample s of candidate b on the calling quad (lane q = tidx() & 3),
// its K_red strict lower triangle at kr (LDS staging); zr: kQpZeros zero
// floats (the padding rows' entries), placed right after the last staged
// triangle, so every read past a row end -- masked, never used -- lands on
// K_red entries or zeros; ok = false: compute on the clamped inputs, store
// nothing
template <int NP>
DEVI void bqp_solve(const Params& p, int b, int s, bool ok, const float* kr, const float* zr) {
  constexpr int T4 = NP / 4;
  const int n = p.n, M = p.M, q = tidx() & 3;
  const float* br = p.brow + (size_t(b) * kBetaSamples + s) * n;
  const double inv_m = double(1.0f / float(M));
  const float cdiag = 1.0f + 0.05f;
  // row i = 4t+q of K_red (k_bkernel's strict lower triangle: entry (i, k < i)
  // at i (i-1)/2 + k), read at constant offsets k <= 4t+3 past the row start
  // (entries k >= i are the next row's or zeros, masked); padding rows i >= n
  // read zeros
  const float* rowp[T4];
#pragma unroll
  for (int t = 0; t < T4; ++t) {
    const int i = 4 * t + q;
    rowp[t] = i < n ? kr + i * (i - 1) / 2 : zr;
  }
  // own rows: A[t][k] = C[4t+q][k], k <= 4t+3; loaded as K_red (every load
  // unconditional, so they are all in flight together), factored in place
  float A[T4][NP];
  float a1[T4], a2[T4], rin[T4];
#pragma unroll
  for (int t = 0; t < T4; ++t) {
#pragma unroll
    for (int k = 0; k < NP; ++k)
      if (k <= 4 * t + 3) A[t][k] = rowp[t][k];
    const int i = 4 * t + q;
    const float g = float(double(br[min(i, n - 1)]) * inv_m);
    a1[t] = i < n ? g : 0.0f;
    a2[t] = i < n ? 1.0f : 0.0f;
    rin[t] = 0.0f;
  }
  // C in place: strict lower part from K_red, the diagonal 1.05 (1 for the
  // padding rows), entries above the diagonal 0
#pragma unroll
  for (int t = 0; t < T4; ++t)
#pragma unroll
    for (int k = 0; k <= 4 * t + 3; ++k) {
      const int i = 4 * t + q;
      float v = k < i ? A[t][k] : 0.0f;  // padding rows: zeros
      if (k == i) v = i < n ? cdiag : 1.0f;
      A[t][k] = v;
    }
  // Cholesky, right-looking: column k scaled by 1 / sqrt(C_kk), then the
  // trailing columns c > k updated (every update of a step independent)
#pragma unroll
  for (int k = 0; k < NP; ++k) {
    const int tk = k >> 2, qk = k & 3;
    const float sv = quad_bcast(A[tk][k], qk);  // the pivot, from the lane owning row k
    const float y = rsqrt_nr(sv);
    if (q == qk) rin[tk] = y;
#pragma unroll
    for (int t = tk; t < T4; ++t) {
      const float v = A[t][k] * y;
      A[t][k] = t > tk ? v : (q > qk ? v : (q == qk ? sv * y : 0.0f));
    }
#pragma unroll
    for (int c = k + 1; c < NP; ++c) {
      const int tc = c >> 2;
      const float lck = quad_bcast(A[tc][k], c & 3);  // L_ck from the lane owning row c
      // rows (t, t + 1), t even, as packed pairs (v_pk_fma_f32: two fmaf)
      int t = tc;
      if (t & 1) {
        A[t][c] = fmaf(-A[t][k], lck, A[t][c]);
        ++t;
      }
#pragma unroll
      for (; t + 1 < T4; t += 2) {
        const f2 x = __builtin_elementwise_fma(f2{-A[t][k], -A[t + 1][k]}, f2{lck, lck}, f2{A[t][c], A[t + 1][c]});
        A[t][c] = x.x;
        A[t + 1][c] = x.y;
      }
      if (t < T4) A[t][c] = fmaf(-A[t][k], lck, A[t][c]);
    }
  }
  // forward: L y = (g, 1)
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    const int tj = j >> 2, qj = j & 3;
    const float y1 = a1[tj] * rin[tj], y2 = a2[tj] * rin[tj];
    if (q == qj) {
      a1[tj] = y1;
      a2[tj] = y2;
    }
    const float b1 = quad_bcast(y1, qj), b2 = quad_bcast(y2, qj);
#pragma unroll
    for (int t = tj; t < T4; ++t) {
      const float lij = (t == tj && q <= qj) ? 0.0f : A[t][j];
      a1[t] = fmaf(-lij, b1, a1[t]);
      a2[t] = fmaf(-lij, b2, a2[t]);
    }
  }
  // C^-1 = L^-T L^-1, so with y1 = L^-1 g, y2 = L^-1 1: sum x1 = y2 . y1,
  // sum x2 = |y2|^2 and beta = L^-T (y1 + alpha y2) -- one backward sweep
  float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
  for (int t = 0; t < T4; ++t) {  // padding rows hold y = 0
    s1 = fmaf(a2[t], a1[t], s1);
    s2 = fmaf(a2[t], a2[t], s2);
  }
  s1 = quad_sum(s1);
  s2 = quad_sum(s2);
  const float alpha = (1.0f - s1) / s2;
#pragma unroll
  for (int t = 0; t < T4; ++t) a1[t] = fmaf(alpha, a2[t], a1[t]);
  // backward: L^T beta = y1 + alpha y2 (beta overwrites it row by row, last row first)
#pragma unroll
  for (int j = NP - 1; j >= 0; --j) {
    const int tj = j >> 2, qj = j & 3;
    float p1 = 0.0f;
#pragma unroll
    for (int t = tj; t < T4; ++t) {
      const float lij = (t == tj && q <= qj) ? 0.0f : A[t][j];
      p1 = fmaf(lij, a1[t], p1);
    }
    p1 = quad_sum(p1);
    if (q == qj) a1[tj] = (a1[tj] - p1) * rin[tj];
  }
  float bf[T4];
#pragma unroll
  for (int t = 0; t < T4; ++t) bf[t] = 4 * t + q < n ? a1[t] : 0.0f;
  // cost = beta^T K beta - 2 g^T beta in fp64, K = K_red re-read (unit
  // diagonal): r_i = sum_{k<i} K_ik beta_k by columns k, column k + 1's
  // entries in flight while column k is summed (two columns live, not the
  // whole triangle); row i contributes beta_i (beta_i + 2 r_i).  An entry
  // outside the triangle is a zero (padding rows) or masked to zero (k >= i
  // in the diagonal block), and fma(0, beta_k, r) = r: the masked sum's bits
  double r[T4];
  float kc[T4], kn[T4];
#pragma unroll
  for (int t = 0; t < T4; ++t) {
    r[t] = 0.0;
    kc[t] = rowp[t][0];
  }
#pragma unroll
  for (int k = 0; k < NP; ++k) {
#pragma unroll
    for (int t = (k + 1) >> 2; t < T4; ++t) kn[t] = rowp[t][min(k + 1, NP - 1)];
    __builtin_amdgcn_sched_barrier(0);
    const double bk = double(quad_bcast(bf[k >> 2], k & 3));
#pragma unroll
    for (int t = k >> 2; t < T4; ++t) {
      const float kv = t == (k >> 2) && !(k < 4 * t + q) ? 0.0f : kc[t];
      r[t] = fma(double(kv), bk, r[t]);
      kc[t] = kn[t];
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  double c1 = 0.0, c3 = 0.0;
#pragma unroll
  for (int t = 0; t < T4; ++t) {
    const int i = 4 * t + q;
    const double bi = double(bf[t]);
    c1 = fma(bi, fma(2.0, r[t], bi), c1);
    c3 = fma(i < n ? double(br[min(i, n - 1)]) * inv_m : 0.0, bi, c3);
  }
  c1 = quad_sum(c1);
  c3 = quad_sum(c3);
  if (!ok) return;
  float* bt = p.btop + (size_t(b) * kBetaSamples + s) * n;
#pragma unroll
  for (int t = 0; t < T4; ++t)
    if (4 * t + q < n) bt[4 * t + q] = bf[t];
  if (q == 0) p.bcost[size_t(b) * kBetaSamples + s] = float(c1 - 2.0 * c3);
}

template <int NP>
DEVI void bqp_quad(const Params& p, int tb, float* kl) {
  const int s_lo = first_sample(tb), per = kBetaSamples - s_lo;
  const int gq = (blockIdx.x * blockDim.x + tidx()) >> 2;
  const bool ok = gq < p.nb * per;
  const int gqc = ok ? gq : 0;
  const int b = p.b0 + gqc / per, s = s_lo + gqc % per;
  bqp_stage(p, tb, kl);
  bqp_solve<NP>(p, b, s, ok, kl + (tidx() >> 2) * tri_stride(p.n), kl + (blockDim.x >> 2) * tri_stride(p.n));
}

// padded QP size (a multiple of 4: rows 4 t + q on quad lane q).  The
// padding rows are identity rows with zero right-hand sides, whose every
// contribution to the real rows is an exact zero: any NP >= n gives the same
// bits
HDI int qp_np(int n) {
  return n <= 8 ? 8 : (n <= 12 ? 12 : (n <= 16 ? 16 : (n <= 24 ? 24 : (n <= 32 ? 32 : (n <= 48 ? 48 : 64)))));
}
// threads per workgroup: 32 QPs (their K_red in LDS: 30 KB at n = 22), 16 QPs
// for n > 24 (32 KB at n = 32, so the LDS still admits 4 workgroups per CU)
HDI_CONST int qp_threads(int np) { return np > 24 ? 64 : 128; }

}  // namespace

}  // namespace mpcmmd
