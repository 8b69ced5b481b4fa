// k_bdist, k_dist_pad, k_bmoment, k_bmoment_rows: the mother distance matrix
// and the series records of its rows, once per outer iteration
// (betacem_common.hpp has the pipeline).
#include "betacem_common.hpp"

namespace mpcmmd {

namespace {

// k_bdist: the L1 distance matrix of the mother features,
// D[a][b] = sum_f |F_a,f - F_b,f| (kernel_computation.py:33-39 with the
// 22-dim features of compute_beta.py:120-124), once per outer iteration.
// Every K_mixed / K_red entry the 20 beta-iterations need is exp(-D[a][b] /
// sigma) for a selected row a, so the rows are computed once here instead
// of 20 times.  Workgroup = (candidate, tile of kDistRows rows); a thread
// owns one column (its 22 features in registers), the tile's row features
// are LDS broadcasts; the feature sum is sequential (the oracle's order).
// Pad columns M..Md-1 hold +inf so exp2(-inf) = 0 in the row sums (written
// once per handle by k_dist_pad).
constexpr int kDistRows = 32;
constexpr int kDistThreads = 256;

// XCD-aware tile order: workgroups are dealt round-robin to the 8 XCDs by
// linear id, so id L runs on XCD L % 8.  Candidate b's row tiles get ids
// ((b / 8) * T + tile) * 8 + b % 8: all on one XCD and launched together, so
// the candidate's column features (42 KB) are read from HBM once and then
// hit that XCD's L2, instead of once per tile (kXcds: betacem_common.hpp).
//
// The matrix is symmetric and |a - b| == |b - a| exactly, so a tile of rows
// computes only the columns from its own first row on and also writes the
// mirrored entries D[j][r0 .. r0 + 31] of every later column j: half the
// VALU work of the full matrix, same bits.  The mirrored 32-entry pieces go
// through LDS, so each store instruction writes whole 128-byte rows (eight
// lanes per row) instead of 16 bytes to 64 rows.
constexpr int kMirrorPitch = kDistRows + 4;  // floats per staged row (16-byte aligned, spreads banks)

__global__ __launch_bounds__(kDistThreads) void k_bdist(Params p) {
  __shared__ __attribute__((aligned(16))) float Fr[kDistRows][kF + 2];
  __shared__ __attribute__((aligned(16))) float Tm[kDistThreads * kMirrorPitch];
  const int M = p.M, Md = dist_stride(M), T = (M + kDistRows - 1) / kDistRows;
  const int L = blockIdx.x, q = L / kXcds;
  const int b = (q / T) * kXcds + L % kXcds, r0 = (q % T) * kDistRows;
  if (b >= p.Bt) return;
  const int tid = tidx();
  const float* Fg = p.feat + size_t(b) * kF * M;
  for (int i = tid; i < kDistRows * kF; i += kDistThreads) {
    const int r = i / kF, f = i - r * kF;
    Fr[r][f] = r0 + r < M ? Fg[f * M + r0 + r] : 0.0f;
  }
  __syncthreads();
  const int rn = min(kDistRows, M - r0);
  float* Db = p.bdist + size_t(b) * M * Md;
  float* D = Db + size_t(r0) * Md;
  // a later real column exists only if this tile is full (r0 + 32 < M)
  for (int j0 = r0; j0 < Md; j0 += kDistThreads) {  // wave-uniform trip count
    const int j = j0 + tid;
    if (j < Md) {
      float fj[kF];
      const int jc = min(j, M - 1);
#pragma unroll
      for (int f = 0; f < kF; ++f) fj[f] = Fg[f * M + jc];
      for (int rg = 0; rg < kDistRows / 4; ++rg) {
        float dv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          const int r = 4 * rg + rr;
          if (r < rn) {
            const float* fr = Fr[r];  // wave-uniform: LDS broadcast
            // the differences two features at a time (v_pk_add_f32: the same
            // roundings as two v_sub_f32), the sum sequential as before
            static_assert(kF % 2 == 0, "feature pairs");
            f2 df = f2{fr[0], fr[1]} - f2{fj[0], fj[1]};
            float d = fabsf(df.x);
            d = d + fabsf(df.y);
#pragma unroll
            for (int f = 2; f < kF; f += 2) {
              df = f2{fr[f], fr[f + 1]} - f2{fj[f], fj[f + 1]};
              d = d + fabsf(df.x);
              d = d + fabsf(df.y);
            }
            if (j < M) D[size_t(r) * Md + j] = d;  // pad columns: +inf once per handle (k_dist_pad)
            dv[rr] = d;
          }
        }
        *reinterpret_cast<float4*>(&Tm[tid * kMirrorPitch + 4 * rg]) = make_float4(dv[0], dv[1], dv[2], dv[3]);
      }
    }
    __syncthreads();
    // rows j0 + c (c < 256) of the mirror: 8 lanes per row, 16 bytes each
    for (int i = tid; i < kDistThreads * (kDistRows / 4); i += kDistThreads) {
      const int c = i >> 3, part = i & 7, jj = j0 + c;
      if (jj >= r0 + kDistRows && jj < M)
        *reinterpret_cast<float4*>(Db + size_t(jj) * Md + r0 + 4 * part) =
            *reinterpret_cast<const float4*>(&Tm[c * kMirrorPitch + 4 * part]);
    }
    __syncthreads();
  }
}

// k_bmoment: the series record of every distance row (once per outer
// iteration, after k_bdist).  A K_mixed row sum of sample s over the mother
// set (kernel_computation.py:33-39, 45; compute_beta.py:75) is
//   S(r, c) = sum_j exp(-c D[r][j]),  c = 1 / sigma_s.
// With R = max_j D[r][j] / 2, t_j = D[r][j] / R - 1 in [-1, 1] and a = c R,
//   S = exp(-a) sum_j exp(-a t_j) = exp(-a) sum_{k < 12} (-a)^k / k! P_k + E,
//   P_k = sum_j t_j^k,   |E| / S <= e^{2a} a^12 / 12!
// (each term's Taylor remainder is <= a^12 e^a / 12! while each term is
// >= e^-a), i.e. <= 1.5e-8 for a <= 1: below half an fp32 ulp, so the
// series is as exact as the reference's fp32 exponentials and sum.  P_k
// depends on the row only; k_bkernel then pays a 12-term Horner sum per
// (sample, row) pair instead of M exponentials (pairs with a > 1 are summed
// directly).  One wave per row: the row as float4s in registers, the row max
// by DPP, t and its powers in packed fp32 (the column pairs of a float4 as
// one v_pk_* operand), one wave sum per moment.  Pad columns (+inf) count 0.
// The first beta-iteration's pairs of the row (Params::rp0, the handle's
// table) whose a > 1 are summed here directly, from the row already in
// registers, instead of re-reading it in k_bdirect.
constexpr int kMomRowsPerBlock = 4;

// one distance row (global row index gw over the launch's candidates) held in x
// Its first-iteration pairs: rpair0[q0 .. q1), lane L's record of the first 64
// (pr) loaded with the row, ahead of it.
struct RowPairs {
  int q0, q1;
  int2 pr;
};

DEVI RowPairs load_row_pairs(const Params& p, int r) {
  const int lane = tidx() & 63;
  RowPairs rp;
  rp.q0 = p.rp0[r];
  rp.q1 = p.rp0[r + 1];
  rp.pr = p.rpair0[max(min(rp.q0 + lane, rp.q1 - 1), 0)];  // a row without pairs reads a valid record, unused
  return rp;
}

// The per-lane part of a first-iteration direct row sum (bmoment_row and
// bmoment_row16): the lane's NV float4s of the row as exp2(D * cs), cs =
// -log2 e / sigma (pad columns: +inf * cs = -inf -> 0), added in sequence to
// one packed accumulator.  Not betacem_kernel.hpp's pair_terms, which keeps
// two accumulators and adds them at the end (half the length of the add
// chain): that is the order of the later iterations' sums (k_bdirect and
// k_bdirect_pairs, bit-equal to each other), this the order of the first
// iteration's.  Both stay, since moving either to the other's order changes
// the bits of its row sums.
template <int NV>
DEVI float row_terms(const float4 (&x)[NV], float cs) {
  const f2 c2 = {cs, cs};
  f2 acc = {0.0f, 0.0f};
#pragma unroll
  for (int t = 0; t < NV; ++t) {
    const f2 t0 = f2{x[t].x, x[t].y} * c2, t1 = f2{x[t].z, x[t].w} * c2;
    acc += f2{__builtin_amdgcn_exp2f(t0.x), __builtin_amdgcn_exp2f(t0.y)};
    acc += f2{__builtin_amdgcn_exp2f(t1.x), __builtin_amdgcn_exp2f(t1.y)};
  }
  return acc.x + acc.y;
}

template <int NV4>
DEVI void bmoment_row(const Params& p, int gw, const float4 (&x)[NV4], const RowPairs& rq) {
  const int lane = tidx() & 63;
  const int M = p.M;
  const int b = gw / M, r = gw - b * M;
  // columns j = 4 (lane + 64 t) + c; pad columns j >= M
  auto valid = [&](int t, int c) { return 4 * (lane + 64 * t) + c < M; };
  float mx = 0.0f;
#pragma unroll
  for (int t = 0; t < NV4; ++t) {
    if (valid(t, 0)) mx = fmaxf(mx, x[t].x);
    if (valid(t, 1)) mx = fmaxf(mx, x[t].y);
    if (valid(t, 2)) mx = fmaxf(mx, x[t].z);
    if (valid(t, 3)) mx = fmaxf(mx, x[t].w);
  }
  const float R = 0.5f * wave_max(mx);
  const float invR = R > 0.0f ? 1.0f / R : 0.0f;  // R = 0: every t = -1, every a = 0
  f2 acc[kMom - 1];
#pragma unroll
  for (int k = 0; k < kMom - 1; ++k) acc[k] = f2{0.0f, 0.0f};
#pragma unroll
  for (int t = 0; t < NV4; ++t) {
    const float e[4] = {x[t].x, x[t].y, x[t].z, x[t].w};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const float t0 = valid(t, 2 * h) ? fmaf(e[2 * h], invR, -1.0f) : 0.0f;
      const float t1 = valid(t, 2 * h + 1) ? fmaf(e[2 * h + 1], invR, -1.0f) : 0.0f;
      const f2 tt = {t0, t1};
      f2 pw = tt;
#pragma unroll
      for (int k = 0; k < kMom - 1; ++k) {
        acc[k] += pw;
        if (k + 1 < kMom - 1) pw *= tt;
      }
    }
  }
  static_assert(kMomStride == 16 && kMomR < 16 && kMom == kMomR, "record slots");
  float v[16];  // slot k + 1 of the record: P_{k+1}
#pragma unroll
  for (int k = 0; k < 16; ++k) v[k] = k >= 1 && k < kMom ? acc[k - 1].x + acc[k - 1].y : 0.0f;
  const int slot = lane >> 2;  // lanes 4 s .. 4 s + 3 hold slot s
  float rec = wave_totals16(v);
  if (slot == 0) rec = float(M);
  if (slot == kMomR) rec = R;
  if ((lane & 3) == 0) p.bmom[(size_t(b) * M + r) * kMomStride + slot] = rec;
  // first-iteration pairs of this row that the series does not cover (the
  // test is k_bkernel's, on the same R and sigma)
  const int n = p.n;
  float* rowsum = p.brow + size_t(b) * kBetaSamples * n;
  const int q0 = rq.q0, q1 = rq.q1;
  for (int c0 = q0; c0 < q1; c0 += 64) {  // one (index, sigma) record per lane
    const int2 pr = c0 == q0 ? rq.pr : p.rpair0[min(c0 + lane, q1 - 1)];
    const int il = pr.x;
    const float sl = __int_as_float(pr.y);
    const bool dl = !(double(R) * (1.0 / double(sl)) <= p.mom_amax) && c0 + lane < q1;
    unsigned long long todo = __ballot(dl);
    while (todo) {  // wave-uniform
      const int j = __builtin_ctzll(todo);
      todo &= todo - 1;
      const int i = __builtin_amdgcn_readlane(il, j);
      const float sg = readlane(sl, j);
      const float cs = kNegLog2e / sg;
      const float sum = wave_total(row_terms<NV4>(x, cs));
      if (lane == 0) rowsum[i] = sum;
    }
  }
}

// rows per wave: the next row's loads are issued before the current row is
// processed (a wave no longer waits one full memory latency per row)
template <int NV4>
constexpr int mom_rows_per_wave() { return NV4 <= 2 ? 4 : (NV4 <= 4 ? 2 : 1); }

template <int NV4>
__global__ __launch_bounds__(64 * kMomRowsPerBlock) void k_bmoment(Params p) {
  constexpr int RPW = mom_rows_per_wave<NV4>();
  const int lane = tidx() & 63;
  const int total = p.Bt * p.M, Md = dist_stride(p.M);
  const int g0 = (blockIdx.x * kMomRowsPerBlock + (tidx() >> 6)) * RPW;
  if (g0 >= total) return;  // wave-uniform
  auto load = [&](float4 (&x)[NV4], int g) {
    const float4* row = reinterpret_cast<const float4*>(p.bdist + size_t(g) * Md) + lane;  // rows of all candidates are consecutive
#pragma unroll
    for (int t = 0; t < NV4; ++t) x[t] = row[64 * t];
  };
  const int M = p.M;
  float4 x[NV4], xn[NV4];
  RowPairs rq = load_row_pairs(p, g0 % M), rqn;
  load(x, g0);
#pragma unroll
  for (int i = 0; i < RPW; ++i) {
    const int g = g0 + i;
    if (g >= total) break;  // wave-uniform
    if (i + 1 < RPW) {  // the next row's pair records, then its distances
      const int gn = min(g + 1, total - 1);
      rqn = load_row_pairs(p, gn % M);
      load(xn, gn);
    }
    bmoment_row<NV4>(p, g, x, rq);
    if (i + 1 < RPW) {
      rq = rqn;
#pragma unroll
      for (int t = 0; t < NV4; ++t) x[t] = xn[t];
    }
  }
}

// k_bmoment_rows: the same series records (and first-iteration direct sums)
// with a distance row on one 16-lane DPP row instead of a whole wave: four
// rows per wave, NV float4s (4 NV columns) per lane.  The per-row work that
// does not scale with the row length -- the maximum, the division, the
// totals of the eleven moments, the record store -- is then shared by four
// times the columns per lane: 16-lane reductions (two quad_perm and two
// row_ror DPP steps) instead of 64-lane ones, and the eleven totals by one
// transposing butterfly over the row (row_mirror, row_half_mirror and the
// two quad pairings: lane l ends with slot l of the record).  Same values as
// bmoment_row up to the summation order of the moments and direct sums.
// Columns j = 4 (l + 16 t) + c, l = lane & 15.
template <int NV>
DEVI void bmoment_row16(const Params& p, int g, bool live, const float4 (&x)[NV], int q0, int q1) {
  const int l = tidx() & 15, grp = (tidx() & 63) >> 4;
  const int M = p.M;
  const int b = g / M;
  // M > dist_stride(M) - 256, so the columns of t < NV - 4 are all real; only
  // the last four float4s of a lane can hold pad columns (+inf)
  auto sure = [](int t) { return t < NV - 4; };
  auto valid = [&](int t, int c) { return sure(t) || 4 * (l + 16 * t) + c < M; };
  // the row maximum on the bit patterns: distances are >= +0 (sums of fabsf),
  // where unsigned order is float order (and no canonicalising v_max per
  // element).  A NaN distance (NaN features) now makes R NaN where fmaxf
  // skipped it; its row's sums are NaN either way (t = NaN for that column)
  auto key = [](float v) { return __float_as_uint(v); };
  uint32_t mb = 0u;
#pragma unroll
  for (int t = 0; t < NV; ++t) {
    const float e[4] = {x[t].x, x[t].y, x[t].z, x[t].w};
#pragma unroll
    for (int c = 0; c < 4; ++c) mb = max(mb, valid(t, c) ? key(e[c]) : 0u);
  }
  const float R = 0.5f * row16_max(__uint_as_float(mb));
  const float invR = R > 0.0f ? 1.0f / R : 0.0f;  // R = 0: every t = -1, every a = 0
  f2 acc[kMom - 1];
#pragma unroll
  for (int k = 0; k < kMom - 1; ++k) acc[k] = f2{0.0f, 0.0f};
#pragma unroll
  for (int t = 0; t < NV; ++t) {
    const float e[4] = {x[t].x, x[t].y, x[t].z, x[t].w};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const float t0 = valid(t, 2 * h) ? fmaf(e[2 * h], invR, -1.0f) : 0.0f;
      const float t1 = valid(t, 2 * h + 1) ? fmaf(e[2 * h + 1], invR, -1.0f) : 0.0f;
      const f2 tt = {t0, t1};
      f2 pw = tt;
#pragma unroll
      for (int k = 0; k < kMom - 1; ++k) {
        acc[k] += pw;
        if (k + 1 < kMom - 1) pw *= tt;
      }
      // one column pair's powers at a time (left to itself the scheduler
      // interleaves all of them: 230 VGPRs)
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  float v[16];  // slot k + 1 of the record: P_{k+1}
#pragma unroll
  for (int k = 0; k < 16; ++k) v[k] = k >= 1 && k < kMom ? acc[k - 1].x + acc[k - 1].y : 0.0f;
  float rec = row16_totals16(v);
  if (l == 0) rec = float(M);
  if (l == kMomR) rec = R;
  if (live) p.bmom[size_t(g) * kMomStride + l] = rec;
  // first-iteration pairs of this row that the series does not cover (k_bkernel's
  // test, on the same R and sigma: about 3/4 of the pairs on real distances),
  // each 16-lane row on its own records, one distinct sigma per round, the
  // wave looping while any row has one left (a whole wave per pair would need
  // the rows in LDS: 32-64 KB per workgroup, measured slower)
  const int n = p.n;
  float* rowsum = p.brow + size_t(b) * kBetaSamples * n;
  int nmax = q1 - q0;
  nmax = max(nmax, __shfl_xor(nmax, 16));
  nmax = max(nmax, __shfl_xor(nmax, 32));
  for (int c0 = 0; c0 < nmax; c0 += 16) {  // wave-uniform
    const int c = q0 + c0 + l;
    const bool have = c < q1;
    const int2 pr = p.rpair0[have ? c : max(q0, 0)];
    const int il = pr.x;
    const float sl = __int_as_float(pr.y);
    bool todo = have && !(double(R) * (1.0 / double(sl)) <= p.mom_amax);
    while (__ballot(todo)) {  // wave-uniform
      const unsigned field = unsigned(__ballot(todo) >> (16 * grp)) & 0xFFFFu;
      const int j = field ? __builtin_ctz(field) : 0;
      const int src = 16 * grp + j;
      const float sg = __int_as_float(__shfl(__float_as_int(sl), src));
      const float cs = kNegLog2e / sg;
      const float sum = row16_total(row_terms<NV>(x, cs));
      // every pair of the row with this sigma (the first iteration's samples
      // share sigma = 0.01, the clip, about half of them) takes the same sum
      const bool same = todo && __float_as_uint(sl) == __float_as_uint(sg);
      if (field && same) rowsum[il] = sum;
      if (field && same) todo = false;
    }
  }
}

constexpr int kMomRowWaves = 4;  // waves per k_bmoment_rows workgroup

// four rows per wave and nothing else: measured against 2-16 four-row passes
// per wave with the next pass's rows in flight (0.306 vs 0.318-0.363 ms per
// configs[1] step), more resident waves hide the row loads better than a
// prefetch within each
template <int NV>
__global__ __launch_bounds__(64 * kMomRowWaves) void k_bmoment_rows(Params p) {
  const int l = tidx() & 15;
  const int total = p.Bt * p.M, Md = dist_stride(p.M), M = p.M;
  const int w = blockIdx.x * kMomRowWaves + (tidx() >> 6);
  if (w * 4 >= total) return;  // wave-uniform
  // position gp of the candidates' rows in pair-count order (Params::rperm): the
  // wave's four rows carry nearly the same number of first-iteration pairs
  const int gp = w * 4 + ((tidx() & 63) >> 4);
  // positions past the end (the last wave's) compute on a clamped row, store nothing
  const bool live = gp < total;
  const int gpc = live ? gp : total - 1, bc = gpc / M, r = p.rperm[gpc - bc * M], gc = bc * M + r;
  const float4* row = reinterpret_cast<const float4*>(p.bdist + size_t(gc) * Md) + l;
  float4 x[NV];
#pragma unroll
  for (int t = 0; t < NV; ++t) x[t] = row[16 * t];
  const int q0 = live ? p.rp0[r] : 0, q1 = live ? p.rp0[r + 1] : 0;
  bmoment_row16<NV>(p, gc, live, x, q0, q1);
}

}  // namespace

// the pad columns M..Md-1 of every distance row, +inf (exp(-inf) = 0 in the
// row sums): once per handle, k_bdist writes the real columns only
__global__ __launch_bounds__(256) void k_dist_pad(Params p, int cap) {
  const int M = p.M, Md = dist_stride(M), np = Md - M;
  const size_t total = size_t(cap) * M * np;
  for (size_t x = size_t(blockIdx.x) * 256 + tidx(); x < total; x += size_t(gridDim.x) * 256) {
    const size_t row = x / np;
    p.bdist[row * Md + M + (x - row * np)] = __builtin_inff();
  }
}

void launch_dist_pad(const Params& p, int cap, hipStream_t s) {
  if (dist_stride(p.M) == p.M) return;
  hipLaunchKernelGGL(k_dist_pad, dim3(2048), dim3(256), 0, s, p, cap);
}

void launch_bdist(const Params& p, hipStream_t s) {
  const int T = (p.M + kDistRows - 1) / kDistRows, groups = (p.Bt + kXcds - 1) / kXcds;
  hipLaunchKernelGGL(k_bdist, dim3(groups * T * kXcds), dim3(kDistThreads), 0, s, p);
}

template <int NV4>
void launch_bmoment_v(const Params& p, hipStream_t s) {
  const size_t rows = size_t(p.Bt) * p.M, per = size_t(kMomRowsPerBlock) * mom_rows_per_wave<NV4>();
  hipLaunchKernelGGL((k_bmoment<NV4>), dim3((rows + per - 1) / per),
                     dim3(64 * kMomRowsPerBlock), 0, s, p);
}

template <int NV>
void launch_bmoment_rows(const Params& p, hipStream_t s) {
  const size_t rows = size_t(p.Bt) * p.M, per = size_t(kMomRowWaves) * 4;
  hipLaunchKernelGGL((k_bmoment_rows<NV>), dim3((rows + per - 1) / per), dim3(64 * kMomRowWaves), 0, s, p);
}

void launch_bmoment(const Params& p, hipStream_t s) {
  if (p.mom_rows) {
    switch (dist_stride(p.M) >> 8) {  // 16 lanes x NV float4s = one row of dist_stride(M) columns
      case 1:
        return launch_bmoment_rows<4>(p, s);
      case 2:
        return launch_bmoment_rows<8>(p, s);
      case 3:
        return launch_bmoment_rows<12>(p, s);
      case 4:
        return launch_bmoment_rows<16>(p, s);
      default:
        break;
    }
  }
  with_dist_blocks(p.M, [&](auto v) { launch_bmoment_v<decltype(v)::value>(p, s); });
}

}  // namespace mpcmmd
