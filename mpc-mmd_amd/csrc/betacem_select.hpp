// The beta-CEM top-n selection's device code (k_bsample.hip, k_bcem_small.hip).
//
// top-n of |v_j| (j < M) in jnp.argsort order, one wave.  out[k] (k < n) are
// the indices at sorted positions M-n+k (ascending by (|v|, j)).
// Lane holds NQ keys (j = lane + 64 q).  The n-th largest key is found by
// bisection on the key bits; the counts are VALU (per-lane compares, then a
// DPP reduction of two samples' counts packed in 16-bit halves), so the
// search does not serialise on the CU's scalar unit.  The search stops as
// soon as exactly n keys lie above the candidate threshold (continuous data:
// well before the 31 steps).  Ties at the threshold go to the largest
// indices.  scratch: 2 * 64 ints of LDS owned by the wave.
#pragma once
#include "betacem_common.hpp"

namespace mpcmmd {

namespace {

template <int NQ, class V>
DEVI void load_keys(V val, int M, uint32_t* key) {
  const int lane = tidx() & 63;
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int j = lane + 64 * q;
    const float v = val(min(j, M - 1));
    key[q] = j < M ? sort_key_abs(v) : 0u;  // real keys have bit 31 set
  }
}

// Threshold search for NB samples at once (independent chains interleave):
// T[u] = the n-th largest key of sample u, or exact[u] when exactly n keys
// are >= T[u].
template <int NQ, int NB>
DEVI void find_thresholds(const uint32_t (*key)[NQ], int nb, int n, uint32_t* T, bool* exact) {
  constexpr int NP = (NB + 1) / 2;
#pragma unroll
  for (int u = 0; u < NB; ++u) {
    T[u] = 0x80000000u;  // real keys have bit 31 set, padding keys are 0
    exact[u] = u >= nb;
  }
  for (int bit = 30; bit >= 0; --bit) {
    int packed[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) packed[i] = 0;
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      if (exact[u]) continue;  // wave-uniform
      const uint32_t cand = T[u] | (1u << bit);
      int c = 0;
#pragma unroll
      for (int q = 0; q < NQ; ++q) c += key[u][q] >= cand;
      packed[u >> 1] += c << (16 * (u & 1));
    }
    bool all = true;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int tot = wave_total(packed[i]);
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int u = 2 * i + h;
        if (u >= NB || exact[u]) continue;
        const int cnt = (tot >> (16 * h)) & 0xFFFF;
        if (cnt >= n) T[u] |= 1u << bit;
        exact[u] = cnt == n;
        all = all && exact[u];
      }
    }
    if (all) break;
  }
}

// Given the threshold, write the indices of the top n keys to out[0..n) in
// jnp.argsort order (ascending key, ties by index).  Ties at a non-exact
// threshold go to the largest indices.
template <int NQ>
DEVI void emit_top(const uint32_t* key, uint32_t T, bool exact, int n, int32_t* out, int* scratch) {
  const int lane = tidx() & 63;
  int need = 0;
  unsigned long long eqm[NQ];
  if (!exact) {
    int gt = 0;
#pragma unroll
    for (int q = 0; q < NQ; ++q) gt += __popcll(__ballot(key[q] > T));
    need = n - gt;
#pragma unroll
    for (int q = 0; q < NQ; ++q) eqm[q] = __ballot(key[q] == T);
  } else {
#pragma unroll
    for (int q = 0; q < NQ; ++q) eqm[q] = 0ull;
  }
  const unsigned long long above = lane == 63 ? 0ull : (~0ull << (lane + 1));
  int* lj = scratch;
  uint32_t* lk = reinterpret_cast<uint32_t*>(scratch + 64);
  int base = 0;
  int later_eq = 0;  // equal keys in q' > q
#pragma unroll
  for (int q = 0; q < NQ; ++q) later_eq += __popcll(eqm[q]);
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    later_eq -= __popcll(eqm[q]);
    const int larger = later_eq + __popcll(eqm[q] & above);
    const bool sel = exact ? key[q] >= T : (key[q] > T || (key[q] == T && larger < need));
    const unsigned long long sm = __ballot(sel);
    if (sel) {
      const int pos = base + __popcll(sm & ((1ull << lane) - 1ull));
      lj[pos] = lane + 64 * q;
      lk[pos] = key[q];
    }
    base += __popcll(sm);
  }
  wave_sync();
  // compaction order is ascending index, so ties rank by lane
  const int j = lane < n ? lj[lane] : 0;
  const uint32_t k = lane < n ? lk[lane] : 0xFFFFFFFFu;
  int r = 0;
  for (int c = 0; c < n; ++c) {
    const uint32_t kc = __builtin_amdgcn_readlane(k, c);
    r += (kc < k) || (kc == k && c < lane);
  }
  if (lane < n) out[r] = j;
  wave_sync();
}

// Window top-n.  Given a threshold T with n <= c = #{keys >= T}, the keys
// >= T are compacted into LDS as 64-bit words (key << 32 | j), whose unsigned
// order is the jnp.argsort order (ascending |v|, ties by index); if c <= 64 R
// each lane ranks R of them exactly (one broadcast LDS read and one 64-bit
// compare per candidate, no scalar-unit chains) and the top n go to out[] in
// argsort order (out[n - 1 - rank], rank 0 = largest).  Returns false (and
// writes nothing) when c > 64 R.
template <int NQ, int R>
DEVI bool emit_window(const uint32_t* key, uint32_t T, int n, int32_t* out, unsigned long long* cand) {
  constexpr int cap = 64 * R;
  const int lane = tidx() & 63;
  const unsigned long long below = (1ull << lane) - 1ull;
  int c = 0;
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const bool sel = key[q] >= T;
    const unsigned long long m = __ballot(sel);
    const int pos = c + __popcll(m & below);
    // unconditional store: overflow and unselected lanes write the dump slot
    cand[sel && pos < cap ? pos : cap + 3] = (static_cast<unsigned long long>(key[q]) << 32) | uint32_t(lane + 64 * q);
    c += __popcll(m);
  }
  if (c > cap) return false;
  if (lane < 8) cand[c + lane] = 0ull;  // pad the reads past c (rank nothing: real keys have bit 31 set)
  wave_sync();
  unsigned long long mine[R];
  int rank[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    mine[r] = cand[lane + 64 * r];  // slots >= c are stale; never emitted
    rank[r] = 0;
  }
  const ulonglong2* c2 = reinterpret_cast<const ulonglong2*>(cand);
  for (int e = 0; e < c; e += 8) {  // four broadcast reads in flight, not one LDS latency per pair
    ulonglong2 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = c2[(e >> 1) + u];  // wave-uniform address: LDS broadcast
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int r = 0; r < R; ++r) rank[r] += int(v[u].x > mine[r]) + int(v[u].y > mine[r]);
  }
#pragma unroll
  for (int r = 0; r < R; ++r)
    if (lane + 64 * r < c && rank[r] < n) out[n - 1 - rank[r]] = int32_t(uint32_t(mine[r]));
  wave_sync();
  return true;
}

// A threshold T0 with #{keys >= T0} >= n and few keys above it: the n-th
// largest of the G group maxima (groups of 64 / G lanes; each of the n groups
// whose maximum is >= T0 holds a key >= T0).  For the top 22 of 484 keys in
// 32 lane pairs about 37 keys lie above it.  Ranks by broadcast LDS reads,
// the pick by a wave minimum; lm: G words of the wave's LDS.
template <int NQ, int G>
DEVI uint32_t group_max_threshold(const uint32_t* key, int n, uint32_t* lm) {
  const int lane = tidx() & 63;
  uint32_t m = key[0];
#pragma unroll
  for (int q = 1; q < NQ; ++q) m = max(m, key[q]);
  if constexpr (G == 32) m = max(m, dpp_old<0xB1>(m, 0u));
  if (lane % (64 / G) == 0) lm[lane / (64 / G)] = m;
  wave_sync();
  int gt = 0;
  const uint4* l4 = reinterpret_cast<const uint4*>(lm);
#pragma unroll
  for (int e = 0; e < G / 4; ++e) {
    const uint4 v = l4[e];  // broadcast
    gt += int(v.x > m) + int(v.y > m) + int(v.z > m) + int(v.w > m);
  }
  const uint32_t t = wave_min_u32(gt < n ? m : 0xFFFFFFFFu);
  wave_sync();
  return t;
}

// Top-n of the samples s = first, first + stride, ... < last, one wave, the
// next sample's keys in flight while one is ranked.  With M <= 64 R every key
// is a candidate; otherwise the window threshold comes from the group maxima
// (G = 32 lane pairs for n <= 24, 64 lanes for n <= 48).  Larger n, and ties
// so massive that the window overflows, take the exact bit bisection
// (find_thresholds) and the ballot emission (emit_top).
template <int NQ, int R, int G, class Row, class Out>
DEVI void select_walk(Row row, Out out, int first, int last, int stride, int M, int n, unsigned long long* cand,
                      uint32_t* lm, int* scratch) {
  uint32_t key[NQ], nxt[NQ];
  load_keys<NQ>(row(first), M, key);
  for (int s = first; s < last; s += stride) {
    load_keys<NQ>(row(min(s + stride, last - 1)), M, nxt);  // next sample's keys in flight
    bool done = false;
    if (M <= 64 * R)
      done = emit_window<NQ, R>(key, 0x80000000u, n, out(s), cand);  // real keys have bit 31 set
    else if (G > 0 && n <= G * 3 / 4)
      done = emit_window<NQ, R>(key, group_max_threshold<NQ, (G > 0 ? G : 64)>(key, n, lm), n, out(s), cand);
    if (!done) {
      uint32_t Tn[1];
      bool ex[1];
      find_thresholds<NQ, 1>(&key, 1, n, Tn, ex);
      emit_top<NQ>(key, Tn[0], ex[0], n, out(s), scratch);
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) key[q] = nxt[q];
  }
}

// k_bselect: top-n |beta| rows (compute_beta.py:117-118) and sigma of the
// 100 samples.  Single-wave workgroups, W = gridDim.y waves per candidate;
// wave (b, g) walks samples g, g + W, g + 2W, ... (select_walk).
// NQ = keys per lane (M <= 64 NQ), R = window capacity / 64, G = groups for
// the window threshold (0: bisection): one instantiation per size, so each
// has its own register allocation
// the samples g, g + W, ... of candidate b on the calling wave; cand [64 R +
// 8], lm [64], scratch [128]: the wave's LDS
template <int NQ, int R, int G>
DEVI void bselect_wave(const Params& p, int tb, int b, int g, int W, unsigned long long* cand, uint32_t* lm,
                       int* scratch) {
  const int M = p.M, M1 = M + 1, n = p.n;
  int32_t* sel = p.bsel + size_t(b) * kBetaSamples * n;
  float* sig = p.bsig + size_t(b) * kBetaSamples;
  const float* E = p.belite + (size_t(tb & 1) * p.Bt + b) * kBetaElite * M1;
  const int ys = ygen_stride(M);
  const float* Y = p.ygen + size_t(b) * kBzCols * ys;
  const float* z0 = p.beta_z0;
  // sample s: initial MVN(0, 20 I) draws (tb = 0, compute_beta.py:41-49), the
  // previous elites (rows 0..10) or this iteration's new samples
  auto row = [&](int s) {
    const float* r = tb == 0 ? z0 + size_t(s) * M1 : (s < kBetaElite ? E + size_t(s) * M1 : Y + size_t(s - kBetaElite) * ys);
    const bool scale = tb == 0;
    return [=](int j) { return scale ? float(kSqrt20 * double(r[j])) : r[j]; };
  };
  // samples 0..10 of iteration tb >= 1 are the previous elites, whose rows
  // and sigma k_belite carried over
  const int s_lo = first_sample(tb);
  if (s_lo + g >= kBetaSamples) return;
  select_walk<NQ, R, G>(row, [&](int s) { return sel + s * n; }, s_lo + g, kBetaSamples, W, M, n, cand, lm, scratch);
  const int lane = tidx() & 63;
  for (int s = s_lo + g + lane * W; lane < 16 && s < kBetaSamples; s += 16 * W) {
    const float v = row(s)(M);
    sig[s] = tb == 0 ? fmaxf(v, 0.01f) : v;  // later rows are clipped when written
  }
}

}  // namespace

}  // namespace mpcmmd
