// k_bkernel, k_bdirect, k_bdirect_pairs: the K_mixed row sums and K_red of a
// beta-iteration (betacem_kernel.hpp has the bodies).
#include <algorithm>

#include "betacem_kernel.hpp"

namespace mpcmmd {

namespace {

// two workgroups per CU: 8 waves per SIMD, which needs <= 64 VGPRs and <= 80
// SGPRs (MI355X_MICROARCH.md residency rules: 90 SGPRs admitted one)
template <bool kList>
__global__ __launch_bounds__(64 * kKerWaves) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_bkernel(Params p, int tb, int split, int scratch) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int cand = blockIdx.x / split, part = blockIdx.x - cand * split;
  bkernel_body<kList, false>(p, tb, cand, part, split, scratch, smem);
}

template <int NV4>
__global__ __launch_bounds__(64 * kDirWaves) void k_bdirect(Params p, int tb, int kparts, int split, int lpt) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int cand = blockIdx.x / split, part = blockIdx.x - cand * split;
  const int total = bdirect_total(p, p.b0 + cand, kparts);
  if (total == 0) return;  // block-uniform
  bdirect_body<NV4, kDirWaves>(p, tb, split, lpt, cand, part, total, smem);
}

// k_bdirect_pairs, workgroup = (candidate, part), kDirWaves waves each
template <int NV4, int PJ>
__global__ __launch_bounds__(64 * kDirWaves) void k_bdirect_pairs(Params p, int tb, int parts) {
  // a candidate's parts on blocks of one blockIdx % 8 (one XCD under the
  // observed round-robin dispatch, for L2 reuse of its distance rows; any
  // placement is correct): the grid is a multiple of 8, its block L of XCD
  // group x = blockIdx % 8 is the (x * grid / 8 + blockIdx / 8)-th (cand, part)
  const int per = gridDim.x >> 3, L = (blockIdx.x & 7) * per + (blockIdx.x >> 3);
  const int cand = L / parts, part = L - cand * parts;
  if (cand >= p.nb) return;
  const int b = p.b0 + cand, n = p.n;
  const int w = __builtin_amdgcn_readfirstlane(int(tidx()) >> 6);
  const int cnt = min(p.bdlcount[size_t(b) * kBetaIters + tb], kBetaSamples * n);
  if (part * kDirWaves >= (cnt + PJ - 1) / PJ) return;  // block-uniform
  if (part == 0 && tidx() == 0) atomicAdd(&p.stats[1], static_cast<unsigned long long>(cnt));
  direct_pairs_wave<NV4, PJ>(p, b, cnt, part * kDirWaves + w, parts * kDirWaves);
}

}  // namespace

bool mmdopt_supported(int n, int H, int O, std::string* why) {
  const int M = n * n;
  if (n > kMaxReduced) {
    if (why) *why = "mmd_opt needs num_reduced <= 64";
    return false;
  }
  if (dir_lds(M, n).total > kLdsBudget || ker_lds(M, n, ker_scratch(M, n, 1, ker_tab_budget(M, n))).total > kLdsBudget) {
    if (why) *why = "mmd_opt: num_reduced^2 too large for the kernel-sum stage";
    return false;
  }
  const EliteLds e = elite_lds(M + 1);
  if (e.total > kLdsBudget) {
    if (why) *why = "mmd_opt: num_reduced^2 too large for the elite stage";
    return false;
  }
  (void)H;
  (void)O;
  return true;
}

// parts per candidate: enough workgroups to fill the chip
int ker_split(int nb, int target) {
  int split = 1;
  while (split < kMaxSplit && nb * split < target) split <<= 1;
  return split;
}

// k_bdirect_pairs (and k_bkernel's pair list) for launches of <= 256
// candidates: at B = 100 the row-sorted k_bdirect's per-candidate setup
// dominates; at B = 1024 (few direct pairs) the list's atomics cost k_bkernel
// more than they save (mmd_opt 133 -> 129 steps/s), so k_bdirect stays there
bool use_pairs(const Params& p) { return p.dir_pairs && p.nb <= 256; }

void launch_bkernel(const Params& p, int tb, hipStream_t s) {
  const size_t sc = ker_scratch(p.M, p.n, p.ker_path == 1 ? 1 : tb, ker_tab_budget(p.M, p.n));
  const dim3 grid(p.nb * ker_split(p.nb, p.ker_target)), block(64 * kKerWaves);
  const size_t lds = ker_lds(p.M, p.n, sc).total;
  if (use_pairs(p))
    hipLaunchKernelGGL(k_bkernel<true>, grid, block, lds, s, p, tb, ker_split(p.nb, p.ker_target), int(sc));
  else
    hipLaunchKernelGGL(k_bkernel<false>, grid, block, lds, s, p, tb, ker_split(p.nb, p.ker_target), int(sc));
}

template <int NV4>
void launch_bdirect_v(const Params& p, int tb, int split, hipStream_t s) {
  hipLaunchKernelGGL((k_bdirect<NV4>), dim3(p.nb * split), dim3(64 * kDirWaves), dir_lds(p.M, p.n).total, s, p, tb,
                     ker_split(p.nb, p.ker_target), split, 1);
}

template <int NV4>
void launch_bdirect_pairs_v(const Params& p, int tb, hipStream_t s) {
  constexpr int PJ = direct_pj(NV4);
  const int parts = std::max(1, std::min(64, (p.dir_target + p.nb - 1) / p.nb));
  const int grid = (p.nb * parts + 7) & ~7;
  hipLaunchKernelGGL((k_bdirect_pairs<NV4, PJ>), dim3(grid), dim3(64 * kDirWaves), 0, s, p, tb, parts);
}

void launch_bdirect(const Params& p, int tb, hipStream_t s) {
  if (use_pairs(p)) return with_dist_blocks(p.M, [&](auto v) { launch_bdirect_pairs_v<decltype(v)::value>(p, tb, s); });
  const int split = ker_split(p.nb, p.dir_target);
  with_dist_blocks(p.M, [&](auto v) { launch_bdirect_v<decltype(v)::value>(p, tb, split, s); });
}

}  // namespace mpcmmd
