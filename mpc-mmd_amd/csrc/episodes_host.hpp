// The parts of the episode contexts' host layer (episodes.hpp) that touch no
// HIP call: compiled by g++ and built a second time under ASan/UBSan
// (tests/native/asan_host.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace mpcmmd {

constexpr int kRiskSigmaSlots = 8;  // sigma[8] of mpcmmd_world_validation / mpcmmd_mpc_validation

// the checks of a validation stage's num_rollouts, alpha, num_sigma and sigma[]: MPCMMD_OK and the
// quantile's order statistics and fp32 weights (mpcmmd_quantile_position of R, alpha), or
// MPCMMD_E_INVALID with "<prefix> validation: ..." recorded
__attribute__((visibility("hidden"))) int check_risk_config(const char* prefix, int32_t R, float alpha, int32_t S,
                                                             const float* sigma, int32_t* lo, int32_t* hi, float* w_lo,
                                                             float* w_hi);

// idx[e] = tick + keys[e] in 32-bit wrap-around arithmetic: episode e's idx_mpc of a tick
__attribute__((visibility("hidden"))) void tick_indices(int32_t tick, const std::vector<uint32_t>& keys, int32_t* idx);
// cov [8][8] once per episode: [E][64]
__attribute__((visibility("hidden"))) std::vector<float> replicate_cov(const float* cov, int E);

// The validation log's read-back order: `planes` holds n_counts arrays of n words one after the
// other (count, count_lane[, count_rows]), `stat_planes` four of n x 3 (var, cvar, mean, max);
// counts [n][n_counts] and stats [n][4][3] take them row by row.
__attribute__((visibility("hidden"))) void interleave_risk_log(size_t n, int n_counts, const int32_t* planes,
                                                               const float* stat_planes, int32_t* counts,
                                                               float* stats);

}  // namespace mpcmmd
