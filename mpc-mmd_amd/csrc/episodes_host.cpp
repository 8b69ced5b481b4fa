// libmpcmmd: the HIP-free parts of the episode contexts' host layer (episodes_host.hpp).
#include "episodes_host.hpp"

#include <cmath>
#include <cstring>
#include <string>

#include "host_api.hpp"

namespace mpcmmd {

int check_risk_config(const char* prefix, int32_t R, float alpha, int32_t S, const float* sigma, int32_t* lo,
                      int32_t* hi, float* w_lo, float* w_hi) {
  const std::string p = std::string(prefix) + " validation: ";
  if (R < 1 || R > (1 << 20)) return fail(MPCMMD_E_INVALID, p + "num_rollouts out of 1..2^20");
  if (!(alpha >= 0.0f && alpha <= 1.0f)) return fail(MPCMMD_E_INVALID, p + "alpha out of [0, 1]");
  if (S < 0 || S > kRiskSigmaSlots) return fail(MPCMMD_E_INVALID, p + "num_sigma out of [0, 8]");
  for (int i = 0; i < S; ++i)
    if (!(std::isfinite(sigma[i]) && sigma[i] > 0.0f))
      return fail(MPCMMD_E_INVALID, p + "every sigma must be finite and > 0");
  if (mpcmmd_quantile_position(R, alpha, lo, hi, w_lo, w_hi) != MPCMMD_OK)
    return fail(MPCMMD_E_INVALID, p + "quantile position");
  return MPCMMD_OK;
}

void tick_indices(int32_t tick, const std::vector<uint32_t>& keys, int32_t* idx) {
  for (size_t e = 0; e < keys.size(); ++e) idx[e] = int32_t(uint32_t(tick) + keys[e]);
}

std::vector<float> replicate_cov(const float* cov, int E) {
  std::vector<float> covs(size_t(E) * 64);
  for (int e = 0; e < E; ++e) std::memcpy(&covs[size_t(e) * 64], cov, 64 * 4);
  return covs;
}

void interleave_risk_log(size_t n, int n_counts, const int32_t* planes, const float* stat_planes, int32_t* counts,
                         float* stats) {
  const size_t nc = size_t(n_counts);
  for (size_t i = 0; i < n; ++i)
    for (size_t k = 0; k < nc; ++k) counts[i * nc + k] = planes[k * n + i];
  for (size_t i = 0; i < n; ++i)
    for (size_t k = 0; k < 4; ++k) std::memcpy(stats + (i * 4 + k) * 3, &stat_planes[(k * n + i) * 3], 12);
}

}  // namespace mpcmmd
