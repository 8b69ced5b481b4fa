// The device buffers of a handle: the one list of record.  Each line names a
// `Params` member (kernels.hpp has its layout comment; the buffer's name in
// mpcmmd_read / mpcmmd_write / mpcmmd_buffer_info is the member's name), its
// element type, its element count over the handle's shape, the condition under
// which it exists, and the number of pieces mpcmmd_begin uploads it in through
// the pinned staging area (0: never).  mpcmmd_create_batch allocates the list
// in this order; the staging capacity is computed from it.  No HIP include:
// the sanitizer build (tests/native/asan_host.cpp) expands the list too.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "host_constants.hpp"
#include "layout.hpp"

namespace mpcmmd {

#ifndef __HIPCC__
struct int2 {  // HIP's vector type, for sizeof where no HIP header is
  int32_t x, y;
};
#endif

struct BufferShape {
  int B, S, H, O, n, M, T;
  int Gmax;  // configurations the buffers hold; candidate capacity BT = Gmax B
  int R0;    // noisy initial rows per configuration (CARLA)
  bool beta_noise, mmd_ok, carla;
  bool stampw;  // MPCMMD_STAMPW: per-workgroup phase stamps (tools/stampsw.py)
};

// X(member, element type, elements, exists, staged pieces), with the shape's
// fields and BT, G (= Gmax), M1 = M + 1, Pp = pos_pad(M) in scope.  A buffer of
// zero bytes is allocated as 16.
#define MPCMMD_BUFFERS(X)                                                          \
  /* constants (packed by solve_host.cpp) */                                       \
  X(basis, float, size_t(3) * kNum * kNvar, true, 0)                               \
  X(guess_g, double, size_t(2) * kNvar * 4, true, 0)                               \
  X(proj_m, double, size_t(2) * kNvar * kNvar, true, 0)                            \
  X(fit, double, size_t(kNvar) * H, true, 0)                                       \
  /* per configuration */                                                          \
  X(solve_c, double, G * 4 * kNvar, true, 1)                                       \
  X(obs, float, G * 2 * O * H, true, 1)                                            \
  X(st0, float, G * 8, true, 1)                                                    \
  X(idx_mpc, int32_t, G, true, 1)                                                  \
  X(v_des, float, G, true, 1)                                                      \
  X(roll, float, G * T * 3 * H * S, true, 1)                                       \
  X(resample, float, G * T * (B - kElite) * 8, true, 1)                            \
  /* Beta noise: 16-byte placeholders without it, and no attempt table */          \
  X(bplane, float, beta_noise ? BT * 2 * H * S : 4, true, 0)                       \
  X(bfix, uint32_t, beta_noise ? BT * H * S : 4, true, 0)                          \
  X(bfix_n, uint32_t, 4, true, 0)                                                  \
  X(gtab, double, G * gtab_stride(S, H), beta_noise, 0)                            \
  /* mmd_opt (beta-CEM) */                                                         \
  X(beta_z0, float, size_t(kBetaSamples) * M1, mmd_ok, 0)                          \
  X(beta_z, float, size_t(kBetaIters) * Pp * kBzCols, mmd_ok, 0)                   \
  X(feat, float, BT * 22 * M, mmd_ok, 0)                                           \
  X(featr, float, BT * M * kFeatStride, mmd_ok, 0)                                 \
  X(bmom, float, BT * M * kMomStride, mmd_ok, 0)                                   \
  X(bdflag, unsigned char, BT * kBetaSamples * n, mmd_ok, 0)                       \
  X(bdcount, int32_t, BT * kMaxSplit, mmd_ok, 0)                                   \
  X(bdlist, int32_t, BT * kBetaSamples * n, mmd_ok, 0)                             \
  X(bdlcount, int32_t, BT * kBetaIters, mmd_ok, 0)                                 \
  X(sel0, int32_t, size_t(kBetaSamples) * n, mmd_ok, 0)                            \
  X(sig0, float, size_t(kBetaSamples), mmd_ok, 0)                                  \
  X(rp0, int32_t, M1, mmd_ok, 0)                                                   \
  X(rpair0, int2, size_t(kBetaSamples) * n, mmd_ok, 0)                             \
  X(rperm, int32_t, size_t(M), mmd_ok, 0)                                          \
  X(bdist, float, BT * M * dist_stride(M), mmd_ok, 0)                              \
  X(ctrl_n, float, BT * 2 * n * H, mmd_ok, 0)                                      \
  X(bsel, int32_t, BT * kBetaSamples * n, mmd_ok, 0)                               \
  X(bsig, float, BT * kBetaSamples, mmd_ok, 0)                                     \
  X(btop, float, BT * kBetaSamples * n, mmd_ok, 0)                                 \
  X(bcost, float, BT * kBetaSamples, mmd_ok, 0)                                    \
  X(belite, float, 2 * BT * kBetaElite * M1, mmd_ok, 0)                            \
  X(gen, double, BT * Pp * kGenStride, mmd_ok, 0)                                  \
  X(genm, double, BT * Pp, mmd_ok, 0)                                              \
  X(phib, double, BT * ((M1 + 15) / 16) * 66, mmd_ok, 0)                           \
  X(bimin, int32_t, BT, mmd_ok, 0)                                                 \
  X(bestsel, int32_t, BT * n, mmd_ok, 0)                                           \
  X(brow, float, BT * kBetaSamples * n, mmd_ok, 0)                                 \
  X(bkred, float, BT * kBetaSamples * tri_stride(n), mmd_ok, 0)                    \
  X(ygen, float, BT * kBzCols * ygen_stride(M), mmd_ok, 0)                         \
  /* CARLA: det projection, path (six arrays), noisy initial rows, curvature,      \
     rollout points, steering results */                                           \
  X(proj_m_det, double, size_t(2) * kNvar * kNvar, carla, 0)                       \
  X(obs_full, float, G * 2 * O * kNum, carla, 2)                                   \
  X(path, float, G * 6 * kMaxPath, carla, 6)                                       \
  X(st0r, float, G * R0 * 8, carla, 1)                                             \
  X(kappa_i, float, BT * kNum, carla, 0)                                           \
  X(lane_des, float, BT, carla, 0)                                                 \
  X(rxy, float, BT * S * 2 * H, carla, 0)                                          \
  X(res_steer, float, G * T * kNum, carla, 0)                                      \
  /* carry / state, per-iteration intermediates */                                 \
  X(pop, float, 2 * BT * 8, true, 1)                                               \
  X(mean, float, G * 8, true, 1)                                                   \
  X(cov, float, G * 64, true, 1)                                                   \
  X(lam_x, float, BT * kNvar, true, 0)                                             \
  X(lam_y, float, BT * kNvar, true, 0)                                             \
  X(s_lane, float, BT * kLane, true, 0)                                            \
  X(cx, float, BT * kNvar, true, 0)                                                \
  X(cy, float, BT * kNvar, true, 0)                                                \
  X(traj, float, 6 * BT * kNum, true, 0)                                           \
  X(cnorm, double, BT * kCnormStride, true, 0)                                     \
  X(res_norm, float, BT, true, 0)                                                  \
  X(acc, float, BT * kNum, true, 0)                                                \
  X(steer, float, BT * kNum, true, 0)                                              \
  X(obs_cost, float, BT, true, 0)                                                  \
  X(lane_cost, float, BT, true, 0)                                                 \
  X(beta, float, BT * n, true, 0)                                                  \
  X(sigma, float, BT, true, 0)                                                     \
  X(res_beta, float, BT * kBetaIters, true, 0)                                     \
  X(btrace, float, BT * kBetaIters, true, 0)                                       \
  X(dbg, unsigned long long, 64, true, 0)                                          \
  X(dbgw, unsigned long long, size_t(65536) * 8, stampw, 0)                        \
  X(stats, unsigned long long, 8, true, 0)                                         \
  /* outputs */                                                                    \
  X(results, float, G * T * kResultStride, true, 0)                                \
  X(tr_proj, int32_t, G * T * B, true, 0)                                          \
  X(tr_obs, int32_t, G * T * kEliteCost, true, 0)                                  \
  X(tr_cem, int32_t, G * T * kElite, true, 0)

struct BufferSpec {
  const char* name;
  size_t bytes;  // 0: the buffer does not exist for this shape (its Params member is null)
  int staged;    // pieces mpcmmd_begin uploads it in through the staging area
};

// the list for one shape, in allocation order
inline std::vector<BufferSpec> buffer_specs(const BufferShape& sh) {
  const size_t B = sh.B, S = sh.S, H = sh.H, O = sh.O, n = sh.n, M = sh.M, T = sh.T, G = sh.Gmax, R0 = sh.R0;
  const size_t BT = G * B, M1 = M + 1, Pp = pos_pad(sh.M);
  const bool beta_noise = sh.beta_noise, mmd_ok = sh.mmd_ok, carla = sh.carla, stampw = sh.stampw;
  std::vector<BufferSpec> out;
#define X(name, type, count, exists, staged)                                             \
  {                                                                                      \
    const size_t bytes = size_t(count) * sizeof(type);                                   \
    out.push_back(BufferSpec{#name, (exists) ? (bytes ? bytes : size_t(16)) : 0, staged}); \
  }
  MPCMMD_BUFFERS(X)
#undef X
  return out;
}

// Bytes of pinned staging mpcmmd_begin needs at most: every staged buffer in
// full, each piece 64-byte aligned (begin fills one half of pop and G <= Gmax
// configurations, so this is an upper bound).
inline size_t staging_bytes(const std::vector<BufferSpec>& specs) {
  size_t s = 0;
  for (const BufferSpec& b : specs)
    if (b.staged && b.bytes) s += size_t(b.staged) * (((b.bytes + b.staged - 1) / b.staged + 63) & ~size_t(63));
  return s;
}

}  // namespace mpcmmd
