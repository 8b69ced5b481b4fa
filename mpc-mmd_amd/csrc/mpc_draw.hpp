// The synthetic closed loop's perturbation variates u[3] of one (episode, tick)
// (DESIGN.md section 21), drawn where the controls are known: by thread 0 of
// k_mpc_step and, through a callback, by the host twin.  Philox streams of
// rng.hpp keyed (episode key, seed), element = tick: u0, u1, u2 are normals 0,
// 1, 2 of block `tick` of kStreamMpcNormal.  beta: u0 ~ Beta(2 |a_c|, 5 |a_c|),
// u1 ~ Beta(2 |s_c|, 5 |s_c|), the optimizer's beta_pair parameters, by the
// validators' fp64 sampler (validate_step.hpp: beta_direct, with its |control|
// = 0 limit rule), rounded once; u2 as above.
// HIP sources only (rng.hpp); host and device.
#pragma once
#include "mpc_step.hpp"
#include "validate_step.hpp"

namespace mpcmmd {

HDI void mpc_draw(int noise, uint32_t key, uint32_t seed, int tick, float a_c, float s_c, float* u) {
  double z[4];
  philox_normals4(key, seed, kStreamMpcNormal, 0u, uint32_t(tick), z);
  u[0] = float(z[0]), u[1] = float(z[1]), u[2] = float(z[2]);
  if (noise == 1) {
    const double fa = fabs(double(a_c)), fs = fabs(double(s_c));
    u[0] = canon_nan(float(beta_direct(2.0 * fa, 5.0 * fa, key, seed, kStreamMpcGammaAccA, kStreamMpcGammaAccB,
                                       uint32_t(tick))));
    u[1] = canon_nan(float(beta_direct(2.0 * fs, 5.0 * fs, key, seed, kStreamMpcGammaSteerA, kStreamMpcGammaSteerB,
                                       uint32_t(tick))));
  }
}

}  // namespace mpcmmd
