// The surrogate world's perturbation variates u[4] of one (episode, tick)
// (DESIGN.md section 19), drawn where the controls are known: by thread 0 of
// k_world_step and, through a callback, by the host twin.  Philox streams of
// rng.hpp keyed (episode key, seed), element = tick.  gaussian: u0, u2, u3 are
// normals 0, 2, 3 of block `tick` of kStreamWorldNormal (u1 is normal 1,
// unused by the model: the reference draws one normal for both controls).
// beta (main_carla.py:424-433): u0 ~ Beta(2 |a_c|, 5 |a_c|), u1 ~ Beta(2 |s_c|,
// 5 |s_c|) by the validators' fp64 sampler (validate_step.hpp: beta_direct,
// with its |control| = 0 limit rule), rounded once; u2, u3 as above.
// HIP sources only (rng.hpp); host and device.
#pragma once
#include "validate_step.hpp"

namespace mpcmmd {

HDI void world_draw(int noise, uint32_t key, uint32_t seed, int tick, float a_c, float s_c, float* u) {
  double z[4];
  philox_normals4(key, seed, kStreamWorldNormal, 0u, uint32_t(tick), z);
  u[0] = float(z[0]), u[1] = float(z[1]), u[2] = float(z[2]), u[3] = float(z[3]);
  if (noise == 1) {
    const double fa = fabs(double(a_c)), fs = fabs(double(s_c));
    u[0] = float(beta_direct(2.0 * fa, 5.0 * fa, key, seed, kStreamWorldGammaAccA, kStreamWorldGammaAccB, uint32_t(tick)));
    u[1] = float(beta_direct(2.0 * fs, 5.0 * fs, key, seed, kStreamWorldGammaSteerA, kStreamWorldGammaSteerB,
                             uint32_t(tick)));
  }
}

}  // namespace mpcmmd
