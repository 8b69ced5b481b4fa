// The synthetic closed loop's validation stage: what
// k_mpc_validate.hip (the kernel) and mpc_api.hip (the entry points) share.
// Internal to the library.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace mpcmmd {

constexpr int kMpcValidateThreads = 256;

// k_mpc_validate_prep's arguments, all device pointers: the solve's results as
// the handle holds them (with their episode stride in floats), the episodes'
// state as the context holds it before the step moves it, then the packed plan
// inputs of launch_validate / launch_vrisk_roll (ValidateParams) with a leading
// episode axis.
struct MpcValidateParams {
  int H, O, tick;
  const float* res;     // the last iteration's result row of episode 0: cx [11], cy [11], cost_lane, cost_obs
  int s_res;
  const double* pos;    // [E][2] x, y
  const float* vel;     // [E][3] vx, vy, psi
  const float* obs;     // [E][2][O][H] the tick's tracks (obstacle_transpose's layout)
  const uint32_t* key;  // [E] episode keys
  double* cx;           // [E][11]
  double* cy;           // [E][11]
  double* init;         // [E][6]: float(x), float(y), vx, vy widened; words 4, 5 zero (not read)
  float* x_obs;         // [E][O][100], columns >= H zero
  float* y_obs;
  uint32_t* keys;       // [E] tick + key
  float* est;           // [E][2] the solve's own cost_lane, cost_obs (the tick's log row)
};

void launch_mpc_validate_prep(const MpcValidateParams& q, int episodes, hipStream_t s);

}  // namespace mpcmmd
