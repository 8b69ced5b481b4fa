// The world context's validation stage: what
// k_world_validate.hip (the kernel) and world_api.hip (the entry points)
// share.  Internal to the library.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace mpcmmd {

constexpr int kWorldValidateThreads = 256;

// k_world_validate_prep's arguments, all device pointers: the solve's results
// and the tick's inputs as the handle and the tick context hold them (with
// their episode strides in floats), then the packed inputs of
// launch_validate_carla (ValidateCarlaParams) with a leading episode axis.
struct WorldValidateParams {
  int H, O, P, tick;
  const double* pd;         // [100][11] the fp64 Pdot of plan_speed
  const float* res;         // the last iteration's result row of episode 0: cx [11], cy [11], cost_lane, cost_obs
  int s_res;
  const float* res_steer;   // the last iteration's steering [100] of episode 0
  int s_steer;
  const float* in;          // the tick context's input image: init_state [6] at the head of each tick
  int s_in;
  const float* path_in;     // [E][6][kMaxPath]
  const float* obs;         // [E][2][O][H]
  const uint32_t* key;      // [E] episode keys
  float* acc;               // [E][H]
  float* steer;             // [E][H]
  float* st0;               // [E][8]
  float* path;              // [E][6][P]
  float* x_obs;             // [E][O][100], columns >= H zero
  float* y_obs;
  uint32_t* keys;           // [E] tick + key
  float* est;               // [E][2] the solve's own cost_lane, cost_obs (the tick's log row)
};

void launch_world_validate_prep(const WorldValidateParams& q, int episodes, hipStream_t s);

}  // namespace mpcmmd
