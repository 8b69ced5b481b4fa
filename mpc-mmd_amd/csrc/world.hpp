// The surrogate world on the device: what k_world.hip (the kernel) and
// world_api.hip (the entry point) share.  Internal to the library.
#pragma once
#include <hip/hip_runtime.h>

#include "world_step.hpp"
#include "world_vehicle.hpp"

namespace mpcmmd {

constexpr int kWorldThreads = 256;

// k_world_step's arguments: the model's arrays, then the per-episode arrays
// of mpcmmd_world_step_io with a leading episode axis, all device pointers.
// The plan and the next tick's inputs have their episode strides (in floats)
// spelled out: the harness gives dense arrays, the chained route (world_api.hip)
// the handle's result buffers and the tick context's input image.
struct WorldStepParams {
  WorldScalars w;
  int tick;
  int reset;                        // 1: every episode as if frozen, no log row, done untouched (tick 0's inputs)
  int s_plan, s_steer;              // strides of cx / cy and of steer
  int s_init, s_wp, s_obs;          // strides of init, of xw / yw and of obs
  float* st0;                       // [E][8] the handle's st0 through initial_state's formula, or null
  const uint32_t* key;              // [E] episode keys of the drawn variates (u null), with seed
  uint32_t seed;
  float* plan;                      // [E][34] cx, cy, steer[4], mean: the chained route's log of the plan, or null
  const double *route_x, *route_y, *arc, *sx, *sy;  // [n_route], splines [4][n_route - 1]
  const double *pdot4, *chol;                       // [4][11], [8][8]
  const float* pop0;                                // [B][8]
  const float *cx, *cy, *steer, *u, *mean;          // [E][11], [E][11], [E][4], [E][4] or null (drawn), [E][8]
  double* pos;                                      // [E][2]
  float* ego;                                       // [E][3]
  float* veh;                                       // [E][total][5]
  int32_t* done;                                    // [E]
  float *init, *xw, *yw, *obs, *pop;                // [E][6], [E][P], [E][P], [E][O][5], [E][B][8]
  double* logd;                                     // [E][3]
  float* logf;                                      // [E][13]
  int32_t* logi;                                    // [E][4]
};

// The vehicle policy k_world_step is instantiated on.  Constant velocity: the rows of q.veh move by
// (vx, vy) dt and carry no further state.
struct WorldConstantVelocity {};

// Routed (world_vehicle.hpp): the arrays of mpcmmd_world_routed with a leading episode axis, device pointers.
struct WorldRoutedParams {
  VehScalars p;
  double* s;           // [E][total]
  float* v;            // [E][total]
  const float* param;  // [E][total][2] d, v0
  float* log;          // [E][total][2] v, a of this step, or null
  double* log_s;       // [E][total] s after this step (the chained route's vehicle log), or null
};

void launch_world_step(const WorldStepParams& q, int episodes, hipStream_t s);
void launch_world_step_routed(const WorldStepParams& q, const WorldRoutedParams& r, int episodes, hipStream_t s);

}  // namespace mpcmmd
