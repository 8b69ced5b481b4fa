// The surrogate world of a closed CARLA loop: the host
// twin of k_world_step.  One step of one episode over plain arrays, from the
// expressions of world_step.hpp; the argument checks the device entry point
// (world_api.hip) shares.  No HIP: compiled by g++ and built a second time
// under ASan/UBSan (tests/native/asan_world.cpp).
#pragma once
#include "../../include/mpcmmd.h"
#include "world_step.hpp"
#include "world_vehicle.hpp"

namespace mpcmmd {

WorldScalars world_scalars(const mpcmmd_world_model& m);

// MPCMMD_OK, or the error of a model or an io that no step may run on
int check_world(const mpcmmd_world_model* m, const mpcmmd_world_step_io* io);  // io.u or io.key must be given

// The variates u[4] of (key, seed, tick) once a_c and s_c are known: world_draw.hpp's, handed in as a
// function because the Philox streams live in a HIP header this file's compiler does not read.
using WorldDraw = void (*)(int noise, uint32_t key, uint32_t seed, int tick, float a_c, float s_c, float* u);

// the routed vehicles' scalars, and MPCMMD_OK or the error of a policy no step may run on
VehScalars veh_scalars(const mpcmmd_world_routed& r);
int check_world_routed(const mpcmmd_world_model* m, const mpcmmd_world_routed* rt);

// One episode's step: io's arrays are those of that episode.  io.u null: the variates are drawn
// with `draw` from (io.key[0], m.seed, tick).  rt: the vehicles are routed (world_vehicle.hpp), rt's
// arrays those of the episode; tick < 0 is then the reset-mode step.
void world_step_host(const mpcmmd_world_model& m, int tick, const mpcmmd_world_step_io& io, WorldDraw draw = nullptr,
                     const mpcmmd_world_routed* rt = nullptr);

}  // namespace mpcmmd
