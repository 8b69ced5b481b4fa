// The receding-horizon world of the synthetic variants:
// the host twin of k_mpc_step.  One step of one episode over plain arrays, from
// the expressions of mpc_step.hpp; the argument checks the device entry points
// (mpc_api.hip) share; and the planned vehicles of section 23 (mpc_vehicle.hpp).
// No HIP: compiled by g++ and built a second time under ASan/UBSan
// (tests/native/asan_mpc.cpp, asan_mpc_vehicles.cpp).
#pragma once
#include "../../include/mpcmmd.h"
#include "host_constants.hpp"
#include "mpc_step.hpp"
#include "mpc_vehicle.hpp"

namespace mpcmmd {

MpcScalars mpc_scalars(const mpcmmd_mpc_model& m);

// MPCMMD_OK, or the error of a model or an io that no step may run on (io.u or io.key must be given)
int check_mpc_model(const mpcmmd_mpc_model* m);
int check_mpc(const mpcmmd_mpc_model* m, const mpcmmd_mpc_step_io* io);

// The variates u[3] of (key, seed, tick) once a_c and s_c are known: mpc_draw.hpp's, handed in as a
// function because the Philox streams live in a HIP header this file's compiler does not read.
using MpcDraw = void (*)(int noise, uint32_t key, uint32_t seed, int tick, float a_c, float s_c, float* u);

// The planned vehicles' constants for one tick length: the dynamic
// driver's QP (built once per process) and the basis rows at double(dt).  Throws for dt outside (0, 15).
struct MpcVehTables {
  const DynObsConsts* qp;
  std::vector<double> adv;  // [3][11]
  MpcVehConsts view() const;
};
MpcVehTables mpc_vehicle_tables(float dt);

// MPCMMD_OK, or the error of a policy no step may run with (m checked before: check_mpc)
int check_mpc_planned(const mpcmmd_mpc_model* m, const mpcmmd_mpc_planned* pl);

// One episode's step: io's arrays are those of that episode.  io.u null: the variates are drawn
// with `draw` from (io.key[0], m.seed, tick).  pl and vc given: the vehicles follow their re-planned
// QP (mpc_vehicle.hpp) in place of the constant-velocity step.
void mpc_step_host(const mpcmmd_mpc_model& m, int tick, const mpcmmd_mpc_step_io& io, MpcDraw draw = nullptr,
                   const mpcmmd_mpc_planned* pl = nullptr, const MpcVehConsts* vc = nullptr);

}  // namespace mpcmmd
