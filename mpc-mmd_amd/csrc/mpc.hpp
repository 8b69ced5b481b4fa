// The synthetic closed loop on the device: what k_mpc.hip (the kernel) and
// mpc_api.hip (the entry points) share.  Internal to the library.
#pragma once
#include <hip/hip_runtime.h>

#include "mpc_queue.hpp"
#include "mpc_step.hpp"
#include "mpc_vehicle.hpp"

namespace mpcmmd {

constexpr int kMpcThreads = 256;

// k_mpc_step's arguments: the model's arrays, then the per-episode arrays of
// mpcmmd_mpc_step_io with a leading episode axis, all device pointers.  The
// plan's episode stride (in floats) is spelled out: the harness gives dense
// arrays, the chained route (mpc_api.hip) the handle's result buffer.  The
// tracks go to x_obs / y_obs [E][O][100] (the harness) or, first H points
// only, to obs [E][2][O][H] (the handle's buffer); solve_c is written where
// kcol is given.
struct MpcStepParams {
  MpcScalars w;
  int tick;
  int reset;                       // 1: every episode as if frozen, no controller, no log row, done untouched
  int s_plan;                      // stride of cx / cy
  int H;                           // points of a track in obs
  const uint32_t* key;             // [E] episode keys of the drawn variates (u null), with seed
  uint32_t seed;
  const double *pdot2, *pddot1, *chol;  // [2][11], [11], [8][8]
  const double* kcol;              // [4][11][4] KKT coefficient columns (solve_columns), or null
  const float* pop0;               // [B][8]
  const float *cx, *cy, *u, *mean;  // [E][11] (stride s_plan), [E][3] or null (drawn), [E][8]
  double* pos;                     // [E][2]
  float* vel;                      // [E][3]
  float* veh;                      // [E][O][4]
  int32_t* done;                   // [E]
  float *init, *st0, *pop;         // [E][6], [E][8], [E][B][8]
  float *x_obs, *y_obs;            // [E][O][100], or null
  float* obs;                      // [E][2][O][H], or null
  double* solve_c;                 // [E][4][11] (with kcol)
  double* logd;                    // [E][2]
  float* logf;                     // [E][12]
  int32_t* logi;                   // [E][4]
  float* plan;                     // [E][30] cx, cy, mean: the chained route's log of the plan, or null
  // the scene queue's instantiations only
  const int32_t* ltick;            // [E] each slot's own tick, in place of `tick`
  const int32_t* fresh;            // [E] or null: a slot whose word is < 0 is left alone (the masked reset)
};

// The planned instantiation's further arguments: the
// constants in device memory and the per-episode arrays of mpcmmd_mpc_planned.
struct MpcVehParams {
  MpcVehConsts k;
  float* acc;           // [E][O][2]
  const float* target;  // [E][O][2]
  float* log;           // [E][O][6], or null
};

void launch_mpc_step(const MpcStepParams& q, int episodes, hipStream_t s);
void launch_mpc_step_planned(const MpcStepParams& q, const MpcVehParams& pv, int episodes, hipStream_t s);
// the same two steps with a tick per slot (q.ltick) and the mask (q.fresh)
void launch_mpc_step_queue(const MpcStepParams& q, int episodes, hipStream_t s);
void launch_mpc_step_planned_queue(const MpcStepParams& q, const MpcVehParams& pv, int episodes, hipStream_t s);

// k_mpc_queue's arguments: the rule's words (mpc_queue.hpp), the step's log_i row of this tick, the
// scene table and the slots' state it refills.  The state tables are null in the harness.
struct MpcQueueParams {
  MpcQueueState st;
  int E, N, ticks_per_episode, tick, O;
  const int32_t* flags;        // [E][4]
  const uint32_t* tab_key;     // [N]
  const float* tab_v_des;      // [N]
  const double* tab_pos;       // [N][2], or null: no state is copied
  const float *tab_vel, *tab_veh, *tab_mean;  // [N][3], [N][O][4], [N][8]
  const float *tab_target, *tab_acc;          // [N][O][2] each, or null (no planned policy)
  double* pos;                 // [E][2]
  float *vel, *veh, *mean;     // [E][3], [E][O][4], [E][8] (the handle's mean)
  float *target, *acc;         // [E][O][2]
};

void launch_mpc_queue(const MpcQueueParams& p, hipStream_t s);

}  // namespace mpcmmd
