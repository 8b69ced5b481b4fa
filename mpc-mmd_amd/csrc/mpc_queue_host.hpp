// The scene queue of the synthetic closed loop: the host
// twin of k_mpc_queue over plain arrays, from the rule of mpc_queue.hpp, and the
// argument check the device harness (mpc_api.hip) shares.  No HIP.
#pragma once
#include "../../include/mpcmmd.h"
#include "mpc_queue.hpp"

namespace mpcmmd {

// MPCMMD_OK, or the error of arrays the rule may not run on
int check_mpc_queue(const mpcmmd_mpc_queue_io* io);

// the rule's words of io's arrays
MpcQueueState mpc_queue_state(const mpcmmd_mpc_queue_io& io);

// one lockstep tick of the rule over io's slots, in ascending slot order
void mpc_queue_host(const mpcmmd_mpc_queue_io& io);

}  // namespace mpcmmd
