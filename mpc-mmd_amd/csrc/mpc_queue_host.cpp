// libmpcmmd: the scene queue's rule on host arrays (mpc_queue.hpp, DESIGN.md
// section 25): the twin of k_mpc_queue and the argument checks its one-launch
// harness shares.  No HIP: compiled by g++ and built a second time under
// ASan/UBSan (tests/native/asan_mpc_queue.cpp).
#include "mpc_queue_host.hpp"

#include "host_api.hpp"

namespace mpcmmd {

int check_mpc_queue(const mpcmmd_mpc_queue_io* io) {
  if (!io) return fail(MPCMMD_E_INVALID, "null argument");
  if (!io->flags || !io->keys || !io->v_des || !io->scene || !io->ltick || !io->done || !io->fresh || !io->key ||
      !io->idx_mpc || !io->slot_v_des || !io->sched || !io->count)
    return fail(MPCMMD_E_INVALID, "mpc queue: null array");
  if (io->n_slots < 1 || io->n_slots > 65535) return fail(MPCMMD_E_INVALID, "mpc queue: 1 <= n_slots <= 65535");
  if (io->n_scenes < 1) return fail(MPCMMD_E_INVALID, "mpc queue: n_scenes >= 1");
  if (io->ticks_per_episode < 1) return fail(MPCMMD_E_INVALID, "mpc queue: ticks_per_episode >= 1");
  for (int e = 0; e < io->n_slots; ++e)
    if (io->scene[e] < -1 || io->scene[e] >= io->n_scenes)
      return fail(MPCMMD_E_INVALID, "mpc queue: a scene word outside -1..n_scenes-1");
  if (io->count[0] < 0 || io->count[0] > io->n_scenes) return fail(MPCMMD_E_INVALID, "mpc queue: started outside 0..n_scenes");
  return MPCMMD_OK;
}

MpcQueueState mpc_queue_state(const mpcmmd_mpc_queue_io& io) {
  return MpcQueueState{io.scene, io.ltick, io.done, io.fresh, io.key, io.idx_mpc, io.slot_v_des, io.sched, io.count};
}

void mpc_queue_host(const mpcmmd_mpc_queue_io& io) {
  const MpcQueueState q = mpc_queue_state(io);
  const int started = io.count[0];
  int rank = 0;  // ended slots so far: ascending slot order
  for (int e = 0; e < io.n_slots; ++e)
    rank += queue_slot(q, e, io.tick, io.ticks_per_episode, io.n_scenes, started, rank, io.flags + size_t(e) * 4,
                       reinterpret_cast<const uint32_t*>(io.keys), io.v_des);
  queue_counters(io.count, io.n_scenes, rank);
}

}  // namespace mpcmmd

extern "C" int mpcmmd_mpc_queue_host(const mpcmmd_mpc_queue_io* io) {
  using namespace mpcmmd;
  if (int rc = check_mpc_queue(io)) return rc;
  mpc_queue_host(*io);
  return MPCMMD_OK;
}
