// The scene queue of the synthetic closed loop, written
// once for the host twin (mpc_queue_host.cpp, g++) and the kernel
// (k_mpc_queue.hip): what happens to one slot after the step of a lockstep tick.
// Slot e carries scene[e] (a scene index, or -1: idle) and ltick[e] (the local
// tick of its episode).  Its episode has ended when done[e] >= 0 (a collision or
// the goal) or ltick[e] == ticks_per_episode - 1.  Ended slots are served in
// ascending slot order: the slot with `rank` ended slots before it takes scene
// started + rank, or becomes idle once the table is exhausted.  The two callers
// differ only in how they find `rank`: a running count (host), ballots within a
// wave and a carry across chunks of 64 slots (kernel).  No HIP header: plain C++
// with an attribute macro (world_step.hpp's).
#pragma once
#include "world_step.hpp"

namespace mpcmmd {

// end reasons of a schedule row (MPCMMD_QUEUE_* of include/mpcmmd.h)
constexpr int kQueueUnfinished = 0, kQueueCollision = 1, kQueueGoal = 2, kQueueTickLimit = 3;

// The queue's words: per slot, per scene, and the two counters.
struct MpcQueueState {
  int32_t* scene;    // [E] scene index, or -1
  int32_t* ltick;    // [E] local tick of the slot's episode
  int32_t* done;     // [E] the step's done (local tick an episode ended at, or -1)
  int32_t* fresh;    // [E] out: the scene the slot took this tick, or -1
  uint32_t* key;     // [E] episode key of the slot's scene
  int32_t* idx_mpc;  // [E] out: the next solve's idx_mpc
  float* v_des;      // [E] out: the next solve's v_des
  int32_t* sched;    // [N][4] slot, first lockstep tick, ticks run, end reason
  int32_t* count;    // [2] started, finished
};

WORLD_FN bool queue_ended(int scene, int done, int ltick, int ticks_per_episode) {
  return scene >= 0 && (done >= 0 || ltick >= ticks_per_episode - 1);
}

// flags: the step's log_i row (lane_out, collided, goal, frozen)
WORLD_FN int queue_reason(int done, const int32_t* flags) {
  return done < 0 ? kQueueTickLimit : (flags[1] ? kQueueCollision : kQueueGoal);
}

// started <= N and rank < E: no overflow
WORLD_FN int queue_next_scene(int started, int rank, int N) { return rank < N - started ? started + rank : -1; }

// tick_indices' 32-bit wrap
WORLD_FN int32_t queue_idx(int ltick, uint32_t key) { return int32_t(uint32_t(ltick) + key); }

// Slot e after the step of lockstep tick `tick`: `started` is the counter before this tick, `rank`
// the ended slots below e.  Returns whether the slot's episode ended.  A slot that takes scene s
// gets that scene's key and v_des, ltick 0 and done -1 (the caller copies the scene's state); a
// slot that ends with the table exhausted becomes idle and frozen (done >= 0); every other live
// slot advances its local tick; an idle slot keeps its words.
WORLD_FN bool queue_slot(const MpcQueueState& q, int e, int tick, int ticks_per_episode, int N, int started, int rank,
                         const int32_t* flags, const uint32_t* tab_key, const float* tab_v_des) {
  const int sc = q.scene[e], lt = q.ltick[e], dn = q.done[e];
  const bool ended = queue_ended(sc, dn, lt, ticks_per_episode);
  int fresh = -1;
  if (ended) {
    q.sched[sc * 4 + 2] = lt + 1;
    q.sched[sc * 4 + 3] = queue_reason(dn, flags);
    fresh = queue_next_scene(started, rank, N);
    q.scene[e] = fresh;
    if (fresh >= 0) {
      q.sched[fresh * 4 + 0] = e, q.sched[fresh * 4 + 1] = tick + 1;
      q.sched[fresh * 4 + 2] = 0, q.sched[fresh * 4 + 3] = kQueueUnfinished;
      q.ltick[e] = 0, q.done[e] = -1;
      q.key[e] = tab_key[fresh], q.v_des[e] = tab_v_des[fresh];
    } else if (dn < 0) {
      q.done[e] = lt;  // the tick limit with nothing left to run: frozen from here on
    }
  } else if (sc >= 0) {
    q.ltick[e] = lt + 1;
    q.sched[sc * 4 + 2] = lt + 1;  // ticks run so far: what an unfinished scene reports
  }
  q.fresh[e] = fresh;
  q.idx_mpc[e] = queue_idx(q.ltick[e], q.key[e]);
  return ended;
}

// the counters after a tick in which `ended` slots' episodes ended
WORLD_FN void queue_counters(int32_t* count, int N, int ended) {
  const int started = count[0];
  count[0] = ended < N - started ? started + ended : N;
  count[1] += ended;
}

}  // namespace mpcmmd
