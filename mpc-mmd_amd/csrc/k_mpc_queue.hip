// k_mpc_queue: the scene queue of the synthetic closed loop (DESIGN.md section
// 25), one workgroup of 256 threads, launched once per lockstep tick behind
// k_mpc_step.  Every decision is mpc_queue.hpp's, shared with the host twin
// (mpcmmd_mpc_queue_host); the kernel only finds each slot's rank and spreads
// the copies:
//   1  wave 0, a lane per slot in chunks of 64: the ended slots' ballot, a
//      slot's rank = the chunks' carry + the set bits below its lane; the
//      slot's words (scene, ltick, done, fresh, key, idx_mpc, v_des) and its
//      scenes' schedule rows; lane 0: the counters
//   2  all threads, an element per thread: the state of every slot that took a
//      scene, from the scene table (pos, vel, the vehicles, the start mean and,
//      with the planned policy, the accelerations and targets)
// Deterministic by construction: one workgroup, no atomics.  The tables are
// null in the one-launch harness (mpcmmd_mpc_queue_device): phase 1 only.
#include "lanes.hpp"
#include "mpc.hpp"

namespace mpcmmd {

namespace {

// dst[e][k] = tab[fresh[e]][k] for every slot that took a scene
template <class T>
DEVI void queue_rows(T* dst, const T* tab, const int32_t* fresh, int E, int width, int tid) {
  for (int i = tid; i < E * width; i += kMpcThreads) {
    const int e = i / width, s = fresh[e];
    if (s >= 0) dst[i] = tab[size_t(s) * width + (i - e * width)];
  }
}

__global__ __launch_bounds__(kMpcThreads) void k_mpc_queue(const MpcQueueParams p) {
  const int tid = threadIdx.x, lane = tid & 63;
  if (tid < 64) {  // 1
    const int started = p.st.count[0];
    int carry = 0;
    for (int base = 0; base < p.E; base += 64) {
      const int e = base + lane;
      const bool ended = e < p.E && queue_ended(p.st.scene[e], p.st.done[e], p.st.ltick[e], p.ticks_per_episode);
      const unsigned long long b = __ballot(ended);
      const int rank = carry + __popcll(b & ((1ull << lane) - 1ull));
      if (e < p.E)
        queue_slot(p.st, e, p.tick, p.ticks_per_episode, p.N, started, rank, p.flags + size_t(e) * 4, p.tab_key,
                   p.tab_v_des);
      carry += __popcll(b);
    }
    if (lane == 0) queue_counters(p.st.count, p.N, carry);
  }
  __threadfence_block();
  __syncthreads();
  if (!p.tab_pos) return;
  // 2
  const int32_t* fresh = p.st.fresh;
  queue_rows(p.pos, p.tab_pos, fresh, p.E, 2, tid);
  queue_rows(p.vel, p.tab_vel, fresh, p.E, 3, tid);
  queue_rows(p.mean, p.tab_mean, fresh, p.E, 8, tid);
  queue_rows(p.veh, p.tab_veh, fresh, p.E, p.O * 4, tid);
  if (p.tab_target) {
    queue_rows(p.target, p.tab_target, fresh, p.E, p.O * 2, tid);
    queue_rows(p.acc, p.tab_acc, fresh, p.E, p.O * 2, tid);
  }
}

}  // namespace

void launch_mpc_queue(const MpcQueueParams& p, hipStream_t s) {
  hipLaunchKernelGGL(k_mpc_queue, dim3(1), dim3(kMpcThreads), 0, s, p);
}

}  // namespace mpcmmd
