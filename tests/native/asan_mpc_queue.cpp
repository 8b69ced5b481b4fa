// Sanitizer harness of the scene queue's host rule (csrc/mpc_queue_host.cpp:
// mpcmmd_mpc_queue_host over mpc_queue.hpp), built by `make -C mpc-mmd_amd
// asan_mpc_queue` from the host-only sources with -fsanitize=address,undefined
// -fno-sanitize-recover and run by tests/test_mpc_queue_host.py as a child
// process.  A campaign of 7 scenes through 3 slots of 5 ticks on exact-size heap
// arrays -- scene 1 collides and scene 3 reaches the goal at their local tick 0,
// the others run all their ticks -- so any read or write past an array is an
// ASan report.  It prints
//   ticks <lockstep ticks>
//   scene <i> <slot> <first tick> <ticks run> <end reason>      (7 lines)
// which the test compares with the NumPy rule.  Then the edges: 65 slots for one
// scene, one slot for 4 scenes with a key that wraps, and the argument errors.
// "ok" and exit status 0 on success.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/mpcmmd.h"

static void expect(bool ok, const char* what, int a = 0) {
  if (ok) return;
  std::printf("FAILED %s (%d)\n", what, a);
  std::exit(1);
}

struct Queue {
  int E, N;
  std::vector<int32_t> flags, keys, scene, ltick, done, fresh, idx, sched, count;
  std::vector<uint32_t> key;
  std::vector<float> v_des, slot_v;
  mpcmmd_mpc_queue_io io{};
  Queue(int E_, int N_, int tpe) : E(E_), N(N_) {
    const int k = E < N ? E : N;
    flags.assign(size_t(E) * 4, 0), keys.resize(N), v_des.assign(N, 15.0f);
    scene.resize(E), ltick.assign(E, 0), done.resize(E), fresh.assign(E, -1), idx.assign(E, 0);
    key.assign(E, 0), slot_v.assign(E, 15.0f), sched.assign(size_t(N) * 4, 0), count = {k, 0};
    for (int n = 0; n < N; ++n) keys[n] = 100003 * n, sched[n * 4] = n < k ? n : -1, sched[n * 4 + 1] = n < k ? 0 : -1;
    for (int e = 0; e < E; ++e) scene[e] = e < k ? e : -1, done[e] = e < k ? -1 : 0, key[e] = uint32_t(keys[e < k ? e : 0]);
    io.n_slots = E, io.n_scenes = N, io.ticks_per_episode = tpe;
    io.flags = flags.data(), io.keys = keys.data(), io.v_des = v_des.data();
    io.scene = scene.data(), io.ltick = ltick.data(), io.done = done.data(), io.fresh = fresh.data();
    io.key = key.data(), io.idx_mpc = idx.data(), io.slot_v_des = slot_v.data();
    io.sched = sched.data(), io.count = count.data();
  }
  // one lockstep tick: scene s ends at its local tick 0 where end[s] is 1 (collision) or 2 (goal)
  void tick(int t, const std::vector<int>& end) {
    for (int e = 0; e < E; ++e) {
      for (int k = 0; k < 4; ++k) flags[size_t(e) * 4 + k] = 0;
      const int s = scene[e];
      if (s >= 0 && done[e] < 0 && ltick[e] == 0 && end[s]) done[e] = 0, flags[size_t(e) * 4 + end[s]] = 1;
    }
    io.tick = t;
    expect(mpcmmd_mpc_queue_host(&io) == MPCMMD_OK, "queue_host", t);
  }
};

int main() {
  {
    Queue q(3, 7, 5);
    const std::vector<int> end = {0, 1, 0, 2, 0, 0, 0};
    int t = 0;
    while (q.count[1] < 7) {
      expect(t < 40, "the campaign ends");
      q.tick(t++, end);
      expect(q.count[0] - q.count[1] == (q.scene[0] >= 0) + (q.scene[1] >= 0) + (q.scene[2] >= 0), "live slots", t);
    }
    std::printf("ticks %d\n", t);
    for (int n = 0; n < 7; ++n)
      std::printf("scene %d %d %d %d %d\n", n, q.sched[n * 4], q.sched[n * 4 + 1], q.sched[n * 4 + 2], q.sched[n * 4 + 3]);
  }
  {  // 65 slots, one scene: 64 idle from the start, and idle after it
    Queue q(65, 1, 2);
    const std::vector<int> end = {0};
    q.tick(0, end), q.tick(1, end);
    expect(q.count[0] == 1 && q.count[1] == 1 && q.sched[2] == 2 && q.sched[3] == MPCMMD_QUEUE_TICK_LIMIT, "one scene");
    for (int e = 0; e < 65; ++e) expect(q.scene[e] == -1 && q.done[e] >= 0 && q.fresh[e] == -1, "idle", e);
    q.tick(2, end);
    expect(q.count[1] == 1, "an idle slot ends nothing");
  }
  {  // one slot, 4 scenes of one tick each; a key at the wrap
    Queue q(1, 4, 1);
    q.keys[1] = INT32_MAX, q.keys[2] = -1;
    const std::vector<int> end = {0, 0, 0, 0};
    q.tick(0, end);
    expect(q.scene[0] == 1 && q.fresh[0] == 1 && q.idx[0] == INT32_MAX && q.key[0] == 0x7FFFFFFFu, "scene 1");
    q.tick(1, end);
    expect(q.scene[0] == 2 && q.idx[0] == -1, "scene 2");
    q.tick(2, end), q.tick(3, end);
    expect(q.count[0] == 4 && q.count[1] == 4 && q.scene[0] == -1 && q.sched[3 * 4 + 1] == 3, "all four");
  }
  {  // a live slot past the wrap: idx_mpc = ltick + key in 32 bits
    Queue q(1, 1, 4);
    q.key[0] = 0xFFFFFFFFu;
    const std::vector<int> end = {0};
    q.tick(0, end);
    expect(q.idx[0] == 0 && q.ltick[0] == 1, "wrap");
  }
  {  // the argument errors
    Queue q(3, 4, 5);
    expect(mpcmmd_mpc_queue_host(nullptr) == MPCMMD_E_INVALID, "null io");
    mpcmmd_mpc_queue_io io = q.io;
    io.fresh = nullptr;
    expect(mpcmmd_mpc_queue_host(&io) == MPCMMD_E_INVALID, "null array");
    io = q.io, io.n_slots = 0;
    expect(mpcmmd_mpc_queue_host(&io) == MPCMMD_E_INVALID, "no slot");
    io = q.io, io.ticks_per_episode = 0;
    expect(mpcmmd_mpc_queue_host(&io) == MPCMMD_E_INVALID, "no tick");
    q.scene[1] = 4;
    expect(mpcmmd_mpc_queue_host(&q.io) == MPCMMD_E_INVALID, "scene out of range");
    q.scene[1] = 1, q.count[0] = 5;
    expect(mpcmmd_mpc_queue_host(&q.io) == MPCMMD_E_INVALID, "started out of range");
    expect(mpcmmd_last_error()[0] != 0, "a message");
  }
  std::printf("ok\n");
  return 0;
}
