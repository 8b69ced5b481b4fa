// Sanitizer harness of the surrogate world's host step (csrc/world_host.cpp,
// check_world and world_step_host, what mpcmmd_world_step_host chains), built by
// `make -C mpc-mmd_amd asan_world` from the host-only sources with
// -fsanitize=address,undefined -fno-sanitize-recover and run by
// tests/test_world_host.py as a child process.  A straight route of 40 points
// (x = arc, y = 0, so its spline pieces are written down, not fitted), 3
// vehicles of which one ends up behind the ego, num_path 5, 2 obstacles, a
// population of 4: five chained ticks on exact-size heap arrays, so any read
// or write past an array is an ASan report.  Per tick it prints
//   tick <k> <sum of the fp32 outputs' words, 8 hex digits> <x> <idx>
// which the test compares with the library's host step on the same inputs.
// Then the worlds at the edge: no vehicle, 64 vehicles with 64 obstacles, a
// frozen episode, and the argument errors.  "ok" and exit status 0 on success.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/mpcmmd.h"
#include "../../mpc-mmd_amd/csrc/world_host.hpp"

// what mpcmmd_world_step_host chains (the entry point itself lives in a HIP source, for the drawn
// variates; here u is always given)
static int step(const mpcmmd_world_model* m, int32_t tick, const mpcmmd_world_step_io* io) {
  if (int rc = mpcmmd::check_world(m, io)) return rc;
  mpcmmd::world_step_host(*m, tick, *io);
  return MPCMMD_OK;
}

static void expect(bool ok, const char* what, int a = 0) {
  if (ok) return;
  std::printf("FAILED %s (%d)\n", what, a);
  std::exit(1);
}

struct World {
  int R, P, O, T, B;
  std::vector<double> rx, ry, arc, sx, sy, pd, chol;
  std::vector<float> pop0;
  mpcmmd_world_model m{};
  World(int R_, int P_, int O_, int T_, int B_) : R(R_), P(P_), O(O_), T(T_), B(B_) {
    rx.resize(R), ry.assign(R, 0.0), arc.resize(R);
    sx.assign(size_t(4) * (R - 1), 0.0), sy.assign(size_t(4) * (R - 1), 0.0);
    for (int i = 0; i < R; ++i) rx[i] = arc[i] = 2.0 * i;
    for (int i = 0; i < R - 1; ++i) sx[size_t(2) * (R - 1) + i] = 1.0, sx[size_t(3) * (R - 1) + i] = rx[i];
    pd.assign(44, 0.0);
    for (int i = 0; i < 4; ++i) pd[i * 11 + 1] = 1.0;
    chol.assign(64, 0.0);
    for (int i = 0; i < 8; ++i) chol[i * 8 + i] = 2.0;
    pop0.resize(size_t(B) * 8);
    for (int i = 0; i < B * 8; ++i) pop0[i] = (float(i) - 16.0f) / 8.0f;
    m.num_path = P, m.num_obs = O, m.total_obs = T, m.num_route = R, m.goal_index = R - 1, m.num_batch = B;
    m.noise = 0, m.dt = 0.05f, m.sigma_acc = 0.2f, m.sigma_steer = 0.1f, m.acc_const = 0.05f, m.steer_const = 0.01f;
    m.steer_max = 0.6f, m.a_obs = 4.5f, m.b_obs = 3.0f, m.y_lb = -2.5f, m.y_ub = 6.0f;
    m.route_x = rx.data(), m.route_y = ry.data(), m.route_arc = arc.data(), m.spline_x = sx.data();
    m.spline_y = sy.data(), m.pdot4 = pd.data(), m.chol = chol.data(), m.pop0 = pop0.data();
  }
};

struct Episode {
  std::vector<float> cx, cy, steer, u, mean, ego, veh, init, xw, yw, obs, pop, lf;
  std::vector<double> pos, ld;
  std::vector<int32_t> done, li;
  mpcmmd_world_step_io io{};
  explicit Episode(const World& w)
      : cx(11, 0.0f), cy(11, 0.0f), steer(4, 0.05f), u{0.5f, -0.25f, 1.0f, -1.0f}, mean(8), ego{2.0f, 0.1f, 0.0f},
        veh(size_t(w.T) * 5, 0.0f), init(6), xw(w.P), yw(w.P), obs(size_t(w.O) * 5), pop(size_t(w.B) * 8),
        lf(MPCMMD_WORLD_LOG_F), pos{1.0, 0.5}, ld(MPCMMD_WORLD_LOG_D), done(1, -1), li(MPCMMD_WORLD_LOG_I) {
    cx[1] = 6.0f;
    for (int i = 0; i < 8; ++i) mean[i] = float(i + 1);
    io.cx = cx.data(), io.cy = cy.data(), io.steer = steer.data(), io.u = u.data(), io.mean = mean.data();
    io.pos = pos.data(), io.ego = ego.data(), io.vehicles = w.T ? veh.data() : nullptr, io.done_tick = done.data();
    io.init_state = init.data(), io.x_wp = xw.data(), io.y_wp = yw.data(), io.obstacles = obs.data();
    io.pop = pop.data(), io.log_d = ld.data(), io.log_f = lf.data(), io.log_i = li.data();
  }
  uint32_t checksum() const {
    uint32_t s = 0;
    for (const std::vector<float>* v : {&init, &xw, &yw, &obs, &pop, &lf})
      for (float f : *v) {
        uint32_t b;
        std::memcpy(&b, &f, 4);
        s += b;
      }
    return s;
  }
};

int main() {
  {
    World w(40, 5, 2, 3, 4);
    Episode e(w);
    const float veh[3][5] = {{20, 1, -1, 0, 0.2f}, {-10, 0, 0, 0, 0}, {30, -2, 0, 0.5f, 3.0f}};
    std::memcpy(e.veh.data(), veh, sizeof veh);
    for (int k = 0; k < 5; ++k) {
      expect(step(&w.m, k, &e.io) == MPCMMD_OK, "step status", k);
      std::printf("tick %d %08x %.17g %d\n", k, e.checksum(), e.pos[0], e.li[0]);
    }
    expect(e.pos[0] > 1.0 && e.done[0] == -1, "the ego moved and nothing ended the episode");
  }
  {  // no vehicle: both obstacles are the placeholders 300 m away
    World w(40, 2, 2, 0, 1);
    Episode e(w);
    expect(step(&w.m, 0, &e.io) == MPCMMD_OK, "no vehicles");
    expect(e.obs[0] == float(300.0 - e.pos[0]) && e.obs[5] == e.obs[0] && e.li[2] == 0, "placeholders");
  }
  {  // 64 vehicles on a line ahead, 64 obstacles; the second tick finds the episode frozen by a collision
    World w(40, 2048, 64, 64, 3);
    Episode e(w);
    for (int o = 0; o < 64; ++o) e.veh[size_t(o) * 5] = 2.0f + float(63 - o), e.veh[size_t(o) * 5 + 1] = 0.5f;
    expect(step(&w.m, 3, &e.io) == MPCMMD_OK, "64 vehicles");
    expect(e.li[2] == 1 && e.done[0] == 3, "collision ends the episode");
    for (int o = 1; o < 64; ++o) expect(e.obs[size_t(o) * 5] > e.obs[size_t(o - 1) * 5], "sorted by distance", o);
    const std::vector<double> pos = e.pos;
    const std::vector<float> veh = e.veh, xw = e.xw;
    expect(step(&w.m, 4, &e.io) == MPCMMD_OK, "frozen");
    expect(pos == e.pos && veh == e.veh && xw == e.xw && e.done[0] == 3, "a frozen episode does not change");
  }
  {
    World w(40, 5, 2, 3, 4);
    Episode e(w);
    expect(step(nullptr, 0, &e.io) == MPCMMD_E_INVALID, "null model");
    expect(step(&w.m, 0, nullptr) == MPCMMD_E_INVALID, "null io");
    mpcmmd_world_model bad = w.m;
    bad.num_path = 2049;
    expect(step(&bad, 0, &e.io) == MPCMMD_E_INVALID, "num_path 2049");
    bad = w.m, bad.total_obs = 65;
    expect(step(&bad, 0, &e.io) == MPCMMD_E_INVALID, "total_obs 65");
    bad = w.m, bad.goal_index = 40;
    expect(step(&bad, 0, &e.io) == MPCMMD_E_INVALID, "goal_index past the route");
    mpcmmd_world_step_io io = e.io;
    io.x_wp = nullptr;
    expect(step(&w.m, 0, &io) == MPCMMD_E_INVALID, "null x_wp");
  }
  std::printf("ok\n");
  return 0;
}
