// Sanitizer harness of the synthetic closed loop's host step (csrc/mpc_host.cpp,
// check_mpc and mpc_step_host, what mpcmmd_mpc_step_host chains), built by
// `make -C mpc-mmd_amd asan_mpc` from the host-only sources with
// -fsanitize=address,undefined -fno-sanitize-recover and run by
// tests/test_mpc_host.py as a child process.  3 vehicles, a population of 4,
// a made-up basis (xd_0 = cx[1], xd_1 = cx[1] + 0.01 cx[2], xdd_0 = 0.5 cx[2]):
// five chained ticks on exact-size heap arrays, so any read or write past an
// array is an ASan report.  Per tick it prints
//   tick <k> <sum of the fp32 outputs' words, 8 hex digits> <x>
// which the test compares with the library's host step on the same inputs.
// Then the models at the edge: no vehicle, 64 vehicles of which one is hit, a
// frozen episode, a NaN plan, and the argument errors.  "ok" and exit status 0
// on success.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/mpcmmd.h"
#include "../../mpc-mmd_amd/csrc/mpc_host.hpp"

// what mpcmmd_mpc_step_host chains (the entry point itself lives in a HIP source, for the drawn
// variates; here u is always given)
static int step(const mpcmmd_mpc_model* m, int32_t tick, const mpcmmd_mpc_step_io* io) {
  if (int rc = mpcmmd::check_mpc(m, io)) return rc;
  mpcmmd::mpc_step_host(*m, tick, *io);
  return MPCMMD_OK;
}

static void expect(bool ok, const char* what, int a = 0) {
  if (ok) return;
  std::printf("FAILED %s (%d)\n", what, a);
  std::exit(1);
}

struct Model {
  int O, B;
  std::vector<double> pd, pdd, chol;
  std::vector<float> pop0;
  mpcmmd_mpc_model m{};
  Model(int O_, int B_) : O(O_), B(B_) {
    pd.assign(22, 0.0), pdd.assign(11, 0.0), chol.assign(64, 0.0);
    pd[1] = 1.0, pd[11 + 1] = 1.0, pd[11 + 2] = 0.01, pdd[2] = 0.5;
    for (int i = 0; i < 8; ++i) chol[i * 8 + i] = 2.0;
    pop0.resize(size_t(B) * 8);
    for (int i = 0; i < B * 8; ++i) pop0[i] = (float(i) - 16.0f) / 8.0f;
    m.num_obs = O, m.num_batch = B, m.noise = 0, m.dt = 0.15f, m.sigma_acc = 0.2f, m.sigma_steer = 0.1f;
    m.acc_const = 0.05f, m.steer_const = 0.01f, m.K_steer = 0.03f, m.a_obs = 4.25f, m.b_obs = 2.75f;
    m.y_lb = -5.25f, m.y_ub = 5.25f, m.goal_x = 1000.0f;
    m.pdot2 = pd.data(), m.pddot1 = pdd.data(), m.chol = chol.data(), m.pop0 = pop0.data();
  }
};

struct Episode {
  std::vector<float> cx, cy, u, mean, vel, veh, init, st0, xo, yo, pop, lf;
  std::vector<double> pos, ld;
  std::vector<int32_t> done, li;
  mpcmmd_mpc_step_io io{};
  explicit Episode(const Model& w)
      : cx(11, 0.0f), cy(11, 0.0f), u{0.5f, -0.25f, 1.0f}, mean(8), vel{6.0f, 0.1f, 0.0f}, veh(size_t(w.O) * 4, 0.0f),
        init(6), st0(8), xo(size_t(w.O) * 100), yo(size_t(w.O) * 100), pop(size_t(w.B) * 8), lf(MPCMMD_MPC_LOG_F),
        pos{1.0, 0.5}, ld(MPCMMD_MPC_LOG_D), done(1, -1), li(MPCMMD_MPC_LOG_I) {
    cx[1] = 6.0f, cx[2] = 40.0f, cy[2] = 0.2f;
    for (int i = 0; i < 8; ++i) mean[i] = float(i + 1);
    io.cx = cx.data(), io.cy = cy.data(), io.u = u.data(), io.mean = mean.data();
    io.pos = pos.data(), io.vel = vel.data(), io.vehicles = w.O ? veh.data() : nullptr, io.done_tick = done.data();
    io.init_state = init.data(), io.st0 = st0.data(), io.x_obs = w.O ? xo.data() : nullptr;
    io.y_obs = w.O ? yo.data() : nullptr, io.pop = pop.data();
    io.log_d = ld.data(), io.log_f = lf.data(), io.log_i = li.data();
  }
  uint32_t checksum() const {
    uint32_t s = 0;
    for (const std::vector<float>* v : {&init, &st0, &xo, &yo, &pop, &lf})
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
    Model w(3, 4);
    Episode e(w);
    const float veh[3][4] = {{40, 1, -1, 0}, {-10, 0, 2, 0}, {60, -2, 0, 0.5f}};
    std::memcpy(e.veh.data(), veh, sizeof veh);
    for (int k = 0; k < 5; ++k) {
      expect(step(&w.m, k, &e.io) == MPCMMD_OK, "step status", k);
      std::printf("tick %d %08x %.17g\n", k, e.checksum(), e.pos[0]);
    }
    expect(e.pos[0] > 1.0 && e.done[0] == -1, "the ego moved and nothing ended the episode");
  }
  {  // no vehicle: clear = -inf
    Model w(0, 1);
    Episode e(w);
    expect(step(&w.m, 0, &e.io) == MPCMMD_OK, "no vehicles");
    expect(std::isinf(e.lf[10]) && e.lf[10] < 0 && e.li[1] == 0, "clear is -inf");
  }
  {  // 64 vehicles on a line ahead, the nearest on the ego: collided; the second tick finds the episode frozen
    Model w(64, 3);
    Episode e(w);
    for (int o = 0; o < 64; ++o) e.veh[size_t(o) * 4] = 3.0f + 20.0f * float(63 - o), e.veh[size_t(o) * 4 + 1] = 0.5f;
    expect(step(&w.m, 3, &e.io) == MPCMMD_OK, "64 vehicles");
    expect(e.li[1] == 1 && e.done[0] == 3, "collision ends the episode");
    const std::vector<double> pos = e.pos;
    const std::vector<float> veh = e.veh, xo = e.xo;
    expect(step(&w.m, 4, &e.io) == MPCMMD_OK, "frozen");
    expect(pos == e.pos && veh == e.veh && xo == e.xo && e.done[0] == 3 && e.li[3] == 1,
           "a frozen episode does not change");
  }
  {  // a NaN plan collides
    Model w(2, 2);
    Episode e(w);
    e.cx[4] = NAN;
    e.veh = {1e4f, 0, 0, 0, 1e4f, 5, 0, 0};
    expect(step(&w.m, 0, &e.io) == MPCMMD_OK, "NaN plan");
    expect(e.li[1] == 1 && e.pos[0] != e.pos[0], "a NaN plan is a collision");
  }
  {
    Model w(3, 4);
    Episode e(w);
    expect(step(nullptr, 0, &e.io) == MPCMMD_E_INVALID, "null model");
    expect(step(&w.m, 0, nullptr) == MPCMMD_E_INVALID, "null io");
    mpcmmd_mpc_model bad = w.m;
    bad.num_obs = 65;
    expect(step(&bad, 0, &e.io) == MPCMMD_E_INVALID, "num_obs 65");
    bad = w.m, bad.noise = 2;
    expect(step(&bad, 0, &e.io) == MPCMMD_E_INVALID, "noise 2");
    bad = w.m, bad.dt = 0.0f;
    expect(step(&bad, 0, &e.io) == MPCMMD_E_INVALID, "dt 0");
    mpcmmd_mpc_step_io io = e.io;
    io.st0 = nullptr;
    expect(step(&w.m, 0, &io) == MPCMMD_E_INVALID, "null st0");
  }
  std::printf("ok\n");
  return 0;
}
