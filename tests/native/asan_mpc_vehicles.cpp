// Sanitizer harness of the planned vehicles' host code (csrc/mpc_vehicle.hpp,
// csrc/mpc_host.cpp: mpc_vehicle_tables, check_mpc_planned and mpc_step_host
// with the policy on, what mpcmmd_mpc_step_host_planned chains; and
// mpcmmd_mpc_vehicle_constant), built by `make -C mpc-mmd_amd
// asan_mpc_vehicles` from the host-only sources with
// -fsanitize=address,undefined -fno-sanitize-recover and run by
// tests/test_mpc_vehicles_host.py as a child process.  3 vehicles cutting in, a
// population of 4, asan_mpc.cpp's made-up basis: five chained ticks on
// exact-size heap arrays, so any read or write past an array is an ASan
// report.  Per tick it prints
//   tick <k> <sum of the fp32 outputs' words, 8 hex digits>
// which the test compares with the library's host step on the same inputs.
// Then the edges: no vehicle, 64 vehicles, a frozen episode, a NULL vehicle
// log, a NaN target, and the argument errors.  "ok" and exit status 0 on
// success.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/mpcmmd.h"
#include "../../mpc-mmd_amd/csrc/mpc_host.hpp"

// what mpcmmd_mpc_step_host_planned chains (the entry point itself lives in a HIP source, for the
// drawn variates; here u is always given)
static int step(const mpcmmd_mpc_model* m, int32_t tick, const mpcmmd_mpc_step_io* io, const mpcmmd_mpc_planned* pl) {
  if (int rc = mpcmmd::check_mpc(m, io)) return rc;
  if (int rc = mpcmmd::check_mpc_planned(m, pl)) return rc;
  const mpcmmd::MpcVehTables t = mpcmmd::mpc_vehicle_tables(m->dt);
  const mpcmmd::MpcVehConsts vc = t.view();
  mpcmmd::mpc_step_host(*m, tick, *io, nullptr, pl, &vc);
  return MPCMMD_OK;
}

static void expect(bool ok, const char* what, int a = 0) {
  if (ok) return;
  std::printf("FAILED %s (%d)\n", what, a);
  std::exit(1);
}

static uint32_t bits(float f) {
  uint32_t b;
  std::memcpy(&b, &f, 4);
  return b;
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
  std::vector<float> cx, cy, u, mean, vel, veh, init, st0, xo, yo, pop, lf, acc, tgt, vlog;
  std::vector<double> pos, ld;
  std::vector<int32_t> done, li;
  mpcmmd_mpc_step_io io{};
  mpcmmd_mpc_planned pl{};
  explicit Episode(const Model& w)
      : cx(11, 0.0f), cy(11, 0.0f), u{0.5f, -0.25f, 1.0f}, mean(8), vel{6.0f, 0.1f, 0.0f}, veh(size_t(w.O) * 4, 0.0f),
        init(6), st0(8), xo(size_t(w.O) * 100), yo(size_t(w.O) * 100), pop(size_t(w.B) * 8), lf(MPCMMD_MPC_LOG_F),
        acc(size_t(w.O) * 2, 0.0f), tgt(size_t(w.O) * 2, 0.0f), vlog(size_t(w.O) * 6), pos{1.0, 0.5},
        ld(MPCMMD_MPC_LOG_D), done(1, -1), li(MPCMMD_MPC_LOG_I) {
    cx[1] = 6.0f, cx[2] = 40.0f, cy[2] = 0.2f;
    for (int i = 0; i < 8; ++i) mean[i] = float(i + 1);
    for (int o = 0; o < w.O; ++o) tgt[size_t(o) * 2] = 6.0f, tgt[size_t(o) * 2 + 1] = -1.75f;
    io.cx = cx.data(), io.cy = cy.data(), io.u = u.data(), io.mean = mean.data();
    io.pos = pos.data(), io.vel = vel.data(), io.vehicles = w.O ? veh.data() : nullptr, io.done_tick = done.data();
    io.init_state = init.data(), io.st0 = st0.data(), io.x_obs = w.O ? xo.data() : nullptr;
    io.y_obs = w.O ? yo.data() : nullptr, io.pop = pop.data();
    io.log_d = ld.data(), io.log_f = lf.data(), io.log_i = li.data();
    pl.veh_acc = w.O ? acc.data() : nullptr, pl.veh_target = w.O ? tgt.data() : nullptr;
    pl.veh_log = w.O ? vlog.data() : nullptr;
  }
  uint32_t checksum() const {
    uint32_t s = 0;
    for (const std::vector<float>* v : {&init, &st0, &xo, &yo, &pop, &lf, &veh, &acc, &vlog})
      for (float f : *v) s += bits(f);
    return s;
  }
};

int main() {
  {
    Model w(3, 4);
    Episode e(w);
    const float veh[3][4] = {{40, 1.75f, 2, 0}, {-10, 1.75f, 3, 0.1f}, {60, -1.75f, 5, 0}};
    const float acc[3][2] = {{0.5f, -0.25f}, {0, 0}, {-1, 0.125f}};
    const float tgt[3][2] = {{6.0f, -1.75f}, {5.5f, -1.75f}, {6.25f, 1.75f}};
    std::memcpy(e.veh.data(), veh, sizeof veh);
    std::memcpy(e.acc.data(), acc, sizeof acc);
    std::memcpy(e.tgt.data(), tgt, sizeof tgt);
    for (int k = 0; k < 5; ++k) {
      expect(step(&w.m, k, &e.io, &e.pl) == MPCMMD_OK, "step status", k);
      std::printf("tick %d %08x\n", k, e.checksum());
    }
    expect(e.veh[0] > 40.0f && e.veh[1] < 1.75f && e.veh[9] > -1.75f && e.done[0] == -1,
           "the vehicles moved towards their lanes and nothing ended the episode");
    expect(e.vlog[0] == e.veh[0] && e.vlog[4] == e.acc[0], "the vehicle log is the state");
  }
  {  // no vehicle, the policy on: clear = -inf and no array is touched
    Model w(0, 1);
    Episode e(w);
    expect(step(&w.m, 0, &e.io, &e.pl) == MPCMMD_OK, "no vehicles");
    expect(std::isinf(e.lf[10]) && e.lf[10] < 0 && e.li[1] == 0, "clear is -inf");
  }
  {  // 64 vehicles on a line ahead, the nearest on the ego: collided; the second tick finds the episode frozen
    Model w(64, 3);
    Episode e(w);
    for (int o = 0; o < 64; ++o)
      e.veh[size_t(o) * 4] = 2.0f + 20.0f * float(63 - o), e.veh[size_t(o) * 4 + 1] = 0.5f, e.veh[size_t(o) * 4 + 2] = 6.0f;
    expect(step(&w.m, 3, &e.io, &e.pl) == MPCMMD_OK, "64 vehicles");
    expect(e.li[1] == 1 && e.done[0] == 3, "collision ends the episode");
    const std::vector<double> pos = e.pos;
    const std::vector<float> veh = e.veh, acc = e.acc, xo = e.xo;
    e.pl.veh_log = nullptr;  // the log is optional
    expect(step(&w.m, 4, &e.io, &e.pl) == MPCMMD_OK, "frozen");
    expect(pos == e.pos && veh == e.veh && acc == e.acc && xo == e.xo && e.done[0] == 3 && e.li[3] == 1,
           "a frozen episode does not change");
  }
  {  // a NaN target: that vehicle's state and tracks are the quiet NaN, the episode collides
    Model w(2, 2);
    Episode e(w);
    e.veh = {1e4f, 0, 5, 0, 1e4f, 5, 5, 0};
    e.tgt[2] = -NAN;
    expect(step(&w.m, 0, &e.io, &e.pl) == MPCMMD_OK, "NaN target");
    expect(e.li[1] == 1 && bits(e.veh[4]) == 0x7FC00000u && bits(e.xo[100 + 57]) == 0x7FC00000u &&
               bits(e.vlog[6 + 4]) == 0x7FC00000u && e.veh[0] == e.veh[0] && e.xo[57] == e.xo[57],
           "a NaN target is a collision");
  }
  {
    Model w(3, 4);
    Episode e(w);
    expect(step(&w.m, 0, &e.io, nullptr) == MPCMMD_E_INVALID, "null pl");
    expect(step(&w.m, 0, nullptr, &e.pl) == MPCMMD_E_INVALID, "null io");
    mpcmmd_mpc_planned pl = e.pl;
    pl.veh_acc = nullptr;
    expect(step(&w.m, 0, &e.io, &pl) == MPCMMD_E_INVALID, "null veh_acc");
    pl = e.pl, pl.veh_target = nullptr;
    expect(step(&w.m, 0, &e.io, &pl) == MPCMMD_E_INVALID, "null veh_target");
    mpcmmd_mpc_model bad = w.m;
    bad.dt = 15.0f;
    expect(step(&bad, 0, &e.io, &e.pl) == MPCMMD_E_INVALID, "dt 15");
    std::vector<double> buf(1100);
    expect(mpcmmd_mpc_vehicle_constant(0.15f, "P", buf.data(), 1100) == 1100, "P");
    expect(mpcmmd_mpc_vehicle_constant(0.15f, "adv", buf.data(), 33) == 33, "adv");
    expect(mpcmmd_mpc_vehicle_constant(0.15f, "kinv_y", buf.data(), 224) == MPCMMD_E_INVALID, "dst too small");
    expect(mpcmmd_mpc_vehicle_constant(0.0f, "adv", buf.data(), 33) == MPCMMD_E_INVALID, "dt 0");
    expect(mpcmmd_mpc_vehicle_constant(15.0f, "adv", buf.data(), 33) == MPCMMD_E_INVALID, "dt 15");
    expect(mpcmmd_mpc_vehicle_constant(0.15f, "nothing", buf.data(), 33) == MPCMMD_E_INVALID, "unknown name");
    expect(mpcmmd_mpc_vehicle_constant(0.15f, nullptr, buf.data(), 33) == MPCMMD_E_INVALID, "null name");
  }
  std::printf("ok\n");
  return 0;
}
