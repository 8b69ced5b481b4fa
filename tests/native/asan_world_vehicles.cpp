// Sanitizer harness of the routed vehicles' host step (csrc/world_vehicle.hpp,
// csrc/world_host.cpp: check_world_routed and world_step_host with a policy, what
// mpcmmd_world_step_host_routed chains), built by
// `make -C mpc-mmd_amd asan_world_vehicles` from the host-only sources with
// -fsanitize=address,undefined -fno-sanitize-recover and run by
// tests/test_world_vehicles_host.py as a child process.  A straight route of 40
// points (x = arc, y = 0), 6 vehicles -- a follower behind two candidates at
// bit-equal gaps, a parked one, one past the route's end at exactly lane_tol from
// the lane, one before its start with a NaN target speed -- num_path 5, 2
// obstacles, a population of 4: the reset-mode step, eight chained ticks and a
// ninth with a NaN arc length, on exact-size heap arrays, so any read or write
// past an array is an ASan report.  Per step it prints
//   tick <k> <sum of the outputs' 32-bit words, 8 hex digits> <done_tick>
// which the test compares with the library's host step on the same inputs.
// Then the worlds at the edge: no vehicle, 64 vehicles in one lane, a frozen
// episode, a NULL log, and the argument errors.  "ok" and exit status 0 on success.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../../include/mpcmmd.h"
#include "../../mpc-mmd_amd/csrc/world_host.hpp"

// what mpcmmd_world_step_host_routed chains (the entry point itself lives in a HIP source, for the
// drawn variates; here u is always given)
static int step(const mpcmmd_world_model* m, int32_t tick, const mpcmmd_world_step_io* io,
                const mpcmmd_world_routed* rt) {
  if (int rc = mpcmmd::check_world(m, io)) return rc;
  if (int rc = mpcmmd::check_world_routed(m, rt)) return rc;
  mpcmmd::world_step_host(*m, tick, *io, nullptr, rt);
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
  std::vector<float> cx, cy, steer, u, mean, ego, veh, init, xw, yw, obs, pop, lf, vv, par, vlog;
  std::vector<double> pos, ld, vs;
  std::vector<int32_t> done, li;
  mpcmmd_world_step_io io{};
  mpcmmd_world_routed rt{};
  explicit Episode(const World& w)
      : cx(11, 0.0f), cy(11, 0.0f), steer(4, 0.05f), u{0.5f, -0.25f, 1.0f, -1.0f}, mean(8), ego{2.0f, 0.1f, 0.0f},
        veh(size_t(w.T) * 5, 0.0f), init(6), xw(w.P), yw(w.P), obs(size_t(w.O) * 5), pop(size_t(w.B) * 8),
        lf(MPCMMD_WORLD_LOG_F, 0.0f), vv(w.T, 0.0f), par(size_t(w.T) * 2, 0.0f), vlog(size_t(w.T) * 2, 0.0f),
        pos{1.0, 0.5}, ld(MPCMMD_WORLD_LOG_D), vs(w.T, 0.0), done(1, -1), li(MPCMMD_WORLD_LOG_I) {
    cx[1] = 6.0f;
    for (int i = 0; i < 8; ++i) mean[i] = float(i + 1);
    io.cx = cx.data(), io.cy = cy.data(), io.steer = steer.data(), io.u = u.data(), io.mean = mean.data();
    io.pos = pos.data(), io.ego = ego.data(), io.vehicles = w.T ? veh.data() : nullptr, io.done_tick = done.data();
    io.init_state = init.data(), io.x_wp = xw.data(), io.y_wp = yw.data(), io.obstacles = obs.data();
    io.pop = pop.data(), io.log_d = ld.data(), io.log_f = lf.data(), io.log_i = li.data();
    rt.veh_s = w.T ? vs.data() : nullptr, rt.veh_v = w.T ? vv.data() : nullptr;
    rt.veh_param = w.T ? par.data() : nullptr, rt.veh_log = w.T ? vlog.data() : nullptr;
    rt.acc_max = 1.5f, rt.brake = 2.0f, rt.gap0 = 5.0f, rt.headway = 1.0f, rt.length = 4.5f, rt.lane_tol = 1.75f;
    rt.gap_min = 0.5f, rt.acc_min = -8.0f;
  }
  uint32_t checksum() const {
    uint32_t s = 0;
    for (const std::vector<float>* v : {&init, &xw, &yw, &obs, &pop, &lf, &veh, &vv, &vlog})
      for (float f : *v) {
        uint32_t b;
        std::memcpy(&b, &f, 4);
        s += b;
      }
    for (double d : vs) {
      uint32_t b[2];
      std::memcpy(b, &d, 8);
      s += b[0] + b[1];
    }
    return s;
  }
};

int main() {
  const float nanf_ = std::numeric_limits<float>::quiet_NaN();
  {
    World w(40, 5, 2, 6, 4);
    Episode e(w);
    const double s[6] = {20.0, 30.0, 30.0, 50.0, 95.0, -4.0};
    const float v[6] = {4.0f, 1.0f, 3.0f, 2.0f, 5.0f, 6.0f};
    const float par[6][2] = {{0.0f, 6.0f}, {0.5f, 0.0f}, {-0.5f, 5.0f}, {0.0f, 5.0f}, {1.75f, 7.0f}, {0.0f, nanf_}};
    std::memcpy(e.vs.data(), s, sizeof s), std::memcpy(e.vv.data(), v, sizeof v);
    std::memcpy(e.par.data(), par, sizeof par);
    for (int k = -1; k < 8; ++k) {
      expect(step(&w.m, k, &e.io, &e.rt) == MPCMMD_OK, "step status", k);
      std::printf("tick %d %08x %d\n", k, e.checksum(), e.done[0]);
      if (k == -1) expect(e.vs[0] == 20.0 && e.pos[0] == 1.0 && e.veh[0] == 20.0f, "the reset-mode step moves nothing");
    }
    expect(e.pos[0] > 1.0 && e.done[0] == -1 && e.vs[0] > 20.0, "the ego and the vehicles moved, nothing ended");
    expect(e.vs[1] == 30.0 && e.vv[1] == 0.0f && e.vs[5] == -4.0 && e.vv[5] == 0.0f, "the parked stay");
    expect(e.vs[4] > 95.0 && e.veh[4 * 5] > 95.0f, "past the end the last piece extrapolates");
    e.vs[3] = std::numeric_limits<double>::quiet_NaN();
    expect(step(&w.m, 8, &e.io, &e.rt) == MPCMMD_OK, "NaN step status");
    std::printf("tick %d %08x %d\n", 8, e.checksum(), e.done[0]);
    expect(e.done[0] == 8 && e.li[2] == 1 && e.veh[3 * 5] != e.veh[3 * 5], "a NaN vehicle collides");
  }
  {  // no vehicle: NULL arrays, both obstacles are the placeholders 300 m away
    World w(40, 2, 2, 0, 1);
    Episode e(w);
    expect(step(&w.m, 0, &e.io, &e.rt) == MPCMMD_OK, "no vehicles");
    expect(e.obs[0] == float(300.0 - e.pos[0]) && e.obs[5] == e.obs[0] && e.li[2] == 0, "placeholders");
  }
  {  // 64 vehicles in one lane ahead, a metre apart: everybody brakes; then the episode frozen, and no log
    World w(40, 2048, 64, 64, 3);
    Episode e(w);
    for (int o = 0; o < 64; ++o) {
      e.vs[o] = 12.0 + double(63 - o), e.vv[o] = 3.0f;
      e.par[size_t(o) * 2] = 0.25f, e.par[size_t(o) * 2 + 1] = 8.0f;
    }
    expect(step(&w.m, 3, &e.io, &e.rt) == MPCMMD_OK, "64 vehicles");
    for (int o = 1; o < 64; ++o) expect(e.vlog[size_t(o) * 2 + 1] == -8.0f, "bumper to bumper: acc_min", o);
    expect(e.vlog[1] > 0.0f && e.done[0] == -1, "the first has a free road");
    e.done[0] = 2;
    e.rt.veh_log = nullptr;
    const std::vector<double> pos = e.pos, vs = e.vs;
    const std::vector<float> veh = e.veh, vv = e.vv, xw = e.xw;
    expect(step(&w.m, 4, &e.io, &e.rt) == MPCMMD_OK, "frozen");
    expect(pos == e.pos && vs == e.vs && vv == e.vv && veh == e.veh && xw == e.xw && e.done[0] == 2,
           "a frozen episode does not change and rewrites the same rows");
  }
  {
    World w(40, 5, 2, 3, 4);
    Episode e(w);
    expect(step(&w.m, 0, &e.io, nullptr) == MPCMMD_E_INVALID, "null policy");
    expect(step(nullptr, 0, &e.io, &e.rt) == MPCMMD_E_INVALID, "null model");
    mpcmmd_world_routed bad = e.rt;
    bad.veh_s = nullptr;
    expect(step(&w.m, 0, &e.io, &bad) == MPCMMD_E_INVALID, "null veh_s");
    bad = e.rt, bad.veh_v = nullptr;
    expect(step(&w.m, 0, &e.io, &bad) == MPCMMD_E_INVALID, "null veh_v");
    bad = e.rt, bad.veh_param = nullptr;
    expect(step(&w.m, 0, &e.io, &bad) == MPCMMD_E_INVALID, "null veh_param");
    bad = e.rt, bad.acc_max = 0.0f;
    expect(step(&w.m, 0, &e.io, &bad) == MPCMMD_E_INVALID, "acc_max 0");
    bad = e.rt, bad.brake = -1.0f;
    expect(step(&w.m, 0, &e.io, &bad) == MPCMMD_E_INVALID, "brake < 0");
    bad = e.rt, bad.gap_min = 0.0f;
    expect(step(&w.m, 0, &e.io, &bad) == MPCMMD_E_INVALID, "gap_min 0");
    bad = e.rt, bad.acc_min = 0.0f;
    expect(step(&w.m, 0, &e.io, &bad) == MPCMMD_E_INVALID, "acc_min 0");
    bad = e.rt, bad.lane_tol = -0.5f;
    expect(step(&w.m, 0, &e.io, &bad) == MPCMMD_E_INVALID, "lane_tol < 0");
    bad = e.rt, bad.lane_tol = nanf_;
    expect(step(&w.m, 0, &e.io, &bad) == MPCMMD_E_INVALID, "lane_tol NaN");
    bad = e.rt, bad.lane_tol = 0.0f;
    expect(step(&w.m, 0, &e.io, &bad) == MPCMMD_OK, "lane_tol 0 is legal");
  }
  std::printf("ok\n");
  return 0;
}
