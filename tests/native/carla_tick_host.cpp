// Sanitizer harness of the host route of a CARLA tick (csrc/carla_host.cpp:
// carla_tick_host, through the C entry point mpcmmd_carla_tick_host of
// csrc/host_api.cpp), built by `make -C mpc-mmd_amd asan_tick` from the
// host-only sources with -fsanitize=address,undefined -fno-sanitize-recover
// and run by tests/test_carla_tick_cpu.py as a child process.  At num_path = 4
// (the minimum) and 37, with 3 obstacles (one of them with a NaN x, one 300 m
// away), it checks
//   chain   the one call equals path_smoothing, path_parameters,
//           global_to_frenet and the track formula called one by one, bit for bit
//   bounds  exact-size heap arrays: any read or write past num_path, [O][5] or
//           [O][100] is an ASan report
//   errors  num_path 3 and 2049, a NULL array and a NaN threshold are MPCMMD_E_INVALID
// Exit status 0 and "ok" on success; the first failed check prints and exits 1.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../../include/mpcmmd.h"
#include "../../mpc-mmd_amd/csrc/carla_host.hpp"

using namespace mpcmmd;

static void expect(bool ok, const char* what, int a = 0, int b = 0) {
  if (ok) return;
  std::printf("FAILED %s (%d, %d)\n", what, a, b);
  std::exit(1);
}

static bool same_bits(const float* a, const float* b, size_t n) { return std::memcmp(a, b, n * 4) == 0; }

static void run(int P) {
  const int O = 3;
  std::vector<float> xw(P), yw(P), ob(size_t(O) * 5), init(6, 0.0f);
  for (int i = 0; i < P; ++i) {  // a gentle left bend, 300 m long
    const float s = 300.0f * float(i) / float(P - 1);
    xw[i] = s;
    yw[i] = 0.0005f * s * s + 0.05f * std::sin(0.3f * s);
  }
  const float obs[O][5] = {{40.0f, 1.0f, 3.0f, 0.5f, 0.2f},
                           {std::numeric_limits<float>::quiet_NaN(), -2.0f, 1.0f, 0.0f, 0.0f},
                           {300.0f, 300.0f, 0.0f, 0.0f, 0.0f}};
  std::memcpy(ob.data(), obs, sizeof obs);
  std::vector<float> p6(size_t(6) * P), xo(size_t(O) * 100), yo(size_t(O) * 100);
  expect(mpcmmd_carla_tick_host(P, O, init.data(), xw.data(), yw.data(), ob.data(), 0.1f, p6.data(), xo.data(),
                                yo.data()) == MPCMMD_OK, "tick_host status", P);
  // the chain, call by call
  std::vector<float> x(P), y(P), fx(P), fy(P), fxx(P), fyy(P), arc(P), kap(P);
  path_smoothing(P, xw.data(), yw.data(), 0.1f, x.data(), y.data());
  path_parameters(P, x.data(), y.data(), fx.data(), fy.data(), fxx.data(), fyy.data(), arc.data(), kap.data(), nullptr);
  const float* want[6] = {x.data(), y.data(), arc.data(), fx.data(), fy.data(), kap.data()};
  for (int k = 0; k < 6; ++k) expect(same_bits(p6.data() + size_t(k) * P, want[k], P), "path array", P, k);
  PathView pv;
  pv.P = P, pv.x = x.data(), pv.y = y.data(), pv.arc = arc.data(), pv.Fxd = fx.data(), pv.Fyd = fy.data();
  pv.kappa = kap.data();
  const float* tt = track_times();
  expect(tt[0] == 0.0f && tt[99] == 15.0f && tt[1] == float(15.0 / 99.0), "track times");
  for (int o = 0; o < O; ++o) {
    const float v = std::sqrt(obs[o][2] * obs[o][2] + obs[o][3] * obs[o][3]);
    const FrenetState f = global_to_frenet(pv, obs[o][0], obs[o][1], v, 0.0f, obs[o][4], 0.0f);
    for (int k = 0; k < 100; ++k) {
      const float ex = f.x + f.vx * tt[k], ey = f.y + f.vy * tt[k];
      expect(same_bits(&ex, &xo[size_t(o) * 100 + k], 1) && same_bits(&ey, &yo[size_t(o) * 100 + k], 1), "track",
             o, k);
    }
  }
  // the NaN obstacle: the first NaN distance is at path point 0, so its track starts at arc_vec[0] = 0
  expect(xo[100] == 0.0f + 0.0f || xo[100] != xo[100], "NaN obstacle's closest point");
  // argument errors
  const float nan = std::numeric_limits<float>::quiet_NaN();
  expect(mpcmmd_carla_tick_host(3, O, init.data(), xw.data(), yw.data(), ob.data(), 0.1f, p6.data(), xo.data(),
                                yo.data()) == MPCMMD_E_INVALID, "num_path 3");
  expect(mpcmmd_carla_tick_host(2049, O, init.data(), xw.data(), yw.data(), ob.data(), 0.1f, p6.data(), xo.data(),
                                yo.data()) == MPCMMD_E_INVALID, "num_path 2049");
  expect(mpcmmd_carla_tick_host(P, O, init.data(), nullptr, yw.data(), ob.data(), 0.1f, p6.data(), xo.data(),
                                yo.data()) == MPCMMD_E_INVALID, "null x_wp");
  expect(mpcmmd_carla_tick_host(P, O, init.data(), xw.data(), yw.data(), ob.data(), nan, p6.data(), xo.data(),
                                yo.data()) == MPCMMD_E_INVALID, "NaN threshold");
  expect(mpcmmd_carla_tick_host(P, 0, init.data(), xw.data(), yw.data(), nullptr, 0.1f, p6.data(), nullptr, nullptr) ==
             MPCMMD_OK, "no obstacles");
}

int main() {
  run(4);
  run(37);
  std::printf("ok\n");
  return 0;
}
