// Host-code sanitizer harness ("run the CPU-side C++ under
// ASan/UBSan").  Built by `make -C mpc-mmd_amd asan` with
// -fsanitize=address,undefined from the library's own host sources
// (csrc/*.cpp: host_constants, carla_host, solve_host, host_api, episodes_host), no GPU and no
// HIP runtime.  Exercises every host-only entry: the batch-invariant constants
// of each variant and horizon (mpcmmd_host_constant's builders) and the
// dynamic-obstacle QP trajectories (mpcmmd_obs_dynamic_traj's builder), then
// prints one line per quantity ("name count sum sumabs") for
// tests/test_asan_host.py to compare with the product library's values.  The
// C entry points that need no device (host_api.cpp) are called with valid and
// with each kind of invalid argument, mpcmmd_create_batch's range check at its
// boundaries, the device buffer list (buffers.hpp) is expanded for five shapes,
// and the episode contexts' host-only pieces (episodes_host.cpp) meet every
// rejection, a hand-written table and a wrapping index; a wrong status ends the
// run with exit code 3.
//
// Given a file name, it also writes there the inputs and results of the path
// helpers (carla_host.cpp) and of every function of solve_host.cpp at the
// smallest shapes where their indexing can go wrong, one array per line
// ("name type count values..."), for tests/test_solve_host.py to hold against
// the oracle.  Without a file name the same cases run, unrecorded.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <set>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../mpc-mmd_amd/csrc/buffers.hpp"
#include "../../mpc-mmd_amd/csrc/episodes_host.hpp"
#include "../../mpc-mmd_amd/csrc/host_api.hpp"
#include "../../mpc-mmd_amd/csrc/host_constants.hpp"
#include "../../mpc-mmd_amd/csrc/layout.hpp"
#include "../../mpc-mmd_amd/csrc/solve_host.hpp"

using namespace mpcmmd;

static void emit(const char* tag, int H, int variant, const char* name, const std::vector<double>& v) {
  double s = 0.0, a = 0.0;
  for (double x : v) {
    s += x;
    a += std::fabs(x);
  }
  std::printf("%s %d %d %s %zu %.17g %.17g\n", tag, H, variant, name, v.size(), s, a);
}

static FILE* g_rec = nullptr;

static void put(const std::string& name, const float* v, size_t n) {
  if (!g_rec) return;
  std::fprintf(g_rec, "%s f32 %zu", name.c_str(), n);
  for (size_t i = 0; i < n; ++i) std::fprintf(g_rec, " %.9g", double(v[i]));
  std::fprintf(g_rec, "\n");
}
static void put(const std::string& name, const double* v, size_t n) {
  if (!g_rec) return;
  std::fprintf(g_rec, "%s f64 %zu", name.c_str(), n);
  for (size_t i = 0; i < n; ++i) std::fprintf(g_rec, " %.17g", v[i]);
  std::fprintf(g_rec, "\n");
}
static void put(const std::string& name, const int32_t* v, size_t n) {
  if (!g_rec) return;
  std::fprintf(g_rec, "%s i32 %zu", name.c_str(), n);
  for (size_t i = 0; i < n; ++i) std::fprintf(g_rec, " %d", v[i]);
  std::fprintf(g_rec, "\n");
}
template <class T>
static void put(const std::string& name, const std::vector<T>& v) {
  put(name, v.data(), v.size());
}

// deterministic test inputs: uniform in [-1, 1), exact in fp32
static uint32_t g_lcg = 12345u;
static uint32_t rnd_u() {
  g_lcg = g_lcg * 1664525u + 1013904223u;
  return g_lcg >> 8;
}
static float rnd() { return float(int32_t(rnd_u() & 0xFFFF) - 32768) / 32768.0f; }
static std::vector<float> rnd_vec(size_t n, float scale = 1.0f, float shift = 0.0f) {
  std::vector<float> v(n);
  for (float& x : v) x = rnd() * scale + shift;
  return v;
}

// carla_host.cpp: a short path through smoothing, parameters and Frenet states
struct TestPath {
  std::vector<float> x, y, Fxd, Fyd, Fxdd, Fydd, arc, kappa;
  PathView view() const {
    return path_view(int(x.size()), x.data(), y.data(), arc.data(), Fxd.data(), Fyd.data(), kappa.data());
  }
};
static TestPath path_case(int P) {
  const std::string c = "path.P" + std::to_string(P) + "/";
  std::vector<float> xw(P), yw(P);
  for (int i = 0; i < P; ++i) {
    xw[i] = 2.0f * float(i) + 0.25f * rnd();
    yw[i] = 0.02f * float(i) * float(i) + 0.25f * rnd();
  }
  TestPath p;
  for (auto* v : {&p.x, &p.y, &p.Fxd, &p.Fyd, &p.Fxdd, &p.Fydd, &p.arc, &p.kappa}) v->assign(P, 0.0f);
  path_smoothing(P, xw.data(), yw.data(), 0.1f, p.x.data(), p.y.data());
  float arc_length = 0.0f;
  path_parameters(P, p.x.data(), p.y.data(), p.Fxd.data(), p.Fyd.data(), p.Fxdd.data(), p.Fydd.data(), p.arc.data(),
                  p.kappa.data(), &arc_length);
  const int N = 8;
  std::vector<float> pts(size_t(N) * 6), fr(size_t(N) * 7);  // x, y, v, vdot, psi, psidot
  const PathView pv = p.view();
  for (int i = 0; i < N; ++i) {
    float* q = &pts[size_t(i) * 6];
    q[0] = float(P) * (rnd() + 1.0f), q[1] = 3.0f * rnd(), q[2] = 5.0f * (rnd() + 1.0f);
    q[3] = rnd(), q[4] = 3.0f * rnd(), q[5] = 0.5f * rnd();
    const FrenetState f = global_to_frenet(pv, q[0], q[1], q[2], q[3], q[4], q[5]);
    const float o[7] = {f.x, f.y, f.vx, f.vy, f.ax, f.ay, f.psi};
    for (int k = 0; k < 7; ++k) fr[size_t(i) * 7 + k] = o[k];
  }
  put(c + "x_wp", xw), put(c + "y_wp", yw), put(c + "x", p.x), put(c + "y", p.y);
  put(c + "Fx_dot", p.Fxd), put(c + "Fy_dot", p.Fyd), put(c + "Fx_ddot", p.Fxdd), put(c + "Fy_ddot", p.Fydd);
  put(c + "arc_vec", p.arc), put(c + "kappa", p.kappa), put(c + "arc_length", &arc_length, 1);
  put(c + "points", pts), put(c + "frenet", fr);
  return p;
}

// what mpcmmd_create_batch / mpcmmd_begin compute per handle and per
// configuration, for a static handle of horizon H with O obstacles
static void begin_case(int H, int O) {
  const int B = 20, T = 1, S = 3;
  const std::string c = "begin.H" + std::to_string(H) + ".O" + std::to_string(O) + "/";
  const ProblemConsts pc = build_constants(H, 0);
  put(c + "basis", pack_basis(pc));
  put(c + "guess_g", pack_guess_g(pc));
  put(c + "proj_m", pack_proj_m(pc.proj_kinv_x, pc.proj_kinv_y));
  const std::vector<float> is = {0.5f + rnd(), 1.75f, 5.0f + rnd(), 0.25f * rnd(), 0.5f * rnd(), 0.5f * rnd()};
  const double bx[3] = {is[0], is[2], is[4]}, by[4] = {is[1], is[3], is[5], 0.0};
  std::vector<double> sc(4 * kNvar);
  solve_columns(pc, pc.proj_kinv_x.data(), pc.proj_kinv_y.data(), bx, by, sc.data());
  std::vector<float> st0(8, -1.0f);
  initial_state(is.data(), st0.data());
  const std::vector<float> xo = rnd_vec(size_t(O) * kNum, 50.0f, 60.0f), yo = rnd_vec(size_t(O) * kNum, 2.0f);
  std::vector<float> ob(size_t(2) * O * H);
  obstacle_transpose(xo.data(), yo.data(), O, H, ob.data());
  // two populations: one around the reference's initial mean, one whose speeds meet both clips
  const std::vector<float> z = rnd_vec(size_t(B) * 8, 3.0f);
  std::vector<float> cov(64), w = rnd_vec(8);
  for (int i = 0; i < 8; ++i)
    for (int j = 0; j < 8; ++j) cov[i * 8 + j] = (i == j ? (i < 4 ? 20.0f : 100.0f) : 0.0f) + w[i] * w[j];
  const float means[2][8] = {{15, 15, 15, 15, 0, 0, 0, 0}, {0.5f, 29.0f, 2.0f, 27.0f, 1.75f, -1.75f, 0.5f, 0}};
  std::vector<float> pop(size_t(2) * B * 8);
  for (int g = 0; g < 2; ++g) initial_population(means[g], cov.data(), z.data(), B, pop.data() + size_t(g) * B * 8);
  const std::vector<float> roll = rnd_vec(size_t(T) * 3 * S * H);
  put(c + "init_state", is), put(c + "solve_c", sc), put(c + "st0", st0);
  put(c + "x_obs", xo), put(c + "y_obs", yo), put(c + "obs", ob);
  put(c + "z", z), put(c + "cov", cov), put(c + "mean", &means[0][0], 16), put(c + "pop", pop);
  put(c + "roll", roll), put(c + "roll_t", roll_transpose(roll.data(), T, S, H));
  // a covariance that is not positive definite throws (and leaks nothing: the leak check runs at exit)
  cov[3 * 8 + 3] = -1.0f;
  int32_t threw = 0;
  try {
    initial_population(means[0], cov.data(), z.data(), B, pop.data());
  } catch (const std::invalid_argument&) {
    threw = 1;
  }
  put(c + "not_pd_threw", &threw, 1);
  // a result's speeds and a validated plan's controls at this horizon
  const std::vector<float> cx = rnd_vec(kNvar, 20.0f, 30.0f), cy = rnd_vec(kNvar, 2.0f);
  std::vector<float> vb(kNum);
  plan_speed(pc, cx.data(), cy.data(), vb.data());
  const int K = 2;
  const std::vector<float> v = rnd_vec(size_t(K) * kNum, 5.0f, 10.0f), steer = rnd_vec(size_t(K) * kNum, 0.3f);
  std::vector<float> acc, steer_h;
  plan_controls(v.data(), steer.data(), K, H, acc, steer_h);
  put(c + "cx", cx), put(c + "cy", cy), put(c + "v_best", vb);
  put(c + "plan_v", v), put(c + "plan_steer", steer), put(c + "plan_acc", acc), put(c + "plan_steer_h", steer_h);
}

// mpcmmd_carla_begin's rows and KKT columns for R = 1 (det), n (cvar), n^2 (mmd_opt)
static void carla_case(int n, int H, int O, const TestPath& path) {
  const ProblemConsts pc = build_constants(H, 2);
  std::vector<double> det_kx, det_ky;
  det_projection_kinv(pc, O, det_kx, det_ky);
  const int M = n * n;
  for (int R : {1, n, M}) {
    const std::string c = "carla.n" + std::to_string(n) + ".R" + std::to_string(R) + "/";
    const std::vector<float> is = {1.0f + rnd(), 0.3f * rnd(), 6.0f + rnd(), 0.2f * rnd(), 0.1f * rnd(), 0.02f * rnd()};
    const std::vector<float> eps = rnd_vec(size_t(R) * 4, 2.0f);
    std::vector<float> rows;
    double bx[3], by[4];
    carla_rows(pc, R, M, is.data(), path.view(), eps.data(), rows, bx, by);
    const bool det = R == 1;
    std::vector<double> sc(4 * kNvar);
    solve_columns(pc, det ? det_kx.data() : pc.proj_kinv_x.data(), det ? det_ky.data() : pc.proj_kinv_y.data(), bx, by,
                  sc.data());
    float vh[3];
    carla_velocity_heading(is[2], is[4], &vh[0], &vh[1], &vh[2]);
    put(c + "init_state", is), put(c + "eps", eps), put(c + "rows", rows), put(c + "bx", bx, 3), put(c + "by", by, 4);
    put(c + "solve_c", sc), put(c + "velocity_heading", vh, 3);
    if (det) put(c + "proj_m_det", pack_proj_m(det_kx, det_ky));
  }
}

// the first-selection tables and the beta_z image of an n^2-row mother set:
// mother row 0 has no pair, row 1's pairs all carry one sigma
static void beta_case(int n) {
  const int M = n * n, np = kBetaSamples * n;
  const std::string c = "beta.n" + std::to_string(n) + "/";
  std::vector<int32_t> sel(np);
  std::vector<float> sig(kBetaSamples);
  for (int s = 0; s < kBetaSamples; ++s) sig[s] = s < 10 ? 1.0f : 0.25f * float(1 + s % 7);
  for (int i = 0; i < np; ++i) sel[i] = i / n < 10 ? 1 + i % 3 : 2 + int(rnd_u() % uint32_t(M - 2));
  const Sel0Tables t = first_selection_tables(sel.data(), sig.data(), n, M);
  put(c + "sel", sel), put(c + "sig", sig), put(c + "rp0", t.rp), put(c + "rpair0", t.pairs), put(c + "rperm", t.rperm);
  int32_t threw = 0;
  sel[np - 1] = M;  // one past the last mother row
  try {
    (void)first_selection_tables(sel.data(), sig.data(), n, M);
  } catch (const std::runtime_error&) {
    threw = 1;
  }
  put(c + "range_threw", &threw, 1);
  const int M1 = M + 1, R = kBetaSamples - kBetaElite;
  std::vector<float> z(size_t(R) * M1);
  for (size_t i = 0; i < z.size(); ++i) z[i] = float(i + 1);  // distinct and non-zero
  put(c + "beta_z", beta_z_image(z.data(), M));
}

static void expect(const char* what, int got, int want) {
  if (got == want) return;
  std::fprintf(stderr, "asan_host: %s: status %d, expected %d (%s)\n", what, got, want, mpcmmd_last_error());
  std::exit(3);
}
static void expect_true(const char* what, bool ok) { expect(what, ok ? 1 : 0, 1); }

// host_api.cpp: each entry point once with valid small inputs and once per documented invalid argument
static void api_cases() {
  const int OK = MPCMMD_OK, BAD = MPCMMD_E_INVALID;
  expect("abi_version", mpcmmd_abi_version(), MPCMMD_ABI_VERSION);
  // path smoothing / parameters / Frenet states of a 6-point path
  const int P = 6;
  std::vector<float> xw(P), yw(P), x(P), y(P), Fxd(P), Fyd(P), Fxdd(P), Fydd(P), arc(P), kap(P);
  for (int i = 0; i < P; ++i) xw[i] = 2.0f * float(i), yw[i] = 0.05f * float(i * i);
  float len = 0.0f;
  expect("path_smoothing", mpcmmd_path_smoothing(P, xw.data(), yw.data(), 0.1f, x.data(), y.data()), OK);
  expect("path_smoothing null", mpcmmd_path_smoothing(P, nullptr, yw.data(), 0.1f, x.data(), y.data()), BAD);
  expect("path_smoothing null out", mpcmmd_path_smoothing(P, xw.data(), yw.data(), 0.1f, x.data(), nullptr), BAD);
  expect("path_smoothing 3", mpcmmd_path_smoothing(3, xw.data(), yw.data(), 0.1f, x.data(), y.data()), BAD);
  expect("path_smoothing kMaxPath + 1",
         mpcmmd_path_smoothing(kMaxPath + 1, xw.data(), yw.data(), 0.1f, x.data(), y.data()), BAD);
  expect_true("last_error", std::strlen(mpcmmd_last_error()) > 0);
  expect("path_parameters", mpcmmd_path_parameters(P, x.data(), y.data(), Fxd.data(), Fyd.data(), Fxdd.data(),
                                                   Fydd.data(), arc.data(), kap.data(), &len), OK);
  expect("path_parameters null", mpcmmd_path_parameters(P, x.data(), nullptr, Fxd.data(), Fyd.data(), Fxdd.data(),
                                                        Fydd.data(), arc.data(), kap.data(), &len), BAD);
  expect("path_parameters 2", mpcmmd_path_parameters(2, x.data(), y.data(), Fxd.data(), Fyd.data(), Fxdd.data(),
                                                     Fydd.data(), arc.data(), kap.data(), &len), BAD);
  mpcmmd_path pth{P, x.data(), y.data(), arc.data(), Fxd.data(), Fyd.data(), kap.data()};
  const int N = 3;
  const std::vector<float> gx = {1.0f, 4.5f, 9.0f}, gy = {0.2f, -0.3f, 1.0f}, gv = {5.0f, 6.0f, 7.0f};
  const std::vector<float> gvd = {0.1f, 0.0f, -0.1f}, gpsi = {0.0f, 0.1f, 0.2f}, gpd = {0.0f, 0.01f, 0.02f};
  std::vector<float> fr(size_t(N) * 7);
  expect("global_to_frenet", mpcmmd_global_to_frenet(&pth, N, gx.data(), gy.data(), gv.data(), gvd.data(), gpsi.data(),
                                                     gpd.data(), fr.data()), OK);
  expect("global_to_frenet count 0",
         mpcmmd_global_to_frenet(&pth, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), OK);
  expect("global_to_frenet null path", mpcmmd_global_to_frenet(nullptr, N, gx.data(), gy.data(), gv.data(), gvd.data(),
                                                               gpsi.data(), gpd.data(), fr.data()), BAD);
  expect("global_to_frenet count < 0", mpcmmd_global_to_frenet(&pth, -1, gx.data(), gy.data(), gv.data(), gvd.data(),
                                                               gpsi.data(), gpd.data(), fr.data()), BAD);
  expect("global_to_frenet null out", mpcmmd_global_to_frenet(&pth, N, gx.data(), gy.data(), gv.data(), gvd.data(),
                                                              gpsi.data(), gpd.data(), nullptr), BAD);
  mpcmmd_path bad = pth;
  bad.num_path = 1;
  expect("global_to_frenet num_path 1", mpcmmd_global_to_frenet(&bad, N, gx.data(), gy.data(), gv.data(), gvd.data(),
                                                                gpsi.data(), gpd.data(), fr.data()), BAD);
  bad = pth;
  bad.kappa = nullptr;
  expect("global_to_frenet null path array", mpcmmd_global_to_frenet(&bad, N, gx.data(), gy.data(), gv.data(),
                                                                     gvd.data(), gpsi.data(), gpd.data(), fr.data()), BAD);
  // host constants: every name (the det KKT of a CARLA configuration), then the refusals
  mpcmmd_config cfg{};
  cfg.num_reduced = 4, cfg.num_obs = 2, cfg.noise_level = 0.1f, cfg.num_prime = 8, cfg.num_batch = 32;
  cfg.maxiter_cem = 2;
  for (const char* name : {"P", "Pdot", "Pddot", "P_prime", "P64", "Pdot64", "Pddot64", "guess_kinv_x", "guess_kinv_y",
                           "proj_kinv_x", "proj_kinv_y", "fit", "det_kinv_x", "det_kinv_y"}) {
    cfg.variant = std::strncmp(name, "det_", 4) == 0 ? MPCMMD_VARIANT_CARLA_TOWN05 : MPCMMD_VARIANT_STATIC;
    const int cnt = mpcmmd_host_constant(&cfg, name, nullptr, 0);
    expect_true(name, cnt > 0);
    std::vector<double> v(cnt);
    expect(name, mpcmmd_host_constant(&cfg, name, v.data(), v.size()), cnt);
    expect("host_constant count too small", mpcmmd_host_constant(&cfg, name, v.data(), v.size() - 1), BAD);
  }
  expect("host_constant unknown name", mpcmmd_host_constant(&cfg, "no_such_constant", nullptr, 0), BAD);
  expect("host_constant null cfg", mpcmmd_host_constant(nullptr, "P", nullptr, 0), BAD);
  expect("host_constant null name", mpcmmd_host_constant(&cfg, nullptr, nullptr, 0), BAD);
  // dynamic obstacle tracks of two obstacles
  const int O = 2;
  const std::vector<float> x0 = {30.0f, 40.0f}, y0 = {1.75f, -1.75f}, vx0 = {3.0f, 4.0f}, vy0 = {0.0f, 0.1f};
  const std::vector<float> vd = {4.0f, 5.0f};
  std::vector<float> xt(size_t(O) * kNum), yt(size_t(O) * kNum);
  expect("obs_dynamic_traj", mpcmmd_obs_dynamic_traj(O, x0.data(), y0.data(), vx0.data(), vy0.data(), vd.data(), -1.75f,
                                                     xt.data(), yt.data()), OK);
  expect("obs_dynamic_traj 0",
         mpcmmd_obs_dynamic_traj(0, nullptr, nullptr, nullptr, nullptr, nullptr, -1.75f, nullptr, nullptr), OK);
  expect("obs_dynamic_traj -1", mpcmmd_obs_dynamic_traj(-1, x0.data(), y0.data(), vx0.data(), vy0.data(), vd.data(),
                                                        -1.75f, xt.data(), yt.data()), BAD);
  expect("obs_dynamic_traj null", mpcmmd_obs_dynamic_traj(O, x0.data(), nullptr, vx0.data(), vy0.data(), vd.data(),
                                                          -1.75f, xt.data(), yt.data()), BAD);
  int32_t lo = -1, hi = -1;
  float wl = 0.0f, wh = 0.0f;
  expect("quantile_position", mpcmmd_quantile_position(10, 0.95f, &lo, &hi, &wl, &wh), OK);
  expect_true("quantile_position values", lo == 8 && hi == 9 && wl + wh == 1.0f);
  expect("quantile_position n 0", mpcmmd_quantile_position(0, 0.5f, &lo, &hi, &wl, &wh), BAD);
  expect("quantile_position alpha", mpcmmd_quantile_position(10, 1.5f, &lo, &hi, &wl, &wh), BAD);
  expect("quantile_position null", mpcmmd_quantile_position(10, 0.5f, nullptr, &hi, &wl, &wh), BAD);
}

// mpcmmd_create_batch's range check at each boundary it names
static void create_range_cases() {
  const int OK = MPCMMD_OK, BAD = MPCMMD_E_INVALID, UNS = MPCMMD_E_UNSUPPORTED;
  mpcmmd_config base{};
  base.num_reduced = 4, base.num_obs = 3, base.noise_level = 0.1f, base.num_prime = 10, base.num_batch = 32;
  base.maxiter_cem = 2;
  auto with = [&](int32_t mpcmmd_config::*field, int32_t value) {
    mpcmmd_config c = base;
    c.*field = value;
    return c;
  };
  expect("base", check_create_ranges(base, 1), OK);
  expect("max_configs 0", check_create_ranges(base, 0), BAD);
  expect("num_batch 19", check_create_ranges(with(&mpcmmd_config::num_batch, 19), 1), BAD);
  expect("num_batch 20", check_create_ranges(with(&mpcmmd_config::num_batch, 20), 1), OK);
  expect("num_batch 4096", check_create_ranges(with(&mpcmmd_config::num_batch, 4096), 1), OK);
  expect("num_batch 4097", check_create_ranges(with(&mpcmmd_config::num_batch, 4097), 1), BAD);
  expect("num_prime 1", check_create_ranges(with(&mpcmmd_config::num_prime, 1), 1), BAD);
  expect("num_prime 2", check_create_ranges(with(&mpcmmd_config::num_prime, 2), 1), OK);
  expect("num_prime 100", check_create_ranges(with(&mpcmmd_config::num_prime, 100), 1), OK);
  expect("num_prime 101", check_create_ranges(with(&mpcmmd_config::num_prime, 101), 1), BAD);
  expect("num_reduced 1", check_create_ranges(with(&mpcmmd_config::num_reduced, 1), 1), BAD);
  expect("num_reduced 2", check_create_ranges(with(&mpcmmd_config::num_reduced, 2), 1), OK);
  expect("num_reduced 1024", check_create_ranges(with(&mpcmmd_config::num_reduced, 1024), 1), OK);
  expect("num_reduced 1025", check_create_ranges(with(&mpcmmd_config::num_reduced, 1025), 1), UNS);
  mpcmmd_config c = with(&mpcmmd_config::num_prime, 2);  // num_obs * num_prime: 4096 * 2, then 2731 * 3
  c.num_obs = 4096;
  expect("num_obs * num_prime 8192", check_create_ranges(c, 1), OK);
  c.num_obs = 2731, c.num_prime = 3;
  expect("num_obs * num_prime 8193", check_create_ranges(c, 1), UNS);
  expect("65535 candidates", check_create_ranges(with(&mpcmmd_config::num_batch, 3855), 17), OK);
  expect("65536 candidates", check_create_ranges(with(&mpcmmd_config::num_batch, 4096), 16), UNS);
}

// buffers.hpp's list for five shapes: unique names, every buffer the shape has
// of at least one byte, a staging area that holds every staged buffer
static void buffer_list_cases() {
  const BufferShape shapes[] = {
      //  B     S   H   O   n    M       T  Gmax R0  beta   mmd_ok carla  stampw
      {32, 4, 10, 3, 4, 16, 2, 1, 0, false, true, false, false},            // static Gaussian
      {32, 4, 10, 3, 4, 16, 2, 1, 0, true, true, false, false},             // Beta noise
      {32, 4, 10, 3, 4, 16, 2, 3, 0, false, true, false, false},            // batch handle
      {1024, 500, 30, 10, 500, 250000, 2, 1, 0, true, false, false, false},  // no mmd_opt
      {32, 4, 10, 3, 4, 16, 2, 1, 16, false, true, true, false},            // CARLA
  };
  for (const BufferShape& sh : shapes) {
    const std::vector<BufferSpec> specs = buffer_specs(sh);
    std::set<std::string> names;
    size_t staged = 0;
    size_t present = 0;
    for (const BufferSpec& b : specs) {
      expect_true(b.name, names.insert(b.name).second);
      present += b.bytes >= 1;  // 0: the shape has no such buffer
      if (b.staged) staged += b.bytes;
    }
    // all but dbgw, the Beta attempt table, the 29 mmd_opt and the 8 CARLA buffers exist for every shape
    expect("buffers present", int(present),
           int(specs.size()) - 1 - (sh.beta_noise ? 0 : 1) - (sh.mmd_ok ? 0 : 29) - (sh.carla ? 0 : 8));
    expect_true("staging capacity", staging_bytes(specs) >= staged);
  }
}

// episodes_host.cpp: the validation stage's configuration check at each rejection and one acceptance,
// the log's interleave at ticks = 2, E = 3 for both count widths against a table written out by
// hand, and a tick's idx_mpc where the 32-bit sum wraps
static void episode_host_cases() {
  const int OK = MPCMMD_OK, BAD = MPCMMD_E_INVALID;
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  const float good[8] = {0.1f, 0.2f, 0.3f, 0.4f, 0.5f, 0.6f, 0.7f, 0.8f};
  int32_t lo = -1, hi = -1;
  float w_lo = 0.0f, w_hi = 0.0f;
  auto check = [&](int R, float alpha, int S, const float* sigma) {
    return check_risk_config("t", R, alpha, S, sigma, &lo, &hi, &w_lo, &w_hi);
  };
  expect("risk config", check(10, 0.95f, 8, good), OK);
  expect_true("risk config quantile", lo == 8 && hi == 9 && w_lo + w_hi == 1.0f);
  expect("risk config edges", check(1 << 20, 1.0f, 0, nullptr), OK);
  expect("risk config R 1, alpha 0", check(1, 0.0f, 0, nullptr), OK);
  expect("risk config R 0", check(0, 0.5f, 0, nullptr), BAD);
  expect_true("risk config text", std::string(mpcmmd_last_error()) == "t validation: num_rollouts out of 1..2^20");
  expect("risk config R -1", check(-1, 0.5f, 0, nullptr), BAD);
  expect("risk config R 2^20 + 1", check((1 << 20) + 1, 0.5f, 0, nullptr), BAD);
  expect("risk config alpha < 0", check(10, -0.01f, 0, nullptr), BAD);
  expect("risk config alpha > 1", check(10, 1.01f, 0, nullptr), BAD);
  expect("risk config alpha NaN", check(10, nan, 0, nullptr), BAD);
  expect_true("risk config text", std::string(mpcmmd_last_error()) == "t validation: alpha out of [0, 1]");
  expect("risk config S -1", check(10, 0.5f, -1, good), BAD);
  expect("risk config S 9", check(10, 0.5f, 9, good), BAD);
  expect_true("risk config text", std::string(mpcmmd_last_error()) == "t validation: num_sigma out of [0, 8]");
  for (float bad : {0.0f, -0.3f, inf, nan}) {
    const float sigma[2] = {0.3f, bad};
    expect("risk config sigma", check(10, 0.5f, 2, sigma), BAD);
    expect_true("risk config text",
                std::string(mpcmmd_last_error()) == "t validation: every sigma must be finite and > 0");
    expect("risk config sigma beyond S", check(10, 0.5f, 1, sigma), OK);
  }
  // n = ticks * E = 6 rows: plane k of the counts holds 100 k + i, statistic k of row i holds
  // 1000 k + 10 i + channel
  const size_t n = 2 * 3;
  std::vector<int32_t> planes(3 * n);
  std::vector<float> stat_planes(4 * n * 3);
  for (size_t k = 0; k < 3; ++k)
    for (size_t i = 0; i < n; ++i) planes[k * n + i] = int32_t(100 * k + i);
  for (size_t k = 0; k < 4; ++k)
    for (size_t i = 0; i < n; ++i)
      for (size_t ch = 0; ch < 3; ++ch) stat_planes[(k * n + i) * 3 + ch] = float(1000 * k + 10 * i + ch);
  const int32_t want2[12] = {0, 100, 1, 101, 2, 102, 3, 103, 4, 104, 5, 105};
  const int32_t want3[18] = {0, 100, 200, 1, 101, 201, 2, 102, 202, 3, 103, 203, 4, 104, 204, 5, 105, 205};
  const float want_stats[12] = {20, 21, 22, 1020, 1021, 1022, 2020, 2021, 2022, 3020, 3021, 3022};  // row i = 2
  for (int nc : {2, 3}) {
    std::vector<int32_t> counts(n * nc, -1);   // exactly the documented sizes: a write past them is ASan's to find
    std::vector<float> stats(n * 12, -1.0f);
    interleave_risk_log(n, nc, planes.data(), stat_planes.data(), counts.data(), stats.data());
    expect_true("interleave counts", std::memcmp(counts.data(), nc == 2 ? want2 : want3, counts.size() * 4) == 0);
    expect_true("interleave stats", std::memcmp(stats.data() + 2 * 12, want_stats, sizeof want_stats) == 0);
    expect_true("interleave stats ends", stats[0] == 0.0f && stats[n * 12 - 1] == 3052.0f);
  }
  // keys -1 and 7 at tick 2^20 - 1: the sum wraps in uint32 to 2^20 - 2; the covariance once per episode
  const std::vector<uint32_t> keys = {0xFFFFFFFFu, 7u, 0x7FFFFFFFu};
  std::vector<int32_t> idx(keys.size(), 0);
  tick_indices((1 << 20) - 1, keys, idx.data());
  expect_true("tick_indices",
              idx[0] == (1 << 20) - 2 && idx[1] == (1 << 20) + 6 && idx[2] == INT32_MIN + (1 << 20) - 2);
  tick_indices(0, keys, idx.data());
  expect_true("tick_indices tick 0", idx[0] == -1 && idx[1] == 7 && idx[2] == INT32_MAX);
  std::vector<float> cov(64);
  for (int i = 0; i < 64; ++i) cov[i] = float(i);
  const std::vector<float> covs = replicate_cov(cov.data(), 3);
  expect_true("replicate_cov", covs.size() == 192 && covs[64] == 0.0f && covs[191] == 63.0f && covs[127] == 63.0f);
  expect_true("replicate_cov none", replicate_cov(cov.data(), 0).empty());
}

int main(int argc, char** argv) {
  api_cases();
  create_range_cases();
  buffer_list_cases();
  episode_host_cases();
  for (int variant = 0; variant < 4; ++variant) {
    for (int H : {2, 8, 20, 30, 50, 60, 100}) {
      if (variant >= 2 && H > 100) continue;
      ProblemConsts c = build_constants(H, variant);
      emit("const", H, variant, "P", c.P);
      emit("const", H, variant, "P_prime", c.P_prime);
      emit("const", H, variant, "guess_kinv_x", c.guess_kinv_x);
      emit("const", H, variant, "guess_kinv_y", c.guess_kinv_y);
      emit("const", H, variant, "proj_kinv_x", c.proj_kinv_x);
      emit("const", H, variant, "proj_kinv_y", c.proj_kinv_y);
      emit("const", H, variant, "fit", c.fit);
    }
  }
  const DynObsConsts d = build_dyn_obs_consts();
  const int O = 20;
  std::vector<float> x0(O), y0(O), vx0(O), vy0(O), vd(O), xt(O * 100), yt(O * 100);
  for (int i = 0; i < O; ++i) {
    x0[i] = 30.0f + 5.0f * i;
    y0[i] = i % 2 ? 1.75f : -1.75f;
    vx0[i] = 3.0f + 0.5f * i;
    vy0[i] = 0.1f * (i % 3);
    vd[i] = 4.0f + 0.25f * i;
  }
  dyn_obs_traj(d, O, x0.data(), y0.data(), vx0.data(), vy0.data(), vd.data(), -1.75f, xt.data(), yt.data());
  std::vector<double> xs(xt.begin(), xt.end()), ys(yt.begin(), yt.end());
  emit("dyn", 0, 1, "x_traj", xs);
  emit("dyn", 0, 1, "y_traj", ys);

  if (argc > 1 && !(g_rec = std::fopen(argv[1], "w"))) {
    std::perror(argv[1]);
    return 2;
  }
  const TestPath p4 = path_case(4), p50 = path_case(50);
  begin_case(2, 1);
  begin_case(100, 32);
  carla_case(2, 2, 1, p4);
  carla_case(4, 100, 32, p50);
  carla_case(6, 100, 32, p50);
  for (int n : {2, 4, 6}) beta_case(n);
  if (g_rec) std::fclose(g_rec);
  return 0;
}
