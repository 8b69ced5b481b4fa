// Sanitizer harness of the CARLA batch setup (csrc/solve_host.cpp:
// carla_rows_batch, path_image, det_track_image, carla_batch), built by
// `make -C mpc-mmd_amd asan_batch` from the host-only sources with
// -fsanitize=address,undefined -fno-sanitize-recover and run by
// tests/test_carla_batch_cpu.py as a child process.  For G = 3 configurations
// with three different paths it checks
//   rows    the slices and boundary vectors of carla_rows_batch equal three
//           carla_rows calls bit for bit, for R = n^2, n and 1 with R0 > R
//   path    array k of path g starts at (g 6 + k) kMaxPath, the rest is zero
//   tracks  the det track image is [G][2][O][100]
//   pieces  the staged copies per buffer do not depend on G, each within the
//           pieces buffers.hpp declares, and a begin's copies fit the staging area
// Exit status 0 and "ok" on success; the first failed check prints and exits 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../mpc-mmd_amd/csrc/buffers.hpp"
#include "../../mpc-mmd_amd/csrc/host_constants.hpp"
#include "../../mpc-mmd_amd/csrc/layout.hpp"
#include "../../mpc-mmd_amd/csrc/solve_host.hpp"

using namespace mpcmmd;

static uint32_t g_lcg = 2024u;
static float rnd() {
  g_lcg = g_lcg * 1664525u + 1013904223u;
  return float(int32_t((g_lcg >> 8) & 0xFFFF) - 32768) / 32768.0f;
}

static void expect(bool ok, const char* what, int a = 0, int b = 0) {
  if (ok) return;
  std::printf("FAILED %s (%d, %d)\n", what, a, b);
  std::exit(1);
}

struct TestPath {
  std::vector<float> x, y, Fxd, Fyd, Fxdd, Fydd, arc, kappa;
  PathView view() const {
    return path_view(int(x.size()), x.data(), y.data(), arc.data(), Fxd.data(), Fyd.data(), kappa.data());
  }
};

// a smoothed path of P points, bending by `bend`
static TestPath make_path(int P, float bend) {
  std::vector<float> xw(P), yw(P);
  for (int i = 0; i < P; ++i) {
    xw[i] = 2.0f * float(i) + 0.25f * rnd();
    yw[i] = bend * float(i) * float(i) + 0.25f * rnd();
  }
  TestPath p;
  for (auto* v : {&p.x, &p.y, &p.Fxd, &p.Fyd, &p.Fxdd, &p.Fydd, &p.arc, &p.kappa}) v->assign(P, 0.0f);
  path_smoothing(P, xw.data(), yw.data(), 0.1f, p.x.data(), p.y.data());
  float arc_length = 0.0f;
  path_parameters(P, p.x.data(), p.y.data(), p.Fxd.data(), p.Fyd.data(), p.Fxdd.data(), p.Fydd.data(), p.arc.data(),
                  p.kappa.data(), &arc_length);
  return p;
}

int main() {
  const int G = 3, n = 3, M = n * n, H = 20, O = 2, P = 40, B = 22, T = 2;
  const int R0 = M + 3;  // more rows than any R below: the tail of every slice stays zero
  const ProblemConsts pc = build_constants(H, 2);
  const TestPath tp[G] = {make_path(P, 0.02f), make_path(P, -0.03f), make_path(P, 0.0f)};
  std::vector<PathView> views;
  for (const TestPath& p : tp) views.push_back(p.view());
  std::vector<float> is(size_t(G) * 6);
  for (int g = 0; g < G; ++g) {
    float* q = &is[size_t(g) * 6];
    q[0] = 1.0f + rnd(), q[1] = 0.3f * rnd(), q[2] = 6.0f + float(g) + rnd();
    q[3] = 0.2f * rnd(), q[4] = 0.1f * rnd(), q[5] = 0.02f * rnd();
  }
  std::vector<float> xo(size_t(G) * O * kNum), yo(xo.size());
  for (size_t i = 0; i < xo.size(); ++i) xo[i] = 40.0f + 30.0f * rnd(), yo[i] = 3.0f * rnd();

  // ---- rows ------------------------------------------------------------------
  for (int R : {M, n, 1}) {
    std::vector<std::vector<float>> eps(G);
    std::vector<const float*> ep(G);
    for (int g = 0; g < G; ++g) {
      eps[g].resize(size_t(R) * 4);
      for (float& v : eps[g]) v = 2.0f * rnd();
      ep[g] = eps[g].data();
    }
    std::vector<float> rows;
    std::vector<double> bx(size_t(G) * 3, -1.0), by(size_t(G) * 4, -1.0);
    carla_rows_batch(pc, G, R, R0, is.data(), views.data(), ep.data(), rows, bx.data(), by.data());
    expect(rows.size() == size_t(G) * R0 * 8, "rows size", int(rows.size()), G * R0 * 8);
    bool differ = false;
    for (int g = 0; g < G; ++g) {
      std::vector<float> one;
      double b1[3], b2[4];
      carla_rows(pc, R, R0, &is[size_t(g) * 6], views[g], ep[g], one, b1, b2);
      expect(one.size() == size_t(R0) * 8, "carla_rows size", g, R);
      expect(std::memcmp(one.data(), &rows[size_t(g) * R0 * 8], one.size() * 4) == 0, "rows slice", g, R);
      expect(std::memcmp(b1, &bx[size_t(g) * 3], sizeof b1) == 0, "bx slice", g, R);
      expect(std::memcmp(b2, &by[size_t(g) * 4], sizeof b2) == 0, "by slice", g, R);
      for (size_t i = size_t(R) * 8; i < one.size(); ++i) expect(one[i] == 0.0f, "rows past R are zero", g, int(i));
      if (g > 0) differ |= std::memcmp(&rows[0], &rows[size_t(g) * R0 * 8], size_t(R) * 8 * 4) != 0;
    }
    expect(differ, "the configurations' rows differ (a degenerate case shows nothing)", R);
  }

  // ---- path image ------------------------------------------------------------
  {
    const std::vector<float> img = path_image(G, views.data());
    expect(img.size() == size_t(G) * 6 * kMaxPath, "path image size", int(img.size()));
    for (int g = 0; g < G; ++g) {
      const float* arrs[6] = {tp[g].x.data(),   tp[g].y.data(),   tp[g].arc.data(),
                              tp[g].Fxd.data(), tp[g].Fyd.data(), tp[g].kappa.data()};
      for (int k = 0; k < 6; ++k) {
        const float* at = &img[(size_t(g) * 6 + k) * kMaxPath];
        expect(std::memcmp(at, arrs[k], size_t(P) * 4) == 0, "path array", g, k);
        for (int i = P; i < kMaxPath; ++i) expect(at[i] == 0.0f, "path padding", g, k);
      }
    }
    expect(std::memcmp(&img[0], &img[size_t(6) * kMaxPath], size_t(P) * 4) != 0, "paths 0 and 1 differ");
  }

  // ---- det tracks ------------------------------------------------------------
  {
    const std::vector<float> img = det_track_image(G, O, xo.data(), yo.data());
    expect(img.size() == size_t(G) * 2 * O * kNum, "track image size", int(img.size()));
    for (int g = 0; g < G; ++g)
      for (int o = 0; o < O; ++o)
        for (int i = 0; i < kNum; ++i) {
          expect(img[((size_t(g) * 2 + 0) * O + o) * kNum + i] == xo[(size_t(g) * O + o) * kNum + i], "x track", g, o);
          expect(img[((size_t(g) * 2 + 1) * O + o) * kNum + i] == yo[(size_t(g) * O + o) * kNum + i], "y track", g, o);
        }
  }

  // ---- staged pieces ---------------------------------------------------------
  for (bool det : {false, true}) {
    const int R = det ? 1 : n;
    size_t pieces1 = 0;
    for (int g = 1; g <= G; ++g) {  // a batch of g configurations on a handle of g
      std::vector<std::vector<float>> eps(g, std::vector<float>(size_t(R) * 4, 0.5f));
      std::vector<const float*> ep;
      for (auto& e : eps) ep.push_back(e.data());
      const CarlaBatch cb = carla_batch(pc, g, R, R0, O, det, is.data(), views.data(), ep.data(), xo.data(), yo.data());
      const std::vector<CarlaBatch::Piece> st = cb.staged();
      if (g == 1) pieces1 = st.size();
      expect(st.size() == pieces1, "staged copies do not depend on G", int(st.size()), int(pieces1));
      expect(st.size() == (det ? 3u : 2u), "staged copies", int(st.size()));
      const BufferShape sh{B, n, H, O, n, M, T, g, R0, false, true, true, false};
      const std::vector<BufferSpec> specs = buffer_specs(sh);
      std::map<std::string, int> count;
      for (const CarlaBatch::Piece& p : st) {
        ++count[p.buffer];
        bool found = false;
        for (const BufferSpec& b : specs)
          if (p.buffer == std::string(b.name)) {
            found = true;
            expect(count[p.buffer] <= b.staged, "pieces within the declared count", g, b.staged);
            expect(p.image->size() * 4 == b.bytes, "a piece is the whole buffer of g configurations", g,
                   int(p.image->size()));
          }
        expect(found, "staged buffer exists", g);
      }
      // every staged buffer once, the CARLA ones as above: the begin's copies fit the pinned area
      size_t used = 0;
      for (const BufferSpec& b : specs)
        if (b.staged && b.bytes) used = ((used + 63) & ~size_t(63)) + b.bytes;
      expect(used <= staging_bytes(specs), "staging capacity", g, int(used));
    }
  }
  // an unequal num_path is the caller's to reject; a path longer than the image is refused here
  {
    PathView bad = views[0];
    bad.P = kMaxPath + 1;
    bool threw = false;
    try {
      (void)path_image(1, &bad);
    } catch (const std::invalid_argument&) {
      threw = true;
    }
    expect(threw, "path image refuses num_path > kMaxPath");
  }
  std::printf("ok\n");
  return 0;
}
