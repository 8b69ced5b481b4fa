#include "solve_host.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <stdexcept>

#include "layout.hpp"

namespace mpcmmd {

bool chol8(const double* a, double* L) {
  for (int i = 0; i < 64; ++i) L[i] = 0.0;
  for (int j = 0; j < 8; ++j) {
    double d = a[j * 8 + j];
    for (int k = 0; k < j; ++k) d -= L[j * 8 + k] * L[j * 8 + k];
    if (!(d > 0.0)) return false;
    d = std::sqrt(d);
    L[j * 8 + j] = d;
    for (int i = j + 1; i < 8; ++i) {
      double s = a[i * 8 + j];
      for (int k = 0; k < j; ++k) s -= L[i * 8 + k] * L[j * 8 + k];
      L[i * 8 + j] = s / d;
    }
  }
  return true;
}

std::vector<float> pack_basis(const ProblemConsts& pc) {
  std::vector<float> basis(3 * kNum * kNvar);
  for (int i = 0; i < kNum * kNvar; ++i) {
    basis[i] = float(pc.P[i]);
    basis[kNum * kNvar + i] = float(pc.Pd[i]);
    basis[2 * kNum * kNvar + i] = float(pc.Pdd[i]);
  }
  return basis;
}

std::vector<double> pack_guess_g(const ProblemConsts& pc) {
  std::vector<double> gg(2 * kNvar * 4);
  for (int xy = 0; xy < 2; ++xy) {
    const auto& Ki = xy == 0 ? pc.guess_kinv_x : pc.guess_kinv_y;
    const auto& cs = xy == 0 ? pc.guess_colsum_x : pc.guess_colsum_y;
    const int n = xy == 0 ? 14 : 15;
    const double kp = xy == 0 ? pc.k_p_v : pc.k_p;
    for (int k = 0; k < kNvar; ++k)
      for (int j = 0; j < 4; ++j) {
        double s = 0.0;
        for (int i = 0; i < kNvar; ++i) s += Ki[k * n + i] * (-kp * cs[j * kNvar + i]);
        gg[(xy * kNvar + k) * 4 + j] = s;
      }
  }
  return gg;
}

std::vector<double> pack_proj_m(const std::vector<double>& kx, const std::vector<double>& ky) {
  std::vector<double> pm(2 * kNvar * kNvar);
  for (int xy = 0; xy < 2; ++xy) {
    const auto& Ki = xy == 0 ? kx : ky;
    const int n = xy == 0 ? 14 : 15;
    for (int k = 0; k < kNvar; ++k)
      for (int j = 0; j < kNvar; ++j) pm[(xy * kNvar + k) * kNvar + j] = Ki[k * n + j];
  }
  return pm;
}

void solve_columns(const ProblemConsts& pc, const double* proj_kx, const double* proj_ky, const double bx[3],
                   const double by[4], double* sc) {
  for (int k = 0; k < 4 * kNvar; ++k) sc[k] = 0.0;
  for (int k = 0; k < kNvar; ++k) {
    for (int e = 0; e < 3; ++e) sc[0 * kNvar + k] += pc.guess_kinv_x[k * 14 + kNvar + e] * bx[e];
    for (int e = 0; e < 4; ++e) sc[1 * kNvar + k] += pc.guess_kinv_y[k * 15 + kNvar + e] * by[e];
    for (int e = 0; e < 3; ++e) sc[2 * kNvar + k] += proj_kx[k * 14 + kNvar + e] * bx[e];
    for (int e = 0; e < 4; ++e) sc[3 * kNvar + k] += proj_ky[k * 15 + kNvar + e] * by[e];
  }
}

void initial_state(const float* is, float* s0) {
  s0[0] = is[0], s0[1] = is[1], s0[2] = is[2], s0[3] = is[3], s0[4] = atan2f(is[3], is[2]);
  s0[5] = s0[6] = s0[7] = 0.f;
}

void obstacle_transpose(const float* xo, const float* yo, int O, int H, float* out) {
  for (int o = 0; o < O; ++o)
    for (int t = 0; t < H; ++t) {
      out[size_t(o) * H + t] = xo[o * kNum + t];
      out[size_t(O) * H + o * H + t] = yo[o * kNum + t];
    }
}

void initial_population(const float* mean, const float* cov, const float* z, int B, float* pop) {
  double cv[64], L[64];
  for (int i = 0; i < 64; ++i) cv[i] = double(cov[i]);
  if (!chol8(cv, L)) throw std::invalid_argument("cov_param_init is not positive definite");
  for (int b = 0; b < B; ++b)
    for (int a = 0; a < 8; ++a) {
      double s = double(mean[a]);
      for (int c = 0; c <= a; ++c) s += L[a * 8 + c] * double(z[size_t(b) * 8 + c]);
      float v = float(s);
      if (a < 4) v = fminf(fmaxf(v, 0.1f), 30.0f);
      pop[size_t(b) * 8 + a] = v;
    }
}

std::vector<float> roll_transpose(const float* roll, int T, int S, int H) {
  std::vector<float> r(size_t(T) * 3 * H * S);
  for (int t = 0; t < T; ++t)
    for (int k = 0; k < 3; ++k)
      for (int s = 0; s < S; ++s)
        for (int q = 0; q < H; ++q)
          r[((size_t(t) * 3 + k) * H + q) * S + s] = roll[((size_t(t) * 3 + k) * S + s) * H + q];
  return r;
}

PathView path_view(int num_path, const float* x, const float* y, const float* arc, const float* Fxd,
                   const float* Fyd, const float* kappa) {
  PathView pv;
  pv.P = num_path, pv.x = x, pv.y = y, pv.arc = arc;
  pv.Fxd = Fxd, pv.Fyd = Fyd, pv.kappa = kappa;
  return pv;
}

void carla_velocity_heading(float v0, float psi0, float* vx, float* vy, float* psi) {
  *vx = v0 * float(std::cos(double(psi0)));
  *vy = v0 * float(std::sin(double(psi0)));
  *psi = float(std::atan2(double(*vy), double(*vx)));
}

void carla_rows(const ProblemConsts& pc, int R, int R0, const float* is, const PathView& pv, const float* eps,
                std::vector<float>& rows, double* bx, double* by) {
  const float x0 = is[0], y0 = is[1], v0 = is[2], vdot = is[3], psi0 = is[4], psidot = is[5];
  float vx, vy, psi;
  carla_velocity_heading(v0, psi0, &vx, &vy, &psi);
  const float mux = float(pc.init_mu_x), muy = float(pc.init_mu_y);
  const float sgx = float(pc.init_sigma_x), sgy = float(pc.init_sigma_y);
  rows.assign(size_t(R0) * 8, 0.0f);
  double sum[6] = {0, 0, 0, 0, 0, 0};
  for (int r = 0; r < R; ++r) {
    float* o = rows.data() + size_t(r) * 8;
    o[0] = x0 + (eps[size_t(r) * 4] * sgx + mux);
    o[1] = y0 + (eps[size_t(r) * 4 + 1] * sgy + muy);
    o[2] = vx;
    o[3] = vy;
    o[4] = psi;
    const float v = std::sqrt(vx * vx + vy * vy);
    const FrenetState f = global_to_frenet(pv, o[0], o[1], v, vdot, psi, psidot);
    const float vals[6] = {f.x, f.y, f.vx, f.vy, f.ax, f.ay};
    for (int k = 0; k < 6; ++k) sum[k] += double(vals[k]);  // sequential (the oracle's cumsum order)
  }
  float m[6];
  for (int k = 0; k < 6; ++k) m[k] = float(sum[k] / double(R));
  bx[0] = m[0], bx[1] = m[2], bx[2] = m[4];
  by[0] = m[1], by[1] = m[3], by[2] = m[5], by[3] = 0.0;
}

void carla_rows_batch(const ProblemConsts& pc, int G, int R, int R0, const float* init_state, const PathView* paths,
                      const float* const* eps, std::vector<float>& rows, double* bx, double* by) {
  rows.assign(size_t(G) * R0 * 8, 0.0f);
  std::vector<float> one;
  for (int g = 0; g < G; ++g) {
    carla_rows(pc, R, R0, init_state + size_t(g) * 6, paths[g], eps[g], one, bx + size_t(g) * 3, by + size_t(g) * 4);
    std::memcpy(rows.data() + size_t(g) * R0 * 8, one.data(), one.size() * 4);
  }
}

std::vector<float> path_image(int G, const PathView* paths) {
  std::vector<float> img(size_t(G) * 6 * kMaxPath, 0.0f);
  for (int g = 0; g < G; ++g) {
    const PathView& pv = paths[g];
    if (pv.P < 1 || pv.P > kMaxPath) throw std::invalid_argument("path image: num_path out of range");
    const float* arrs[6] = {pv.x, pv.y, pv.arc, pv.Fxd, pv.Fyd, pv.kappa};
    for (int k = 0; k < 6; ++k) std::memcpy(img.data() + (size_t(g) * 6 + k) * kMaxPath, arrs[k], size_t(pv.P) * 4);
  }
  return img;
}

std::vector<float> det_track_image(int G, int O, const float* x_obs, const float* y_obs) {
  const size_t one = size_t(O) * kNum;
  std::vector<float> img(size_t(G) * 2 * one);
  for (int g = 0; g < G; ++g) {
    std::memcpy(img.data() + (size_t(g) * 2) * one, x_obs + size_t(g) * one, one * 4);
    std::memcpy(img.data() + (size_t(g) * 2 + 1) * one, y_obs + size_t(g) * one, one * 4);
  }
  return img;
}

CarlaBatch carla_batch(const ProblemConsts& pc, int G, int R, int R0, int O, bool det, const float* init_state,
                       const PathView* paths, const float* const* eps, const float* x_obs, const float* y_obs) {
  CarlaBatch cb;
  cb.bx.assign(size_t(G) * 3, 0.0);
  cb.by.assign(size_t(G) * 4, 0.0);
  carla_rows_batch(pc, G, R, R0, init_state, paths, eps, cb.rows, cb.bx.data(), cb.by.data());
  cb.path = path_image(G, paths);
  if (det) cb.tracks = det_track_image(G, O, x_obs, y_obs);
  return cb;
}

std::vector<CarlaBatch::Piece> CarlaBatch::staged() const {
  std::vector<Piece> out = {{"st0r", &rows}, {"path", &path}};
  if (!tracks.empty()) out.push_back({"obs_full", &tracks});
  return out;
}

void plan_controls(const float* v_all, const float* steer, int K, int H, std::vector<float>& acc,
                   std::vector<float>& steer_out) {
  acc.assign(size_t(K) * H, 0.0f);
  steer_out.assign(size_t(K) * H, 0.0f);
  for (int k = 0; k < K; ++k) {
    const float* v = v_all + size_t(k) * kNum;
    for (int h = 0; h < H; ++h) {
      const float vn = h + 1 < kNum ? v[h + 1] : v[kNum - 1];
      acc[size_t(k) * H + h] = (vn - v[h]) / 0.15f;  // prob.t (rollout.hpp: kDt)
      steer_out[size_t(k) * H + h] = steer[size_t(k) * kNum + h];
    }
  }
}

Sel0Tables first_selection_tables(const int32_t* sel, const float* sig, int n, int M) {
  const int np = kBetaSamples * n;
  Sel0Tables t;
  std::vector<int32_t>& rp = t.rp;
  std::vector<int32_t>& pairs = t.pairs;
  rp.assign(M + 1, 0);
  pairs.assign(2 * size_t(np), 0);  // (i, sigma bits): one 8-byte load per pair
  for (int i = 0; i < np; ++i) {
    if (sel[i] < 0 || sel[i] >= M) throw std::runtime_error("first beta-iteration selection out of range");
    ++rp[sel[i] + 1];
  }
  for (int r = 0; r < M; ++r) rp[r + 1] += rp[r];
  std::vector<int32_t> fill(rp.begin(), rp.end() - 1);
  for (int i = 0; i < np; ++i) {
    const int at = fill[sel[i]]++;
    pairs[2 * at] = i;
    std::memcpy(&pairs[2 * at + 1], &sig[i / n], 4);
  }
  // k_bmoment_rows' row order: descending number of distinct sigmas among a
  // row's pairs (its direct-sum rounds), so a wave's four rows need about the
  // same number
  std::vector<int32_t> nsig(M, 0);
  t.rperm.resize(M);
  for (int r = 0; r < M; ++r) {
    t.rperm[r] = r;
    std::vector<int32_t> sg;
    for (int q = rp[r]; q < rp[r + 1]; ++q) sg.push_back(pairs[2 * q + 1]);
    std::sort(sg.begin(), sg.end());
    nsig[r] = int(std::unique(sg.begin(), sg.end()) - sg.begin());
  }
  std::stable_sort(t.rperm.begin(), t.rperm.end(), [&](int a, int c) { return nsig[a] > nsig[c]; });
  return t;
}

std::vector<float> beta_z_image(const float* z, int M) {
  const int M1 = M + 1, R = kBetaSamples - kBetaElite;
  std::vector<float> tr(size_t(pos_pad(M)) * kBzCols, 0.0f);
  for (int r = 0; r < R; ++r)
    for (int j = 0; j < M1; ++j) tr[bz_index(j, r)] = z[size_t(r) * M1 + j];
  return tr;
}

void plan_speed(const ProblemConsts& pc, const float* cx, const float* cy, float* v_best) {
  for (int i = 0; i < kNum; ++i) {
    double sx = 0.0, sy = 0.0;
    for (int k = 0; k < kNvar; ++k) {
      sx += pc.Pd[i * kNvar + k] * double(cx[k]);
      sy += pc.Pd[i * kNvar + k] * double(cy[k]);
    }
    const float xd = float(sx), yd = float(sy);
    v_best[i] = std::sqrt(xd * xd + yd * yd);
  }
}

}  // namespace mpcmmd
