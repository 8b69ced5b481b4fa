// libmpcmmd: the per-solve setup (mpcmmd_begin and its variants: host
// arithmetic, uploads through the pinned staging area, the Beta tables) and
// the results (mpcmmd_finish), with the solve wrappers that chain them.
#include <cstring>
#include <stdexcept>
#include <vector>

#include "handle.hpp"
#include "rng.hpp"
#include "solve_host.hpp"

using namespace mpcmmd;

std::vector<float> mpcmmd::host_normals(uint32_t k0, uint32_t k1, uint32_t stream, uint32_t word1, size_t count) {
  std::vector<float> out(count);
  double z[4];
  for (size_t j = 0; j * 4 < count; ++j) {
    philox_normals4(k0, k1, stream, word1, uint32_t(j), z);
    for (int q = 0; q < 4 && j * 4 + q < count; ++q) out[j * 4 + q] = float(z[q]);
  }
  return out;
}

namespace {

// upload through the handle's pinned staging area (mpcmmd_begin): src may be
// a host temporary, the copy still runs after the call returns
void upload_staged(mpcmmd_handle* h, const void* dst, const void* src, size_t bytes, size_t offset = 0) {
  const size_t at = (h->stage_used + 63) & ~size_t(63);
  if (at + bytes > h->stage_bytes)
    throw std::runtime_error(std::string("staging area too small for ") + h->buf_of(dst).name);
  std::memcpy(h->stage + at, src, bytes);
  h->stage_used = at + bytes;
  upload(h, dst, h->stage + at, bytes, offset);
}

// bytes of the first G configurations' slices of a buffer sized for Gmax (buffers.hpp: G * ... and BT * ...)
size_t cfg_bytes(const mpcmmd_handle* h, const void* buf, int G) { return h->buf_of(buf).bytes / h->Gmax * G; }

// beta_z iteration t: [89][M+1] (draw order) in the device layout (beta_z_image)
void upload_beta_z(mpcmmd_handle* h, int t, const float* z) {
  const std::vector<float> tr = beta_z_image(z, h->M);
  upload(h, h->p.beta_z, tr.data(), tr.size() * 4, size_t(t) * tr.size() * 4);
  HIPC(hipStreamSynchronize(h->stream));  // tr is a host temporary
}

void gen_beta_tables(mpcmmd_handle* h) {
  const int M1 = h->M + 1;
  const uint32_t k0 = kFixedKey0, k1 = h->cfg.seed;
  auto z0 = host_normals(k0, k1, kStreamBetaZ0, 0, size_t(kBetaSamples) * M1);
  upload(h, h->p.beta_z0, z0.data(), z0.size() * 4);
  for (int t = 0; t < kBetaIters; ++t) {
    auto z = host_normals(k0, k1, kStreamBetaZ, uint32_t(t), size_t(kBetaSamples - kBetaElite) * M1);
    upload_beta_z(h, t, z.data());
  }
  HIPC(hipStreamSynchronize(h->stream));
  h->beta_tables_internal = true;
  h->sel0_valid = false;
}

}  // namespace

// mpcmmd_begin for n configurations (arrays with a leading configuration
// axis); external draws only for n == 1 (the parity contract)
int mpcmmd::begin_impl(mpcmmd_handle* h, int32_t n_cfg, int32_t cost_kind, const int32_t* idx_mpc,
                       const float* init_state, const float* mean, const float* cov, const float* x_obs,
                       const float* y_obs, const float* v_des, const mpcmmd_draws* draws, const mpcmmd_path* path,
                       const TickRoute* tick, bool resident) {
  // the resident route of the scene queue: idx_mpc and v_des are on the device already (k_mpc_queue wrote them)
  const bool queued = resident && !idx_mpc && !v_des;
  if (resident) {  // the synthetic closed loop (mpc_api.hip): only idx_mpc, cov and v_des come from the host
    if (!h || !cov || (!queued && (!idx_mpc || !v_des))) return fail(MPCMMD_E_INVALID, "null argument");
    if (h->carla || path || tick || draws)
      return fail(MPCMMD_E_INVALID, "the resident begin is the static / dynamic variants' own");
  } else if (!h || !idx_mpc || !init_state || !mean || !cov || (!tick && (!x_obs || !y_obs)) || !v_des) {
    return fail(MPCMMD_E_INVALID, "null argument");
  }
  if (h->carla != (path != nullptr || tick != nullptr))
    return fail(MPCMMD_E_INVALID, h->carla ? "CARLA handle: use mpcmmd_carla_begin / mpcmmd_carla_solve (a path is needed)"
                                           : "mpcmmd_carla_begin needs a handle of a CARLA variant");
  if (h->carla && cost_kind != MPCMMD_COST_MMD_OPT && cost_kind != MPCMMD_COST_CVAR && cost_kind != MPCMMD_COST_DET)
    return fail(MPCMMD_E_UNSUPPORTED,
                "the CARLA optimizer has compute_cem_mmd (mmd_opt), compute_cem_cvar and compute_cem_det only");
  if (!h->carla && cost_kind == MPCMMD_COST_DET)
    return fail(MPCMMD_E_INVALID, "compute_cem_det exists for the CARLA optimizer only");
  if (cost_kind == MPCMMD_COST_DET && h->O > kMaxDetObs)
    return fail(MPCMMD_E_UNSUPPORTED, "compute_cem_det: num_obs <= 32");
  if (cost_kind < 0 || cost_kind > 4) return fail(MPCMMD_E_INVALID, "cost_kind must be 0..4");
  if (n_cfg < 1 || n_cfg > h->Gmax) return fail(MPCMMD_E_INVALID, "n_cfg must be 1..max_configs of the handle");
  for (int g = 0; path && g < n_cfg; ++g) {
    const mpcmmd_path& q = path[g];
    if (q.num_path < 4 || q.num_path > kMaxPath || !q.x_path || !q.y_path || !q.arc_vec || !q.Fx_dot || !q.Fy_dot ||
        !q.kappa)
      return fail(MPCMMD_E_INVALID, "path: 4 <= num_path <= 2048 and six arrays");
    // Params::P is one scalar and the k_frenet / k_front LDS sizes depend on it
    if (q.num_path != path[0].num_path)
      return fail(MPCMMD_E_INVALID, "paths of one batch must have the same num_path");
  }
  if (draws && n_cfg > 1) return fail(MPCMMD_E_INVALID, "external draws need n_cfg == 1");
  if (cost_kind == MPCMMD_COST_MMD_OPT && !h->mmd_ok) return fail(MPCMMD_E_UNSUPPORTED, h->mmd_why);
  return guarded([&] {
    check_device(h);
    Params& p = h->p;
    const int B = h->B, S = h->S, H = h->H, O = h->O, T = h->T, G = n_cfg;
    if (h->stage_pending) HIPC(hipEventSynchronize(h->stage_ev));  // previous begin's copies done
    h->stage_pending = false;
    h->stage_used = 0;
    // a failure after the first staged copy: drain them before the staging area is reused
    struct DrainOnThrow {
      mpcmmd_handle* h;
      bool armed = true;
      ~DrainOnThrow() {
        if (armed) (void)hipStreamSynchronize(h->stream);
      }
    } drain{h};
    h->cost = cost_kind;
    h->G = G;
    p.cost = cost_kind;
    // k_select's residual sort and cost norms in the risk launch (cost.hpp):
    // the baseline rollouts on Beta / Gaussian planes (k_risk_baseline)
    p.select_prep = h->prep_on && !h->carla &&
                    (cost_kind == MPCMMD_COST_CVAR || cost_kind == MPCMMD_COST_SAA || cost_kind == MPCMMD_COST_MMD_RANDOM);
    p.G = G;
    p.Bt = G * B;
    p.b0 = 0;
    p.nb = p.Bt;
    // cem.py:161-163 weights (obs, lane); CARLA: carla/optimizer/cem.py:171-173 (+ desired lane)
    const float w_obs[5] = {1e3f, 1e3f, 1e3f, 1e6f, 0.f}, w_lane[5] = {0.f, 0.f, 0.f, 1e6f, 0.f};
    p.w_obs = w_obs[cost_kind];
    p.w_lane = w_lane[cost_kind];
    p.w_des = 0.0f;
    if (h->carla) {  // det: 0 * the zero risks (cem.py:750)
      p.w_obs = cost_kind == MPCMMD_COST_MMD_OPT ? 0.1f : cost_kind == MPCMMD_COST_DET ? 0.0f : 100.0f;
      p.w_lane = cost_kind == MPCMMD_COST_MMD_OPT ? 0.01f : cost_kind == MPCMMD_COST_DET ? 0.0f : 25.0f;
      p.w_des = 0.0f;
    }
    if (!queued) {
      upload_staged(h, p.idx_mpc, idx_mpc, cfg_bytes(h, p.idx_mpc, G));
      upload_staged(h, p.v_des, v_des, cfg_bytes(h, p.v_des, G));
    }
    // sampling_param (cem_helper.py:122-150): fixed key, the same draws for every configuration
    // (the internal draws depend on the seed and B only: made once per handle)
    std::vector<float> z0x;
    if (draws && draws->pop0) z0x.assign(draws->pop0, draws->pop0 + size_t(B) * 8);
    else if (h->pop0_normals.empty()) h->pop0_normals = host_normals(kFixedKey0, h->cfg.seed, kStreamPop0, 0, size_t(B) * 8);
    const std::vector<float>& z0 = draws && draws->pop0 ? z0x : h->pop0_normals;
    std::vector<double> sc(size_t(G) * 4 * kNvar);
    std::vector<float> st0(size_t(G) * 8), ob(size_t(G) * 2 * O * H), pop(size_t(G) * B * 8);
    const bool det = cost_kind == MPCMMD_COST_DET;  // the det projection's own KKT
    // the world route: st0, pop and mean are on the device; the resident route: solve_c and obs too
    const bool chained = (tick && tick->chained) || resident;
    const double* pkx = det ? h->det_kx.data() : h->pc.proj_kinv_x.data();
    const double* pky = det ? h->det_ky.data() : h->pc.proj_kinv_y.data();
    CarlaBatch cb;  // CARLA: the noisy initial rows, path and det track images of every configuration
    if (tick) {  // the same init_eps streams; the rows, boundary vectors and images are made on the device
      const int R = cost_kind == MPCMMD_COST_MMD_OPT ? h->M : det ? 1 : h->S;
      std::vector<std::vector<float>> own(G);
      std::vector<const float*> eps(G);
      for (int g = 0; g < G; ++g) {
        own[g] = host_normals(uint32_t(idx_mpc[g]), h->cfg.seed, kStreamInitEps, 0, size_t(R) * 4);
        eps[g] = own[g].data();
      }
      tick->enqueue(tick->ctx, G, cost_kind, R, eps.data());
    } else if (h->carla) {
      // compute_noisy_init_state / _baseline / _det (cem_helper.py:661-715): n^2, n or 1 rows,
      // configuration g's normals from the stream keyed by idx_mpc[g]
      const int R = cost_kind == MPCMMD_COST_MMD_OPT ? h->M : det ? 1 : h->S;
      std::vector<std::vector<float>> own(G);
      std::vector<const float*> eps(G);
      std::vector<PathView> views(G);
      for (int g = 0; g < G; ++g) {
        views[g] = view_of(path[g]);
        eps[g] = draws ? draws->init_eps : nullptr;  // external draws: G == 1
        if (!eps[g]) {
          own[g] = host_normals(uint32_t(idx_mpc[g]), h->cfg.seed, kStreamInitEps, 0, size_t(R) * 4);
          eps[g] = own[g].data();
        }
      }
      cb = carla_batch(h->pc, G, R, h->R0, O, det, init_state, views.data(), eps.data(), x_obs, y_obs);
    }
    for (int g = 0; g < G && !resident; ++g) {
      const float* is = init_state + size_t(g) * 6;
      // boundary vectors (cem_helper.py:152-167) and the per-solve KKT columns
      double bx[3] = {is[0], is[2], is[4]};
      double by[4] = {is[1], is[3], is[5], 0.0};
      if (h->carla && !tick) {  // from the mean of the noisy rows' Frenet states (carla_rows)
        std::memcpy(bx, &cb.bx[size_t(g) * 3], sizeof bx);
        std::memcpy(by, &cb.by[size_t(g) * 4], sizeof by);
      }
      initial_state(is, st0.data() + size_t(g) * 8);
      if (!tick) {  // the tick route: solve_c and obs are k_tick_setup's
        solve_columns(h->pc, pkx, pky, bx, by, sc.data() + size_t(g) * 4 * kNvar);
        obstacle_transpose(x_obs + size_t(g) * O * kNum, y_obs + size_t(g) * O * kNum, O, H,
                           ob.data() + size_t(g) * 2 * O * H);
      }
      if (!chained)
        initial_population(mean + size_t(g) * 8, cov + size_t(g) * 64, z0.data(), B, pop.data() + size_t(g) * B * 8);
    }
    if (!tick && !resident) upload_staged(h, p.solve_c, sc.data(), sc.size() * 8);
    if (h->carla) {
      // one staged copy per buffer whatever G is (the staging area holds each staged buffer once)
      // (the tick route: k_tick_path and k_tick_setup write the three buffers)
      for (const CarlaBatch::Piece& piece : cb.staged()) {
        if (tick) break;
        const std::string name(piece.buffer);
        const void* dst = name == "st0r" ? static_cast<const void*>(p.st0r)
                          : name == "path" ? static_cast<const void*>(p.path)
                                           : static_cast<const void*>(p.obs_full);
        upload_staged(h, dst, piece.image->data(), piece.image->size() * 4);
      }
      p.P = tick ? tick->num_path : path[0].num_path;
      if (cost_kind == MPCMMD_COST_DET) {  // the risks stay 0 (no risk stage)
        HIPC(hipMemsetAsync(p.obs_cost, 0, size_t(G) * B * 4, h->stream));
        HIPC(hipMemsetAsync(p.lane_cost, 0, size_t(G) * B * 4, h->stream));
        HIPC(hipMemsetAsync(p.lane_des, 0, size_t(G) * B * 4, h->stream));
      }
    }
    if (!chained) upload_staged(h, p.st0, st0.data(), st0.size() * 4);
    if (!tick && !resident) upload_staged(h, p.obs, ob.data(), ob.size() * 4);
    if (!chained) {
      upload_staged(h, p.pop, pop.data(), pop.size() * 4);  // iteration 0's half: [0][G B][8]
      upload_staged(h, p.mean, mean, cfg_bytes(h, p.mean, G));
    }
    upload_staged(h, p.cov, cov, cfg_bytes(h, p.cov, G));
    HIPC(hipMemsetAsync(p.lam_x, 0, cfg_bytes(h, p.lam_x, G), h->stream));
    HIPC(hipMemsetAsync(p.lam_y, 0, cfg_bytes(h, p.lam_y, G), h->stream));
    HIPC(hipMemsetAsync(p.s_lane, 0, cfg_bytes(h, p.s_lane, G), h->stream));
    // external noise rows: [T][3][S][H] -> device [T][3][H][S]
    h->ext_roll = draws && draws->roll;
    h->ext_res = draws && draws->resample;
    if (h->ext_roll) {
      const std::vector<float> r = roll_transpose(draws->roll, T, S, H);
      upload_staged(h, p.roll, r.data(), r.size() * 4);
    }
    if (h->ext_res) upload_staged(h, p.resample, draws->resample, cfg_bytes(h, p.resample, 1));
    if (cost_kind == MPCMMD_COST_MMD_OPT) {
      const size_t M1 = size_t(h->M) + 1;
      const bool ext_b = draws && (draws->beta_z0 || draws->beta_z);
      if (ext_b) {
        if (!draws->beta_z0 || !draws->beta_z) throw std::invalid_argument("beta_z0 and beta_z go together");
        upload(h, h->p.beta_z0, draws->beta_z0, size_t(kBetaSamples) * M1 * 4);
        for (int t = 0; t < kBetaIters; ++t)
          upload_beta_z(h, t, draws->beta_z + size_t(t) * (kBetaSamples - kBetaElite) * M1);
        h->beta_tables_internal = false;
        h->sel0_valid = false;
      } else if (!h->beta_tables_internal) {
        gen_beta_tables(h);
      }
    }
    HIPC(hipEventRecord(h->stage_ev, h->stream));
    h->stage_pending = true;
    drain.armed = false;
    h->begun = true;
    h->last_t = -1;
    h->ahead_t = -1;
    h->prep_t = -1;
    return MPCMMD_OK;
  });
}

namespace {

// the result of configuration g (cem.py:324-333): the last enqueued iteration
void read_result(mpcmmd_handle* h, int g, mpcmmd_result* out) {
  const int T = h->T;
  std::vector<float> r(kResultStride);
  HIPC(hipMemcpy(r.data(), h->p.results + (size_t(g) * T + h->last_t) * kResultStride, kResultStride * 4,
                 hipMemcpyDeviceToHost));
  std::memcpy(out->cx, &r[0], 11 * 4);
  std::memcpy(out->cy, &r[11], 11 * 4);
  out->cost_lane = r[22];
  out->cost_obs = r[23];
  out->sigma = r[24];
  std::memcpy(out->res_beta, &r[25], 20 * 4);
  if (out->beta && h->cost == MPCMMD_COST_MMD_OPT) std::memcpy(out->beta, &r[45], size_t(h->n) * 4);
  if (h->carla) {  // carla/optimizer/cem.py:413-441: cx, cy, v_best, steering_best, mean_param
    std::vector<float> st(kNum);
    HIPC(hipMemcpy(st.data(), h->p.res_steer + (size_t(g) * T + h->last_t) * kNum, kNum * 4, hipMemcpyDeviceToHost));
    if (out->steering) std::memcpy(out->steering, st.data(), kNum * 4);
    HIPC(hipMemcpy(out->mean_param, h->p.mean + size_t(g) * 8, 8 * 4, hipMemcpyDeviceToHost));
    if (out->v_best) plan_speed(h->pc, out->cx, out->cy, out->v_best);
  }
  const int Tr = h->last_t + 1;
  if (out->elite_proj)
    HIPC(hipMemcpy(out->elite_proj, h->p.tr_proj + size_t(g) * T * h->B, size_t(Tr) * h->B * 4,
                   hipMemcpyDeviceToHost));
  if (out->elite_obs)
    HIPC(hipMemcpy(out->elite_obs, h->p.tr_obs + size_t(g) * T * kEliteCost, size_t(Tr) * kEliteCost * 4,
                   hipMemcpyDeviceToHost));
  if (out->elite_cem)
    HIPC(hipMemcpy(out->elite_cem, h->p.tr_cem + size_t(g) * T * kElite, size_t(Tr) * kElite * 4,
                   hipMemcpyDeviceToHost));
}

}  // namespace

extern "C" {

int mpcmmd_begin(mpcmmd_handle* h, int32_t cost_kind, int32_t idx_mpc, const float init_state[6],
                 const float mean[8], const float cov[64], const float* x_obs, const float* y_obs, float v_des,
                 const mpcmmd_draws* draws) {
  return begin_impl(h, 1, cost_kind, &idx_mpc, init_state, mean, cov, x_obs, y_obs, &v_des, draws);
}

int mpcmmd_begin_batch(mpcmmd_handle* h, int32_t n_cfg, int32_t cost_kind, const int32_t* idx_mpc,
                       const float* init_state, const float* mean, const float* cov, const float* x_obs,
                       const float* y_obs, const float* v_des) {
  return begin_impl(h, n_cfg, cost_kind, idx_mpc, init_state, mean, cov, x_obs, y_obs, v_des, nullptr);
}

int mpcmmd_finish(mpcmmd_handle* h, mpcmmd_result* out) { return mpcmmd_finish_batch(h, 1, out); }

int mpcmmd_finish_batch(mpcmmd_handle* h, int32_t n_cfg, mpcmmd_result* out) {
  if (!h || !out) return fail(MPCMMD_E_INVALID, "null argument");
  if (!h->begun || h->last_t < 0) return fail(MPCMMD_E_STATE, "no iteration has run");
  if (n_cfg < 1 || n_cfg > h->G) return fail(MPCMMD_E_INVALID, "n_cfg exceeds the configurations of the solve");
  return guarded([&] {
    check_device(h);
    HIPC(hipStreamSynchronize(h->stream));
    if (h->prof) h->collect();
    for (int g = 0; g < n_cfg; ++g) read_result(h, g, out + g);
    return MPCMMD_OK;
  });
}

int mpcmmd_solve(mpcmmd_handle* h, int32_t cost_kind, int32_t idx_mpc, const float init_state[6],
                 const float mean[8], const float cov[64], const float* x_obs, const float* y_obs, float v_des,
                 const mpcmmd_draws* draws, mpcmmd_result* out) {
  int rc = mpcmmd_begin(h, cost_kind, idx_mpc, init_state, mean, cov, x_obs, y_obs, v_des, draws);
  if (rc) return rc;
  rc = mpcmmd_iterate(h, 0, h->T);
  if (rc) return rc;
  return mpcmmd_finish(h, out);
}

int mpcmmd_solve_batch(mpcmmd_handle* h, int32_t n_cfg, int32_t cost_kind, const int32_t* idx_mpc,
                       const float* init_state, const float* mean, const float* cov, const float* x_obs,
                       const float* y_obs, const float* v_des, mpcmmd_result* out) {
  int rc = mpcmmd_begin_batch(h, n_cfg, cost_kind, idx_mpc, init_state, mean, cov, x_obs, y_obs, v_des);
  if (rc) return rc;
  rc = mpcmmd_iterate(h, 0, h->T);
  if (rc) return rc;
  return mpcmmd_finish_batch(h, n_cfg, out);
}

int mpcmmd_carla_begin(mpcmmd_handle* h, int32_t cost_kind, int32_t idx_mpc, const float init_state[6],
                       const float mean[8], const float cov[64], const float* x_obs, const float* y_obs, float v_des,
                       const mpcmmd_path* path, const mpcmmd_draws* draws) {
  if (!path) return fail(MPCMMD_E_INVALID, "null path");
  return begin_impl(h, 1, cost_kind, &idx_mpc, init_state, mean, cov, x_obs, y_obs, &v_des, draws, path);
}

int mpcmmd_carla_begin_batch(mpcmmd_handle* h, int32_t n_cfg, int32_t cost_kind, const int32_t* idx_mpc,
                             const float* init_state, const float* mean, const float* cov, const float* x_obs,
                             const float* y_obs, const float* v_des, const mpcmmd_path* paths) {
  if (!paths) return fail(MPCMMD_E_INVALID, "null argument");
  return begin_impl(h, n_cfg, cost_kind, idx_mpc, init_state, mean, cov, x_obs, y_obs, v_des, nullptr, paths);
}

int mpcmmd_carla_solve_batch(mpcmmd_handle* h, int32_t n_cfg, int32_t cost_kind, const int32_t* idx_mpc,
                             const float* init_state, const float* mean, const float* cov, const float* x_obs,
                             const float* y_obs, const float* v_des, const mpcmmd_path* paths, mpcmmd_result* out) {
  if (!out) return fail(MPCMMD_E_INVALID, "null argument");
  int rc = mpcmmd_carla_begin_batch(h, n_cfg, cost_kind, idx_mpc, init_state, mean, cov, x_obs, y_obs, v_des, paths);
  if (rc) return rc;
  rc = mpcmmd_iterate(h, 0, h->T);
  if (rc) return rc;
  return mpcmmd_finish_batch(h, n_cfg, out);
}

int mpcmmd_carla_solve(mpcmmd_handle* h, int32_t cost_kind, int32_t idx_mpc, const float init_state[6],
                       const float mean[8], const float cov[64], const float* x_obs, const float* y_obs, float v_des,
                       const mpcmmd_path* path, const mpcmmd_draws* draws, mpcmmd_result* out) {
  int rc = mpcmmd_carla_begin(h, cost_kind, idx_mpc, init_state, mean, cov, x_obs, y_obs, v_des, path, draws);
  if (rc) return rc;
  rc = mpcmmd_iterate(h, 0, h->T);
  if (rc) return rc;
  return mpcmmd_finish(h, out);
}

}  // extern "C"
