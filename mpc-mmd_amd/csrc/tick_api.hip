// libmpcmmd: the CARLA tick route (include/mpcmmd.h): the tick context with
// its own device and pinned memory, and the begin that hands the per-tick
// arithmetic to k_tick.hip.  Everything else of the begin is begin.hip's
// begin_impl, shared with the host route.
#include <cmath>
#include <cstring>
#include <vector>

#include "handle.hpp"
#include "tick.hpp"

using namespace mpcmmd;

struct mpcmmd_tick {
  mpcmmd_handle* h = nullptr;
  int P = 0;
  TickLayout lay{};
  // device memory of the context (none of it in the handle's buffer list)
  double* inv = nullptr;   // (P + 1)^2 smoothing inverse, column-major
  double* kcol = nullptr;  // [2][4][11][4]: the KKT coefficient columns, then those of the det projection
  float* in = nullptr;     // [Gmax][lay.stride] tick inputs
  float* fr = nullptr;     // [Gmax][R0][6] Frenet states of the noisy rows
  // pinned staging of the inputs: refilled only after ev, recorded behind the previous copy
  float* stage = nullptr;
  hipEvent_t ev = nullptr;
  bool pending = false;
  const mpcmmd_tick_inputs* cur = nullptr;  // the inputs of the begin in progress
  float chained_threshold = 0.0f;           // that of the chained begin in progress
};

namespace {

// guess_kinv_x/y, proj_kinv_x/y columns 11.. of rows 0..10, as solve_columns reads them: [4][11][4]
std::vector<double> kkt_columns(const ProblemConsts& pc, const double* pkx, const double* pky) {
  std::vector<double> out(size_t(4) * kNvar * 4, 0.0);
  for (int k = 0; k < kNvar; ++k) {
    for (int e = 0; e < 3; ++e) out[(0 * kNvar + k) * 4 + e] = pc.guess_kinv_x[k * 14 + kNvar + e];
    for (int e = 0; e < 4; ++e) out[(1 * kNvar + k) * 4 + e] = pc.guess_kinv_y[k * 15 + kNvar + e];
    for (int e = 0; e < 3; ++e) out[(2 * kNvar + k) * 4 + e] = pkx[k * 14 + kNvar + e];
    for (int e = 0; e < 4; ++e) out[(3 * kNvar + k) * 4 + e] = pky[k * 15 + kNvar + e];
  }
  return out;
}

// the two kernels of a begin on inputs that are in t->in
void launch_kernels(mpcmmd_tick* t, int G, int cost_kind, int R, float threshold) {
  mpcmmd_handle* h = t->h;
  const bool det = cost_kind == MPCMMD_COST_DET;
  TickParams q{};
  q.G = G, q.P = t->P, q.O = h->O, q.H = h->H, q.R = R, q.R0 = h->R0, q.det = det ? 1 : 0;
  q.thr = threshold;
  q.lay = t->lay;
  q.mu_x = float(h->pc.init_mu_x), q.mu_y = float(h->pc.init_mu_y);
  q.sg_x = float(h->pc.init_sigma_x), q.sg_y = float(h->pc.init_sigma_y);
  q.inv = t->inv;
  q.kcol = t->kcol + (det ? size_t(4) * kNvar * 4 : 0);
  q.in = t->in;
  q.fr = t->fr;
  // the kernels write the handle's buffers (Params holds them as inputs of the solve)
  auto out = [&](const void* member) { return h->buf_of(member).ptr; };
  q.path = static_cast<float*>(out(h->p.path)), q.st0r = static_cast<float*>(out(h->p.st0r));
  q.obs = static_cast<float*>(out(h->p.obs)), q.obs_full = static_cast<float*>(out(h->p.obs_full));
  q.solve_c = static_cast<double*>(out(h->p.solve_c));
  h->launch(kKTickPath, [&] { launch_tick_path(q, h->stream); });
  h->launch(kKTickSetup, [&] { launch_tick_setup(q, h->stream); });
}

// begin_impl's callback: stage and upload the raw inputs of G ticks, then the two kernels
void enqueue(void* ctx, int G, int cost_kind, int R, const float* const* eps) {
  mpcmmd_tick* t = static_cast<mpcmmd_tick*>(ctx);
  mpcmmd_handle* h = t->h;
  const mpcmmd_tick_inputs& in = *t->cur;
  const int P = t->P, O = h->O;
  if (t->pending) HIPC(hipEventSynchronize(t->ev));  // the previous begin's copy out of the staging
  t->pending = false;
  const TickLayout& l = t->lay;
  std::memset(t->stage, 0, size_t(G) * l.stride * 4);
  for (int g = 0; g < G; ++g) {
    float* s = t->stage + size_t(g) * l.stride;
    std::memcpy(s, in.init_state + size_t(g) * 6, 6 * 4);
    std::memcpy(s + l.xw, in.x_wp + size_t(g) * P, size_t(P) * 4);
    std::memcpy(s + l.yw, in.y_wp + size_t(g) * P, size_t(P) * 4);
    std::memcpy(s + l.obs, in.obstacles + size_t(g) * O * 5, size_t(O) * 5 * 4);
    std::memcpy(s + l.eps, eps[g], size_t(R) * 4 * 4);
  }
  HIPC(hipMemcpyAsync(t->in, t->stage, size_t(G) * l.stride * 4, hipMemcpyHostToDevice, h->stream));
  HIPC(hipEventRecord(t->ev, h->stream));
  t->pending = true;
  launch_kernels(t, G, cost_kind, R, in.threshold);
}

// the chained begin's callback (the world route): init_state, waypoints and
// obstacles are already in t->in, written by k_world_step; only the init_eps
// normals are staged, into each tick's eps slice (one strided copy)
void enqueue_chained(void* ctx, int G, int cost_kind, int R, const float* const* eps) {
  mpcmmd_tick* t = static_cast<mpcmmd_tick*>(ctx);
  mpcmmd_handle* h = t->h;
  if (t->pending) HIPC(hipEventSynchronize(t->ev));
  t->pending = false;
  const TickLayout& l = t->lay;
  const size_t width = size_t(l.stride - l.eps) * 4, pitch = size_t(l.stride) * 4;
  for (int g = 0; g < G; ++g) {
    float* s = t->stage + size_t(g) * l.stride + l.eps;
    std::memset(s, 0, width);
    std::memcpy(s, eps[g], size_t(R) * 4 * 4);
  }
  HIPC(hipMemcpy2DAsync(t->in + l.eps, pitch, t->stage + l.eps, pitch, width, size_t(G), hipMemcpyHostToDevice,
                        h->stream));
  HIPC(hipEventRecord(t->ev, h->stream));
  t->pending = true;
  launch_kernels(t, G, cost_kind, R, t->chained_threshold);
}

int check_begin(mpcmmd_tick* t, int32_t n_cfg, int32_t cost_kind, const int32_t* idx_mpc, const mpcmmd_tick_inputs* in,
                const float* mean, const float* cov, const float* v_des) {
  if (!t || !idx_mpc || !in || !mean || !cov || !v_des) return fail(MPCMMD_E_INVALID, "null argument");
  if (!in->init_state || !in->x_wp || !in->y_wp || !in->obstacles)
    return fail(MPCMMD_E_INVALID, "tick inputs: null array");
  mpcmmd_handle* h = t->h;
  if (!h->carla) return fail(MPCMMD_E_INVALID, "the tick route needs a handle of a CARLA variant");
  if (n_cfg < 1 || n_cfg > h->Gmax) return fail(MPCMMD_E_INVALID, "n_cfg must be 1..max_configs of the handle");
  if (!std::isfinite(in->threshold)) return fail(MPCMMD_E_INVALID, "tick inputs: threshold must be finite");
  if (cost_kind != MPCMMD_COST_MMD_OPT && cost_kind != MPCMMD_COST_CVAR && cost_kind != MPCMMD_COST_DET)
    return fail(MPCMMD_E_INVALID,
                "the CARLA optimizer has compute_cem_mmd (mmd_opt), compute_cem_cvar and compute_cem_det only");
  if (cost_kind == MPCMMD_COST_DET && h->O > kMaxDetObs)
    return fail(MPCMMD_E_UNSUPPORTED, "compute_cem_det: num_obs <= 32");
  if (cost_kind == MPCMMD_COST_MMD_OPT && !h->mmd_ok) return fail(MPCMMD_E_UNSUPPORTED, h->mmd_why);
  return MPCMMD_OK;
}

}  // namespace

// ---- what the world route (world_api.hip) needs of a tick context ----------------
mpcmmd_handle* mpcmmd::tick_handle(mpcmmd_tick* t) { return t->h; }
int mpcmmd::tick_num_path(const mpcmmd_tick* t) { return t->P; }
TickLayout mpcmmd::tick_layout_of(const mpcmmd_tick* t) { return t->lay; }
float* mpcmmd::tick_inputs_device(mpcmmd_tick* t) { return t->in; }

int mpcmmd::tick_begin_chained(mpcmmd_tick* t, int32_t n_cfg, int32_t cost_kind, const int32_t* idx_mpc,
                               const float* cov, const float* v_des, float threshold) {
  // init_state and mean are on the device already: begin_impl reads neither on the chained route
  const std::vector<float> zeros(size_t(n_cfg > 0 ? n_cfg : 1) * 8, 0.0f);
  mpcmmd_tick_inputs in{};
  in.init_state = in.x_wp = in.y_wp = in.obstacles = zeros.data();
  in.threshold = threshold;
  if (int rc = check_begin(t, n_cfg, cost_kind, idx_mpc, &in, zeros.data(), cov, v_des)) return rc;
  t->chained_threshold = threshold;
  TickRoute route{t->P, t, enqueue_chained};
  route.chained = true;
  return begin_impl(t->h, n_cfg, cost_kind, idx_mpc, zeros.data(), zeros.data(), cov, nullptr, nullptr, v_des, nullptr,
                    nullptr, &route);
}

extern "C" {

int mpcmmd_tick_create(mpcmmd_handle* h, int32_t num_path, mpcmmd_tick** out) {
  if (!h || !out) return fail(MPCMMD_E_INVALID, "null argument");
  *out = nullptr;
  if (num_path < 4 || num_path > kMaxPath) return fail(MPCMMD_E_INVALID, "tick: 4 <= num_path <= 2048");
  if (!h->carla) return fail(MPCMMD_E_INVALID, "the tick route needs a handle of a CARLA variant");
  auto* t = new mpcmmd_tick();
  t->h = h;
  t->P = num_path;
  t->lay = tick_layout(num_path, h->O, h->R0);
  int rc = guarded([&] {
    check_device(h);
    int lds = 0;
    HIPC(hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, h->device));
    if (size_t(lds) < tick_lds_bytes(num_path)) return fail(MPCMMD_E_UNSUPPORTED, "tick: the device's LDS is too small");
    const auto inv = smoothing_inverse_cm(num_path);
    const size_t n = size_t(num_path) + 1;
    std::vector<double> kc = kkt_columns(h->pc, h->pc.proj_kinv_x.data(), h->pc.proj_kinv_y.data());
    const std::vector<double> kd = kkt_columns(h->pc, h->det_kx.data(), h->det_ky.data());
    kc.insert(kc.end(), kd.begin(), kd.end());
    const size_t in_bytes = size_t(h->Gmax) * t->lay.stride * 4;
    HIPC(hipMalloc(reinterpret_cast<void**>(&t->inv), n * n * 8));
    HIPC(hipMalloc(reinterpret_cast<void**>(&t->kcol), kc.size() * 8));
    HIPC(hipMalloc(reinterpret_cast<void**>(&t->in), in_bytes));
    HIPC(hipMalloc(reinterpret_cast<void**>(&t->fr), size_t(h->Gmax) * h->R0 * 6 * 4 + 16));
    HIPC(hipHostMalloc(reinterpret_cast<void**>(&t->stage), in_bytes, hipHostMallocDefault));
    HIPC(hipEventCreateWithFlags(&t->ev, hipEventDisableTiming));
    HIPC(hipMemcpy(t->inv, inv->data(), n * n * 8, hipMemcpyHostToDevice));
    HIPC(hipMemcpy(t->kcol, kc.data(), kc.size() * 8, hipMemcpyHostToDevice));
    return MPCMMD_OK;
  });
  if (rc != MPCMMD_OK) {
    mpcmmd_tick_destroy(t);
    (void)hipGetLastError();
    return rc;
  }
  *out = t;
  return MPCMMD_OK;
}

void mpcmmd_tick_destroy(mpcmmd_tick* t) {
  if (!t) return;
  (void)hipSetDevice(t->h->device);
  if (t->h->stream) (void)hipStreamSynchronize(t->h->stream);  // the kernels and the copy out of the staging
  if (t->inv) (void)hipFree(t->inv);
  if (t->kcol) (void)hipFree(t->kcol);
  if (t->in) (void)hipFree(t->in);
  if (t->fr) (void)hipFree(t->fr);
  if (t->stage) (void)hipHostFree(t->stage);
  if (t->ev) (void)hipEventDestroy(t->ev);
  delete t;
}

int mpcmmd_carla_tick_begin_batch(mpcmmd_tick* t, int32_t n_cfg, int32_t cost_kind, const int32_t* idx_mpc,
                                  const mpcmmd_tick_inputs* in, const float* mean, const float* cov,
                                  const float* v_des) {
  if (int rc = check_begin(t, n_cfg, cost_kind, idx_mpc, in, mean, cov, v_des)) return rc;
  t->cur = in;
  const TickRoute route{t->P, t, enqueue};
  const int rc = begin_impl(t->h, n_cfg, cost_kind, idx_mpc, in->init_state, mean, cov, nullptr, nullptr, v_des,
                            nullptr, nullptr, &route);
  t->cur = nullptr;
  return rc;
}

int mpcmmd_carla_tick_solve_batch(mpcmmd_tick* t, int32_t n_cfg, int32_t cost_kind, const int32_t* idx_mpc,
                                  const mpcmmd_tick_inputs* in, const float* mean, const float* cov,
                                  const float* v_des, mpcmmd_result* out) {
  if (!out) return fail(MPCMMD_E_INVALID, "null argument");
  int rc = mpcmmd_carla_tick_begin_batch(t, n_cfg, cost_kind, idx_mpc, in, mean, cov, v_des);
  if (rc) return rc;
  rc = mpcmmd_iterate(t->h, 0, t->h->T);
  if (rc) return rc;
  return mpcmmd_finish_batch(t->h, n_cfg, out);
}

}  // extern "C"
