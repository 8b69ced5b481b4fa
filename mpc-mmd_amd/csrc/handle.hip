// libmpcmmd: the handle's lifetime (mpcmmd_create_batch allocates every
// device buffer of buffers.hpp's list; no allocation after it), the
// environment knobs, streams, and the debug / profiling API.  Host code is
// plain HIP runtime; no torch.
#include <climits>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <stdexcept>
#include <string>
#include <vector>

#include "handle.hpp"
#include "rng.hpp"
#include "solve_host.hpp"

using namespace mpcmmd;

void mpcmmd::upload(mpcmmd_handle* h, const void* dst, const void* src, size_t bytes, size_t offset) {
  const mpcmmd_handle::Buf& b = h->buf_of(dst);
  if (offset + bytes > b.bytes) throw std::runtime_error(std::string("buffer ") + b.name);
  HIPC(hipMemcpyAsync(static_cast<char*>(b.ptr) + offset, src, bytes, hipMemcpyHostToDevice, h->stream));
}

namespace {

// knobs of mpcmmd_create_batch from the environment: dflt when unset
int env_int(const char* name, int dflt) {
  const char* g = std::getenv(name);
  return g ? std::atoi(g) : dflt;
}
bool env_flag(const char* name, bool dflt) { return env_int(name, dflt) != 0; }
int env_clamped(const char* name, int dflt, int lo, int hi) { return std::max(lo, std::min(hi, env_int(name, dflt))); }

const char* const kKernelNames[kNumKernels] = {
#define X(id, name) name,
    MPCMMD_KERNELS(X)
#undef X
};

// the buffer of that name (the by-name debug API), or null
const mpcmmd_handle::Buf* find_buf(const mpcmmd_handle* h, const char* name) {
  for (const mpcmmd_handle::Buf& b : h->bufs)
    if (std::strcmp(b.name, name) == 0) return &b;
  return nullptr;
}

// a packed constant against its element count in buffers.hpp's list
template <class V>
void upload_packed(mpcmmd_handle* h, const void* dst, const V& v) {
  if (v.size() * sizeof(v[0]) != h->buf_of(dst).bytes)
    throw std::logic_error(std::string("packed constant size: ") + h->buf_of(dst).name);
  upload(h, dst, v.data(), v.size() * sizeof(v[0]));
}

}  // namespace

extern "C" {

int32_t mpcmmd_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int mpcmmd_create(const mpcmmd_config* cfg, mpcmmd_handle** out) { return mpcmmd_create_batch(cfg, 1, out); }

int mpcmmd_create_batch(const mpcmmd_config* cfg, int32_t max_configs, mpcmmd_handle** out) {
  if (!cfg || !out) return fail(MPCMMD_E_INVALID, "null argument");
  *out = nullptr;
  const mpcmmd_config& c = *cfg;
  if (int rc = check_create_ranges(c, max_configs)) return rc;
  auto* h = new mpcmmd_handle();
  int rc = guarded([&] {
    h->cfg = c;
    h->device = c.device;
    if (const char* cap = std::getenv("MPCMMD_MAX_HANDLE_BYTES")) h->alloc_cap = size_t(std::strtoull(cap, nullptr, 10));
    int ndev = 0;
    HIPC(hipGetDeviceCount(&ndev));
    if (c.device < 0 || c.device >= ndev) throw std::invalid_argument("device ordinal out of range");
    HIPC(hipSetDevice(c.device));
    // the baseline risk stage keeps 4 O H + 2 H + 3 S floats and S sort pairs in LDS: a
    // shape the device cannot launch is refused here, not at the first risk stage
    // (never on an MI355X: the largest accepted shape needs 150 KiB of its 160)
    if (c.variant == MPCMMD_VARIANT_STATIC || c.variant == MPCMMD_VARIANT_DYNAMIC) {  // CARLA: its own risk kernels
      int lds_max = 0;
      HIPC(hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, c.device));
      const size_t need = risk_lds_bytes(c.num_obs, c.num_prime, c.num_reduced);
      if (need > size_t(lds_max))
        return fail(MPCMMD_E_UNSUPPORTED, "the risk stage's workgroup needs " + std::to_string(need) +
                                              " B of LDS, the device has " + std::to_string(lds_max));
    }
    HIPC(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    h->own_stream = true;
    h->pc = build_constants(c.num_prime, c.variant);
    h->B = c.num_batch;
    h->S = c.num_reduced;
    h->H = c.num_prime;
    h->O = c.num_obs;
    h->n = c.num_reduced;
    h->M = c.num_reduced * c.num_reduced;
    h->T = c.maxiter_cem;
    h->Gmax = max_configs;
    h->G = 1;
    const int B = h->B, S = h->S, H = h->H, O = h->O, T = h->T;
    const size_t BT = size_t(max_configs) * B;  // candidate capacity
    if (gtab_stride(S, H) != gamma_tab_size(S, H)) throw std::logic_error("Beta attempt table stride");
    const bool mmd_ok = mmdopt_supported(h->n, h->H, h->O, &h->mmd_why);
    h->mmd_ok = mmd_ok;
    Params& p = h->p;
    p.B = B;
    p.S = S;
    p.H = H;
    p.O = O;
    p.n = h->n;
    p.M = h->M;
    p.T = T;
    p.noise = c.noise;
    p.seed = c.seed;
    p.G = 1;
    p.Bt = B;
    p.b0 = 0;
    p.nb = B;
    p.sigma_acc = c.noise_level;
    p.sigma_steer = c.noise_level;
    p.acc_const = c.acc_const_noise;
    p.steer_const = c.steer_const_noise;
    // beta noise: steer_pert = float32(K_steer * sigma_steer) * (2 b - 1) (cem_helper.py:436)
    p.K_steer = float(h->pc.K_steer * double(c.noise_level));
    p.y_lb = float(h->pc.y_lb);
    p.y_ub = float(h->pc.y_ub);
    h->carla = h->pc.carla;
    p.carla = h->carla ? 1 : 0;
    p.wheel_base = float(h->pc.wheel_base);
    p.obs_a2 = float(h->pc.a_obs * h->pc.a_obs);
    p.obs_b2 = float(h->pc.b_obs * h->pc.b_obs);
    p.obs_a = float(h->pc.a_obs);
    p.obs_b = float(h->pc.b_obs);
    p.a_centr = float(h->pc.a_centr);
    p.y_des1 = float(h->pc.y_des_1);
    p.y_des2 = float(h->pc.y_des_2);
    p.gamma_des = float(h->pc.gamma_lane_des);
    if (h->carla) {
      h->R0 = mmd_ok ? std::max(h->M, S) : S;
      p.R0 = h->R0;
      // compute_cem_det's projection (projection_det.py:149-160): its own KKT
      det_projection_kinv(h->pc, O, h->det_kx, h->det_ky);
    }
    // every device buffer (buffers.hpp), zeroed; its Params member is its name.  dbgw (per-workgroup
    // phase stamps, tools/stampsw.py) only when asked for: with dbgw null MPCMMD_STAMPW writes nothing
    const BufferShape shape{B, S, H, O, h->n, h->M, T, max_configs, h->R0, c.noise == MPCMMD_NOISE_BETA,
                            mmd_ok, h->carla, std::getenv("MPCMMD_STAMPW") != nullptr};
    const std::vector<BufferSpec> specs = buffer_specs(shape);
    size_t spec = 0;
#define X(name, type, count, exists, staged) p.name = static_cast<type*>(h->alloc(specs[spec++]));
    MPCMMD_BUFFERS(X)
#undef X
    // the +inf pad columns of bdist, once per handle and for the whole capacity
    // (later solves may hold more candidates); here, after the buffer's clear on
    // the same stream, so the launch can never land inside a graph capture
    if (mmd_ok) {
      launch_dist_pad(p, int(BT), h->stream);
      HIPC(hipGetLastError());
    }
    // two candidate groups on two streams once each group still fills the
    // chip: one group's MFMA-bound sampler overlaps the other's VALU-bound
    // kernel sums (B = 1024: 82.2 -> 92.8 steps/s; four groups: 72.6)
    if (BT >= 1024) h->groups = 2;
    // small batches on the per-iteration kernels (num_reduced > 16; CARLA n = 22 at
    // B = 100): two groups as well, for launches of 64..256 candidates
    const int kMaxG = mpcmmd_handle::kMaxGroups, kNoMax = INT_MAX;
    h->small_groups = env_clamped("MPCMMD_SMALL_GROUPS", h->small_groups, 1, kMaxG);
    if (BT >= 64 && BT <= 256) h->groups = std::max(h->groups, h->small_groups);
    h->groups_forced = std::getenv("MPCMMD_GROUPS") != nullptr;
    h->graphs = env_flag("MPCMMD_GRAPH", h->graphs);
    h->ahead_on = env_flag("MPCMMD_AHEAD", h->ahead_on);
    h->fused_small = env_flag("MPCMMD_FUSED", h->fused_small);
    h->prep_on = env_flag("MPCMMD_SELECT_PREP", h->prep_on);
    // the generators' variant is a property of the handle (its capacity), not
    // of a launch's candidate group: a candidate's bits do not depend on how
    // the batch is split into groups or whether k_bcem_small runs it
    p.gen_wave = env_flag("MPCMMD_GENWAVE", BT <= 512 && h->n <= 24);
    p.mom_rows = env_flag("MPCMMD_MOM_ROWS", true);
    p.mom_amax = 1.0;  // == kSeriesAMax
    if (const char* g = std::getenv("MPCMMD_MOM_AMAX")) p.mom_amax = std::atof(g);
    p.dir_pairs = env_flag("MPCMMD_DIR_PAIRS", true);
    p.qp_small = env_flag("MPCMMD_QP_SMALL", true);
    p.sel_cap = env_clamped("MPCMMD_SEL_CAP", 64, 1, kNoMax);
    // parts per candidate only below 128 candidates per launch (B = 100: 8 -> 2 parts)
    p.ker_target = env_clamped("MPCMMD_KER_TARGET", 128, 1, kNoMax);
    p.dir_target = env_clamped("MPCMMD_DIR_TARGET", 2048, 1, kNoMax);
    p.ker_path = env_clamped("MPCMMD_KER_PATH", 0, 0, 2);
    p.beta_dump = env_flag("MPCMMD_BETA_DUMP", p.beta_dump != 0);
    h->groups = env_clamped("MPCMMD_GROUPS", h->groups, 1, kMaxG);
    if (h->groups > 1) {
      HIPC(hipEventCreateWithFlags(&h->gev_start, hipEventDisableTiming));
      for (int g = 0; g < h->groups; ++g) {
        HIPC(hipStreamCreateWithFlags(&h->gstream[g], hipStreamNonBlocking));
        HIPC(hipEventCreateWithFlags(&h->gev_done[g], hipEventDisableTiming));
      }
    }
    h->stage_bytes = staging_bytes(specs);
    HIPC(hipHostMalloc(reinterpret_cast<void**>(&h->stage), h->stage_bytes, hipHostMallocDefault));
    HIPC(hipEventCreateWithFlags(&h->stage_ev, hipEventDisableTiming));
    // the packed constants; the copies are asynchronous, so the vectors live until the synchronize below
    const std::vector<float> basis = pack_basis(h->pc);
    const std::vector<double> gg = pack_guess_g(h->pc), pm = pack_proj_m(h->pc.proj_kinv_x, h->pc.proj_kinv_y);
    const std::vector<double> pm_det = h->carla ? pack_proj_m(h->det_kx, h->det_ky) : std::vector<double>();
    upload_packed(h, p.basis, basis);
    upload_packed(h, p.guess_g, gg);
    upload_packed(h, p.proj_m, pm);
    upload_packed(h, p.fit, h->pc.fit);
    if (h->carla) upload_packed(h, p.proj_m_det, pm_det);
    HIPC(hipStreamSynchronize(h->stream));
    return MPCMMD_OK;
  });
  if (rc != MPCMMD_OK) {
    mpcmmd_destroy(h);
    // a failed hipMalloc leaves its error as the runtime's last error; clear
    // it so a retry in this process (optimizer/sweep.py: batch_handle halves
    // max_configs) does not see the stale code at its first launch check
    (void)hipGetLastError();
    return rc;
  }
  *out = h;
  return MPCMMD_OK;
}

void mpcmmd_destroy(mpcmmd_handle* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  for (auto& kv : h->gexec) {
    (void)hipGraphExecDestroy(kv.second.second);
    (void)hipGraphDestroy(kv.second.first);
  }
  for (int g = 0; g < mpcmmd_handle::kMaxGroups; ++g)  // group streams drained before their buffers go
    if (h->gstream[g]) (void)hipStreamSynchronize(h->gstream[g]);
  for (auto& b : h->bufs) (void)hipFree(b.ptr);
  for (auto& pe : h->pending) {
    (void)hipEventDestroy(pe.second.first);
    (void)hipEventDestroy(pe.second.second);
  }
  for (auto e : h->free_events) (void)hipEventDestroy(e);
  if (h->stage_ev) (void)hipEventDestroy(h->stage_ev);
  for (int g = 0; g < mpcmmd_handle::kMaxGroups; ++g) {
    if (h->gstream[g]) (void)hipStreamSynchronize(h->gstream[g]);
    if (h->gstream[g]) (void)hipStreamDestroy(h->gstream[g]);
    if (h->gev_done[g]) (void)hipEventDestroy(h->gev_done[g]);
  }
  if (h->gev_start) (void)hipEventDestroy(h->gev_start);
  if (h->stage) (void)hipHostFree(h->stage);
  if (h->own_stream && h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
}

int mpcmmd_set_stream(mpcmmd_handle* h, void* s) {
  if (!h) return fail(MPCMMD_E_INVALID, "null handle");
  return guarded([&] {
    check_device(h);
    HIPC(hipStreamSynchronize(h->stream));
    if (h->own_stream) HIPC(hipStreamDestroy(h->stream));
    h->own_stream = false;
    h->stream = static_cast<hipStream_t>(s);
    return MPCMMD_OK;
  });
}

void* mpcmmd_get_stream(mpcmmd_handle* h) { return h ? (void*)h->stream : nullptr; }

int32_t mpcmmd_max_configs(mpcmmd_handle* h) { return h ? h->Gmax : 0; }

int mpcmmd_handle_info(mpcmmd_handle* h, const char* name, int64_t* value) {
  if (!h || !name || !value) return fail(MPCMMD_E_INVALID, "null argument");
  const std::string k(name);
  if (k == "gen_wave") *value = h->p.gen_wave ? 1 : 0;
  else if (k == "select_prep") *value = h->prep_on && !h->carla ? 1 : 0;
  else if (k == "fused_small") *value = h->fused_small ? 1 : 0;
  else if (k == "groups") *value = h->groups;
  else if (k == "ker_path") *value = h->p.ker_path;
  else if (k == "capacity") *value = int64_t(h->Gmax) * h->B;
  else return fail(MPCMMD_E_INVALID, "unknown handle_info name " + k);
  return MPCMMD_OK;
}

int mpcmmd_profile(mpcmmd_handle* h, int32_t enable) {
  if (!h) return fail(MPCMMD_E_INVALID, "null handle");
  return guarded([&] {
    check_device(h);
    HIPC(hipStreamSynchronize(h->stream));
    h->collect();
    h->prof = enable != 0;
    for (int k = 0; k < kNumKernels; ++k) {
      h->launches[k] = 0;
      h->total_ms[k] = 0.0;
    }
    return MPCMMD_OK;
  });
}

int mpcmmd_kernel_times(mpcmmd_handle* h, int32_t* launches, double* total_ms, int32_t max_kernels) {
  if (!h) return fail(MPCMMD_E_INVALID, "null handle");
  return guarded([&] {
    check_device(h);
    h->collect();
    for (int k = 0; k < kNumKernels && k < max_kernels; ++k) {
      if (launches) launches[k] = h->launches[k];
      if (total_ms) total_ms[k] = h->total_ms[k];
    }
    return int(kNumKernels);
  });
}

const char* mpcmmd_kernel_name(int32_t id) {
  return (id >= 0 && id < kNumKernels) ? kKernelNames[id] : nullptr;
}

int mpcmmd_buffer_info(mpcmmd_handle* h, const char* name, size_t* bytes) {
  if (!h || !name) return fail(MPCMMD_E_INVALID, "null argument");
  if (std::string(name) == "*") {  // every device buffer of the handle
    size_t tot = 0;
    for (auto& b : h->bufs) tot += b.bytes;
    if (bytes) *bytes = tot;
    return MPCMMD_OK;
  }
  const auto* it = find_buf(h, name);
  if (!it) return fail(MPCMMD_E_INVALID, std::string("no buffer ") + name);
  if (bytes) *bytes = it->bytes;
  return MPCMMD_OK;
}

int mpcmmd_read(mpcmmd_handle* h, const char* name, void* dst, size_t bytes) {
  if (!h || !name || !dst) return fail(MPCMMD_E_INVALID, "null argument");
  const auto* it = find_buf(h, name);
  if (!it) return fail(MPCMMD_E_INVALID, std::string("no buffer ") + name);
  if (bytes > it->bytes) return fail(MPCMMD_E_INVALID, "read larger than buffer");
  return guarded([&] {
    check_device(h);
    HIPC(hipStreamSynchronize(h->stream));
    HIPC(hipMemcpy(dst, it->ptr, bytes, hipMemcpyDeviceToHost));
    return MPCMMD_OK;
  });
}

int mpcmmd_write(mpcmmd_handle* h, const char* name, const void* src, size_t bytes) {
  if (!h || !name || !src) return fail(MPCMMD_E_INVALID, "null argument");
  const auto* it = find_buf(h, name);
  if (!it) return fail(MPCMMD_E_INVALID, std::string("no buffer ") + name);
  if (bytes > it->bytes) return fail(MPCMMD_E_INVALID, "write larger than buffer");
  return guarded([&] {
    check_device(h);
    HIPC(hipStreamSynchronize(h->stream));
    HIPC(hipMemcpy(it->ptr, src, bytes, hipMemcpyHostToDevice));
    if (std::string(name) == "beta_z0" || std::string(name) == "beta_z") h->beta_tables_internal = false;
    if (std::string(name) == "beta_z0") h->sel0_valid = false;
    return MPCMMD_OK;
  });
}

}  // extern "C"
