// The host layer the two episode contexts share (mpcmmd_world, world_api.hip:
// the CARLA surrogate world; mpcmmd_mpc, mpc_api.hip: the synthetic loop;
// DESIGN.md section 19): who owns the device buffers, the reset's prologue, the
// chained tick loop, the strided read-back of the logs, the validation stage's
// checks, scratch and log, and the one-launch harness of the step kernels.
// Each context keeps its kernels' parameter structs, its enqueue_step and
// enqueue_validation, and what only it has (the side stream; the LDS check).
// Internal to the library.
#pragma once
#include <array>

#include "episodes_host.hpp"
#include "handle.hpp"

#pragma GCC visibility push(hidden)
namespace mpcmmd {

static_assert(kRiskSigmaSlots == kRiskMaxSigma, "the validation structs' sigma[] is the kernels' limit");

// Device allocations that live and die together.  A context holds three: its
// own, the validation stage's and the vehicle policy's, so either stage can be
// dropped or remade whatever was allocated after it.
struct Arena : Scratch {  // which frees what is left when the context goes
  void release() {
    for (void* d : bufs) (void)hipFree(d);
    bufs.clear();
  }
  // `count` elements (room for at least 4), filled from src unless it is null: a synchronous upload
  template <class T>
  T* alloc(size_t count, const void* src = nullptr) {
    return static_cast<T*>(up(count ? src : nullptr, (count ? count : 4) * sizeof(T)));
  }
};

// an optional read-back: nothing for a null dst or no bytes
inline void back_if(void* dst, const void* src, size_t bytes) {
  if (dst && bytes) HIPC(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
}

// rows of Emax -> [ticks][E] rows of row_bytes: one strided copy (ticks, E, row_bytes > 0)
inline void rows_back(void* dst, const void* src, size_t row_bytes, int ticks, size_t E, size_t Emax) {
  HIPC(hipMemcpy2D(dst, E * row_bytes, src, Emax * row_bytes, E * row_bytes, size_t(ticks), hipMemcpyDeviceToHost));
}

// The validation log: one row per (tick, episode) of Emax, written by the validators' launches.
struct RiskLog {
  int n_counts = 0;  // count, count_lane and, with 3, count_rows
  size_t S = 0;      // bandwidths
  int32_t* count[3] = {nullptr, nullptr, nullptr};  // [rows] each
  int32_t* pos = nullptr;                           // [rows][3]
  float* stat[4] = {nullptr, nullptr, nullptr, nullptr};  // var, cvar, mean, max: [rows][3] each
  float* mmd = nullptr;                             // [rows][3][S]
  float* est = nullptr;                             // [rows][2]
  void alloc(Arena& a, size_t rows, size_t S_, int n_counts_) {
    n_counts = n_counts_, S = S_;
    for (int k = 0; k < n_counts; ++k) count[k] = a.alloc<int32_t>(rows);
    pos = a.alloc<int32_t>(rows * 3);
    for (float*& s : stat) s = a.alloc<float>(rows * 3);
    mmd = a.alloc<float>(rows * 3 * S), est = a.alloc<float>(rows * 2);
  }
  // the statistics' results of q at the log's row `row` (a tick's first: tick * Emax)
  void point(ValidateRiskParams& q, size_t row) const {
    q.count_pos = pos + row * 3;
    q.var = stat[0] + row * 3, q.cvar = stat[1] + row * 3, q.mean = stat[2] + row * 3, q.vmax = stat[3] + row * 3;
    q.mmd = S ? mmd + row * 3 * S : nullptr;
  }
  // the first `ticks` ticks: counts [ticks][E][n_counts], count_pos [..][3], stats [..][4][3], mmd [..][3][S],
  // est [..][2]
  void read(int ticks, size_t E, size_t Emax, int32_t* counts, int32_t* count_pos, float* stats, float* mmd_out,
            float* est_out) const {
    const size_t n = size_t(ticks) * E;
    std::vector<int32_t> planes(n * size_t(n_counts));
    for (int k = 0; k < n_counts; ++k) rows_back(planes.data() + size_t(k) * n, count[k], 4, ticks, E, Emax);
    std::vector<float> s4(n * 12);
    for (size_t k = 0; k < 4; ++k) rows_back(s4.data() + k * n * 3, stat[k], 12, ticks, E, Emax);
    interleave_risk_log(n, n_counts, planes.data(), s4.data(), counts, stats);
    rows_back(count_pos, pos, 12, ticks, E, Emax), rows_back(est_out, est, 8, ticks, E, Emax);
    if (S > 0) rows_back(mmd_out, mmd, 12 * S, ticks, E, Emax);
  }
};

// What the two contexts hold alike: the episodes, their variates and keys, the log, the start
// covariance's factor, and the state of the two optional stages.
struct Episodes {
  mpcmmd_handle* h = nullptr;
  int Tmax = 0, Emax = 0, E = 0;
  bool drawn = false;            // the variates are drawn in the kernel (no u given at the reset)
  std::vector<uint32_t> keys;    // [E] episode keys: idx_mpc = tick + key, and the variates' Philox key
  uint32_t* keys_dev = nullptr;  // [Emax]
  bool reset_done = false;
  Arena base, val, veh;     // the context's own allocations, the validation stage's, the vehicle policy's
  double* pos = nullptr;    // [Emax][2] the ego positions (the step kernel's q.pos)
  int32_t* done = nullptr;  // [Emax] the tick an episode ended at, or -1 (q.done)
  int wu = 0, wd = 0, wf = 0, wi = 0, wp = 0;  // row widths of u, logd, logf, logi, plan
  float* u = nullptr;       // [Tmax][Emax][wu]
  double* logd = nullptr;   // [Tmax][Emax][wd]
  float* logf = nullptr;    // [Tmax][Emax][wf]
  int32_t* logi = nullptr;  // [Tmax][Emax][wi]
  float* plan = nullptr;    // [Tmax][Emax][wp]
  double* chol = nullptr;   // [8][8]
  std::array<double, 64> chol_host{};
  bool val_on = false;      // the validation stage (off: nothing of it exists)
  ValidateRiskParams vq{};  // the statistics' scratch (the results point into the log per tick)
  RiskLog vl;
  bool veh_on = false;      // the vehicle policy (off: nothing of it exists)
  int veh_E = 0;            // the episodes the staged arrays are for

  // u, the keys and the four log arrays, of the given row widths
  void alloc_rows(int wu_, int wd_, int wf_, int wi_, int wp_) {
    wu = wu_, wd = wd_, wf = wf_, wi = wi_, wp = wp_;
    const size_t Em = size_t(Emax), rows = size_t(Tmax) * Em;
    u = base.alloc<float>(rows * wu);
    keys_dev = base.alloc<uint32_t>(Em);
    logd = base.alloc<double>(rows * wd), logf = base.alloc<float>(rows * wf);
    logi = base.alloc<int32_t>(rows * wi), plan = base.alloc<float>(rows * wp);
  }
};

// The part of a reset the contexts share, in the order every reset keeps: the factor of cov, then
// -- with nothing in flight after `sync` -- the keys and the positions, the context's own state
// (`upload(E)`: host-to-device and the policy's device-to-device copies), done = -1, the factor, the
// handle's mean and the given variates, and last `step()`, the context's reset-mode step.  The
// blocking uploads behind `upload` are what orders its device-to-device copies before the step.
template <class Sync, class Upload, class Step>
int reset_common(Episodes& s, int32_t n_episodes, const double* pos, const float* mean, const float* cov,
                 const float* u, const int32_t* keys, Sync&& sync, Upload&& upload, Step&& step) {
  double cv[64];
  for (int i = 0; i < 64; ++i) cv[i] = double(cov[i]);
  if (!chol8(cv, s.chol_host.data())) return fail(MPCMMD_E_INVALID, "cov_param_init is not positive definite");
  return guarded([&] {
    check_device(s.h);
    sync();  // a reset starts over: nothing of the last run is in flight
    const size_t E = size_t(n_episodes);
    s.E = n_episodes, s.drawn = u == nullptr;
    s.keys.assign(keys, keys + E);
    HIPC(hipMemcpy(s.keys_dev, s.keys.data(), E * 4, hipMemcpyHostToDevice));
    const std::vector<int32_t> running(E, -1);
    HIPC(hipMemcpy(s.pos, pos, E * 2 * 8, hipMemcpyHostToDevice));
    upload(E);
    HIPC(hipMemcpy(s.done, running.data(), E * 4, hipMemcpyHostToDevice));
    HIPC(hipMemcpy(s.chol, s.chol_host.data(), 64 * 8, hipMemcpyHostToDevice));
    HIPC(hipMemcpy(s.h->p.mean, mean, E * 8 * 4, hipMemcpyHostToDevice));
    if (u) {  // [Tmax][n_episodes][wu] -> rows of Emax, one strided copy
      const size_t row = size_t(s.wu) * 4;
      HIPC(hipMemcpy2D(s.u, size_t(s.Emax) * row, u, E * row, E * row, size_t(s.Tmax), hipMemcpyHostToDevice));
    }
    step();
    s.reset_done = true;
    return MPCMMD_OK;
  });
}

// The chained loop: per tick `begin(idx_mpc, covs)` (the context's chained begin), the CEM
// iterations and `after(tick)` (the validation stage and the step), all enqueued.
template <class Begin, class After>
int run_ticks(Episodes& s, int32_t tick_begin, int32_t count, const float* cov, Begin&& begin, After&& after) {
  std::vector<int32_t> idx(s.E);
  const std::vector<float> covs = replicate_cov(cov, s.E);
  for (int k = tick_begin; k < tick_begin + count; ++k) {
    tick_indices(k, s.keys, idx.data());
    if (int rc = begin(idx.data(), covs.data())) return rc;
    if (int rc = mpcmmd_iterate(s.h, 0, s.h->T)) return rc;
    if (int rc = guarded([&] {
          after(k);
          return MPCMMD_OK;
        }))
      return rc;
  }
  return MPCMMD_OK;
}

// the first `ticks` rows of the four log arrays (ticks > 0)
inline void log_rows_back(const Episodes& s, int ticks, double* log_d, float* log_f, int32_t* log_i, float* plan) {
  const size_t E = size_t(s.E), Em = size_t(s.Emax);
  rows_back(log_d, s.logd, size_t(s.wd) * 8, ticks, E, Em), rows_back(log_f, s.logf, size_t(s.wf) * 4, ticks, E, Em);
  rows_back(log_i, s.logi, size_t(s.wi) * 4, ticks, E, Em), rows_back(plan, s.plan, size_t(s.wp) * 4, ticks, E, Em);
}

// mpcmmd_*_validation_log behind the context's null check: "<prefix>: tick range", "<entry> without
// a validation stage"
template <class Sync>
int validation_log_back(Episodes& s, const std::string& prefix, const std::string& entry, int32_t ticks,
                        int32_t* counts, int32_t* count_pos, float* stats, float* mmd, float* est, Sync&& sync) {
  if (!counts || !count_pos || !stats || !est) return fail(MPCMMD_E_INVALID, "null argument");
  if (s.val_on && s.vl.S > 0 && !mmd) return fail(MPCMMD_E_INVALID, "null argument");
  if (ticks < 0 || ticks > s.Tmax) return fail(MPCMMD_E_INVALID, prefix + ": tick range");
  if (!s.val_on) return fail(MPCMMD_E_STATE, entry + " without a validation stage");
  return guarded([&] {
    check_device(s.h);
    sync();
    if (ticks > 0 && s.E > 0) s.vl.read(ticks, size_t(s.E), size_t(s.Emax), counts, count_pos, stats, mmd, est);
    return MPCMMD_OK;
  });
}

// Drops a stage (the validation stage or the vehicle policy) and, with `on`, makes it anew:
// `sync` idles the context's streams first, the next run needs a reset, and a failed `make`
// leaves no half-made stage.
template <class Sync, class Drop, class Make>
int remake_stage(Episodes& s, bool on, Sync&& sync, Drop&& drop, Make&& make) {
  const int rc = guarded([&] {
    check_device(s.h);
    sync();  // nothing in flight reads the buffers about to go
    drop();
    s.reset_done = false;  // the stage changes with the episodes
    return on ? make() : MPCMMD_OK;
  });
  if (rc != MPCMMD_OK) {
    drop();
    (void)hipGetLastError();
  }
  return rc;
}

// the scratch of the validation stage's statistics for Emax episodes of q.R rollouts and q.S
// bandwidths (sigma[q.S], the same for every episode): costs, np and, with bandwidths, sigma, u, part
inline void alloc_risk_scratch(Arena& a, ValidateRiskParams& q, size_t Emax, const float* sigma) {
  const size_t R = size_t(q.R), S = size_t(q.S), n3 = 3 * Emax, tiles = (R + kRiskTile - 1) / kRiskTile;
  q.costs = a.alloc<float>(n3 * R);  // every element is stored by the validators
  q.np = a.alloc<int32_t>(n3);
  if (S > 0) {
    std::vector<float> sg(Emax * S);
    for (size_t i = 0; i < sg.size(); ++i) sg[i] = sigma[i % S];
    q.sigma = a.alloc<float>(sg.size(), sg.data());
    q.u = a.alloc<float>(n3 * R);
    q.part = a.alloc<double>(n3 * tiles * S);
  }
}

// One launch of a step kernel over the caller's host arrays (mpcmmd_*_step_device): inputs go up,
// state and outputs get a device twin and come back after the launch.
struct StepHarness {
  struct Out {
    void* dev;
    void* host;
    size_t bytes;
  };
  Scratch sc;
  std::vector<Out> outs;
  // selects the device; "<prefix>: ..." on a bad argument
  int open(const std::string& prefix, int32_t device, int32_t n_episodes) {
    if (n_episodes < 1 || n_episodes > 65535) return fail(MPCMMD_E_INVALID, prefix + ": 1 <= n_episodes <= 65535");
    int count = 0;
    HIPC(hipGetDeviceCount(&count));
    if (device < 0 || device >= count) return fail(MPCMMD_E_INVALID, prefix + ": no such device");
    HIPC(hipSetDevice(device));
    return MPCMMD_OK;
  }
  // `count` elements uploaded (src null: only allocated)
  template <class T>
  const T* in(const T* src, size_t count) {
    return static_cast<const T*>(sc.up(src, count * sizeof(T)));
  }
  // state and outputs: a device twin of host[count], uploaded first with `upload`, read back by
  // finish(); an empty array still gets a pointer
  template <class T>
  T* io(T* host, size_t count, bool upload) {
    const size_t bytes = count * sizeof(T);
    void* d = sc.up(upload && bytes ? host : nullptr, bytes ? bytes : 16);
    if (bytes) outs.push_back({d, host, bytes});
    return static_cast<T*>(d);
  }
  // after the launch: its error, the device idle, every io array back
  void finish() {
    HIPC(hipGetLastError());
    HIPC(hipDeviceSynchronize());
    for (const Out& o : outs) HIPC(hipMemcpy(o.host, o.dev, o.bytes, hipMemcpyDeviceToHost));
  }
};

}  // namespace mpcmmd
#pragma GCC visibility pop
