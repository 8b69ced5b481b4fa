// The handle behind the C ABI (include/mpcmmd.h) and what its three sources
// share: handle.hip (create / destroy, knobs, debug and profiling API),
// begin.hip (per-solve setup and results) and sequence.hip (the launch
// sequence and its graph capture).  Internal to the library.
#pragma once
#include <map>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

#include "api_common.hpp"
#include "kernels.hpp"  // before buffers.hpp: HIP's int2
#include "buffers.hpp"

namespace mpcmmd {

// X(id suffix, name of mpcmmd_kernel_name): the launches the profiler tells apart
#define MPCMMD_KERNELS(X)                                                                                        \
  X(Noise, "noise") X(Front, "front") X(RiskBaseline, "risk_baseline") X(Mother, "mother") X(BDist, "bdist")     \
  X(BSample, "bsample") X(BSelect, "bselect") X(BKernel, "bkernel") X(BQp, "bqp") X(BElite, "belite")            \
  X(MmdFinal, "mmdfinal") X(Select, "select") X(GammaTab, "gamma_tab") X(BetaPlanes, "beta_planes")              \
  X(BGen, "bgen") X(BMoment, "bmoment") X(BDirect, "bdirect") X(RollCarla, "roll_carla") X(Frenet, "frenet")     \
  X(RiskCarla, "risk_carla") X(BcemSmall, "bcem_small") X(TickPath, "tick_path") X(TickSetup, "tick_setup")
enum KernelId {
#define X(id, name) kK##id,
  MPCMMD_KERNELS(X)
#undef X
  kNumKernels
};

}  // namespace mpcmmd

struct mpcmmd_handle {
  mpcmmd_config cfg{};
  mpcmmd::ProblemConsts pc;
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  mpcmmd::Params p{};
  int B = 0, S = 0, H = 0, O = 0, n = 0, M = 0, T = 0;
  int Gmax = 1;  // configurations the buffers hold (mpcmmd_create_batch)
  int G = 1;     // configurations of the current solve
  // the device buffers that exist, in the order of buffers.hpp's list
  struct Buf {
    const char* name;
    void* ptr;
    size_t bytes;
  };
  std::vector<Buf> bufs;
  // solve state
  int cost = -1;
  bool begun = false;
  int last_t = -1;
  bool ext_roll = false, ext_res = false;
  bool beta_tables_internal = false;  // device beta tables hold the internal streams
  bool sel0_valid = false;            // sel0 / sig0 / rp0 / rpair0 match the device beta_z0
  // generation of the sel0 table (bumped by every rebuild) and the one
  // k_bmoment last used for the first beta-iteration's direct row sums: the
  // stage API may rewrite beta_z0 between stage 4 and stage 5/6 at t = 0
  unsigned sel0_gen = 0, bmoment_gen = ~0u;
  bool mmd_ok = false;                // mmd_opt buffers allocated (mmdopt_supported)
  bool carla = false;                 // CARLA variant handle (mpcmmd_carla_begin)
  int R0 = 0;                         // noisy initial rows per configuration (CARLA)
  std::vector<double> det_kx, det_ky;  // KKT inverses of the CARLA det projection (14^2, 15^2)
  std::string mmd_why;
  // pinned staging for the per-solve uploads of mpcmmd_begin: the copies are
  // asynchronous, so their source must outlive the call; the next begin waits
  // for stage_ev before refilling it
  char* stage = nullptr;
  size_t stage_bytes = 0, stage_used = 0;
  hipEvent_t stage_ev = nullptr;
  bool stage_pending = false;
  // candidate groups of the beta-CEM, each on its own stream (kernels of
  // different groups overlap); 1 = everything on the handle's stream
  static constexpr int kMaxGroups = 4;
  int groups = 1;
  bool groups_forced = false;
  int small_groups = 2;  // groups for launches of 64..256 candidates (MPCMMD_SMALL_GROUPS)
  hipStream_t gstream[kMaxGroups] = {};
  hipEvent_t gev_start = nullptr, gev_done[kMaxGroups] = {};
  // whole-solve graphs: mpcmmd_iterate(0, T) captured once per (cost, path
  // length, external draws, configurations) and replayed (one hipGraphLaunch
  // instead of ~150 launches per outer iteration)
  bool graphs = false;
  using GraphKey = std::tuple<int, int, int, int, int, int, int>;
  std::map<GraphKey, std::pair<hipGraph_t, hipGraphExec_t>> gexec;
  std::map<GraphKey, int> gahead;  // ahead_t after the captured iterations ran
  // draws ahead: k_select of iteration t also draws iteration t + 1's noise
  // and Beta attempt table (draws.hpp); ahead_t = the iteration whose draws
  // are already on the device that way (-1: none).  Deterministic draws, so
  // producing them early changes no value; invalidated by begin and by any
  // gamma table drawn for another iteration (the table has one slot)
  bool ahead_on = true;
  int ahead_t = -1;
  // k_select's residual sort and cost norms run in the risk launch where it
  // is k_risk_baseline (Params::select_prep); MPCMMD_SELECT_PREP=0: in
  // k_select / k_front
  bool prep_on = true;
  // sampling_param's internal standard normals [B][8] (fixed key: every solve's)
  std::vector<float> pop0_normals;
  // the iteration whose residual sort and cost norms the risk launch made
  // (-1: none since begin / the last front stage); stage 3 with select_prep
  // needs them for its own t
  int prep_t = -1;
  // small batches: the 20 beta-iterations as one launch (k_bcem_small);
  // MPCMMD_FUSED=0 keeps the per-iteration kernels
  bool fused_small = true;
  // profiling
  bool prof = false;
  std::vector<std::pair<int, std::pair<hipEvent_t, hipEvent_t>>> pending;
  std::vector<hipEvent_t> free_events;
  int launches[mpcmmd::kNumKernels] = {0};
  double total_ms[mpcmmd::kNumKernels] = {0};

  size_t alloc_total = 0;
  size_t alloc_cap = 0;  // MPCMMD_MAX_HANDLE_BYTES (tests): refuse buffers past it with a real HIP OOM
  // one line of buffers.hpp's list: null for a buffer this handle's shape lacks
  void* alloc(const mpcmmd::BufferSpec& s) {
    if (!s.bytes) return nullptr;
    void* d = nullptr;
    alloc_total += s.bytes;
    // over the cap: ask for an impossible size, so the failure is the
    // runtime's own out-of-memory error (and its sticky last-error state)
    HIPC(hipMalloc(&d, alloc_cap && alloc_total > alloc_cap ? (size_t(1) << 52) : s.bytes));
    // zeroed on the handle's own (non-blocking) stream: a null-stream memset
    // is not ordered before the constant uploads that follow on this stream
    // and could land after them
    HIPC(hipMemsetAsync(d, 0, s.bytes, stream));
    bufs.push_back({s.name, d, s.bytes});
    return d;
  }
  // the buffer a Params member points to (its base)
  const Buf& buf_of(const void* d) const {
    for (const Buf& b : bufs)
      if (b.ptr == d) return b;
    throw std::logic_error("not a buffer of the handle");
  }
  hipEvent_t ev() {
    if (!free_events.empty()) {
      hipEvent_t e = free_events.back();
      free_events.pop_back();
      return e;
    }
    hipEvent_t e;
    HIPC(hipEventCreate(&e));
    return e;
  }
  template <class F>
  void launch(int kid, F&& f) {
    if (!prof) {
      f();
      HIPC(hipGetLastError());
      return;
    }
    hipEvent_t a = ev(), b = ev();
    HIPC(hipEventRecord(a, stream));
    f();
    HIPC(hipGetLastError());
    HIPC(hipEventRecord(b, stream));
    pending.push_back({kid, {a, b}});
  }
  void collect() {
    for (auto& pe : pending) {
      float ms = 0.f;
      HIPC(hipEventSynchronize(pe.second.second));
      HIPC(hipEventElapsedTime(&ms, pe.second.first, pe.second.second));
      launches[pe.first] += 1;
      total_ms[pe.first] += ms;
      free_events.push_back(pe.second.first);
      free_events.push_back(pe.second.second);
    }
    pending.clear();
  }
};

namespace mpcmmd {

inline void check_device(mpcmmd_handle* h) { HIPC(hipSetDevice(h->device)); }

// Copy `bytes` at src into the buffer behind the Params member dst, from byte
// `offset` on, on the handle's stream (handle.hip).  Throws past the buffer's end.
void upload(mpcmmd_handle* h, const void* dst, const void* src, size_t bytes, size_t offset = 0);

// host Philox normals of stream (stream, word1) with key (k0, k1): `count` values (begin.hip)
std::vector<float> host_normals(uint32_t k0, uint32_t k1, uint32_t stream, uint32_t word1, size_t count);

// The tick route of a begin (tick_api.hip): the device makes the path, the
// obstacle tracks, the noisy rows and the KKT columns from the raw tick data.
// begin_impl calls enqueue once, inside its guarded section, with the
// init_eps normals of every configuration (eps[g] -> [R][4]).
struct TickRoute {
  int num_path;
  void* ctx;
  void (*enqueue)(void* ctx, int G, int cost_kind, int R, const float* const* eps);
  // the world route: init_state, st0, the first population and the mean are on the device already
  // (k_world_step wrote them), so begin_impl uploads none of them
  bool chained = false;
};

// mpcmmd_begin for n_cfg configurations (begin.hip).  path: n_cfg paths (the
// CARLA host route); tick: the CARLA tick route, which takes no path and no
// obstacle tracks (x_obs, y_obs null) and no external draws.  resident: the
// synthetic closed loop's route (mpc_api.hip) for static / dynamic handles, on
// which st0, solve_c, obs, the first population and the mean are on the device
// already (k_mpc_step wrote them; init_state, mean, x_obs, y_obs are not read):
// only idx_mpc, v_des and cov are staged.  resident with idx_mpc and v_des both
// null: the scene queue's mode, in which those two are on
// the device as well (k_mpc_queue wrote them) and only cov is staged.
int begin_impl(mpcmmd_handle* h, int32_t n_cfg, int32_t cost_kind, const int32_t* idx_mpc, const float* init_state,
               const float* mean, const float* cov, const float* x_obs, const float* y_obs, const float* v_des,
               const mpcmmd_draws* draws, const mpcmmd_path* path = nullptr, const TickRoute* tick = nullptr,
               bool resident = false);

}  // namespace mpcmmd
