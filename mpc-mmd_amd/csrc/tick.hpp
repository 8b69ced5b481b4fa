// The CARLA tick route (mpcmmd_carla_tick_begin_batch): what k_tick.hip (the
// kernels) and tick_api.hip (the tick context) share.  Internal to the library.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace mpcmmd {

// One tick's raw inputs in the tick context's input buffer, in floats from the
// tick's base (every array 16-byte aligned): init_state [6], x_wp [P], y_wp
// [P], obstacles [O][5], init_eps [R0][4].
struct TickLayout {
  int xw, yw, obs, eps, stride;
};
inline TickLayout tick_layout(int P, int O, int R0) {
  const int Pa = (P + 3) & ~3, Oa = (5 * O + 3) & ~3;
  TickLayout l;
  l.xw = 8;
  l.yw = l.xw + Pa;
  l.obs = l.yw + Pa;
  l.eps = l.obs + Oa;
  l.stride = l.eps + 4 * R0;
  return l;
}

// dynamic LDS of the two kernels: the fp64 right-hand sides rx, ry [P + 1] of
// k_tick_path, then its six fp32 path arrays; the six path arrays of
// k_tick_setup.  P = 2048: 49168 bytes.
inline size_t tick_lds_bytes(int P) { return size_t(24) * P + 16; }

struct TickParams {
  int G, P, O, H, R, R0, det;
  float thr;
  TickLayout lay;
  float mu_x, mu_y, sg_x, sg_y;  // compute_noisy_init_state's offsets and scales (fp32)
  const double* inv;             // (P + 1)^2 smoothing inverse, column-major
  const double* kcol;            // [4][11][4] KKT coefficient columns (guess x, y, projection x, y)
  const float* in;               // [G][lay.stride]
  float* fr;                     // [G][R0][6] Frenet states of the noisy rows
  // slices of the handle's buffers (kernels.hpp: Params)
  float* path;                   // [G][6][kMaxPath]
  float* st0r;                   // [G][R0][8]
  float* obs;                    // [G][2][O][H]
  float* obs_full;               // [G][2][O][100] (det)
  double* solve_c;               // [G][4][11]
};

void launch_tick_path(const TickParams& t, hipStream_t s);
void launch_tick_setup(const TickParams& t, hipStream_t s);

}  // namespace mpcmmd

// What the world route (world_api.hip) needs of a tick context (tick_api.hip).
struct mpcmmd_tick;
struct mpcmmd_handle;
namespace mpcmmd {
mpcmmd_handle* tick_handle(mpcmmd_tick* t);
int tick_num_path(const mpcmmd_tick* t);
TickLayout tick_layout_of(const mpcmmd_tick* t);
float* tick_inputs_device(mpcmmd_tick* t);  // [Gmax][stride]
// mpcmmd_carla_tick_begin_batch on raw inputs that k_world_step has already
// written to the context's input image, with st0, the first population and
// the mean on the device too: only idx_mpc, v_des, cov and the init_eps
// normals are staged.  Argument checks as the tick begin's, before any HIP call.
int tick_begin_chained(mpcmmd_tick* t, int32_t n_cfg, int32_t cost_kind, const int32_t* idx_mpc, const float* cov,
                       const float* v_des, float threshold);
}  // namespace mpcmmd
