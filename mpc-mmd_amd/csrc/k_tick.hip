// The per-tick setup of the CARLA optimizer on the device (main_carla.py:
// 345-382 before compute_cem_*, and the host arithmetic of
// mpcmmd_carla_begin_batch), from the raw tick data to the handle's buffers:
//
//   k_tick_path   custom_path_smoothing + compute_path_parameters
//                 (carla_host.cpp: path_smoothing, path_parameters) -> path
//   k_tick_setup  global_to_frenet_obs + compute_obs_trajectories -> obs,
//                 obs_full; the noisy initial rows, their Frenet states and
//                 boundary vectors (solve_host.cpp: carla_rows) -> st0r; the
//                 KKT columns (solve_columns) -> solve_c
//
// One workgroup per tick.  Every result is bit-equal to the host route's: the
// same fp32 operations in the same order (-ffp-contract=off), transcendentals
// evaluated in fp64 and rounded once (cr_math.hpp), and every sum that the
// host forms sequentially is formed sequentially here --
//   * the smoothing GEMV: a thread owns a row and walks the columns j = 0..P in
//     ascending order, one fp64 multiply and one fp64 add per term (no tree,
//     no split over the columns);
//   * the arc length: one lane's fp64 running sum of the segment lengths;
//   * the six means of the rows' Frenet states: one lane per component, rows
//     in order;
//   * the KKT columns: 3 or 4 fp64 products added in order to 0.0.
//
// LDS (dynamic, tick_lds_bytes): k_tick_path holds the fp64 right-hand sides
// rx, ry [P + 1] of one tick (16 (P + 1) bytes) and reuses the space for six
// fp32 path arrays (24 P bytes); k_tick_setup holds the six path arrays.  The
// largest shape, P = 2048, needs 49168 bytes in either kernel.  The ADMM state
// of a row lives in its thread's registers; rows beyond 1024 are a second row
// of the same thread.
#include "common.hpp"
#include "cr_math.hpp"
#include "frenet.hpp"
#include "host_constants.hpp"
#include "layout.hpp"
#include "tick.hpp"

namespace mpcmmd {

namespace {

constexpr int kPathThreads = 1024;
constexpr int kSetupThreads = 256;

// NR rows per thread: rows tid and tid + blockDim.x (NR blockDim.x >= P)
template <int NR>
__global__ __launch_bounds__(kPathThreads) void k_tick_path(TickParams t) {
  extern __shared__ double sD[];
  const int g = blockIdx.x, P = t.P, n = P + 1, tid = threadIdx.x, nt = blockDim.x;
  const float* in = t.in + size_t(g) * t.lay.stride;
  const float* xwp = in + t.lay.xw;
  const float* ywp = in + t.lay.yw;
  const float thr = t.thr;
  double* rx = sD;
  double* ry = sD + n;
  int row[NR];
  bool ok[NR];
  float xw[NR], yw[NR], d[NR], lx[NR], ly[NR], ca[NR], sa[NR], xs[NR], ys[NR];
#pragma unroll
  for (int q = 0; q < NR; ++q) {
    const int i = tid + q * nt;
    ok[q] = i < P;
    row[q] = ok[q] ? i : P - 1;  // a thread past the path repeats the last row and stores nothing
    xw[q] = xwp[row[q]];
    yw[q] = ywp[row[q]];
    xs[q] = xw[q];
    ys[q] = yw[q];
    d[q] = thr;
    lx[q] = ly[q] = 0.0f;
    ca[q] = 1.0f;  // cos, sin of alpha = 0
    sa[q] = 0.0f;
  }
  const float xw0 = xwp[0], yw0 = ywp[0];
  for (int it = 0; it < 10; ++it) {
#pragma unroll
    for (int q = 0; q < NR; ++q) {
      const float bx = xw[q] + d[q] * ca[q];
      const float by = yw[q] + d[q] * sa[q];
      const float linx = -lx[q] - bx, liny = -ly[q] - by;
      if (ok[q]) {
        rx[row[q]] = -double(linx);
        ry[row[q]] = -double(liny);
      }
    }
    if (tid == 0) {
      rx[P] = double(xw0);
      ry[P] = double(yw0);
    }
    __syncthreads();
    // sol = inv [rhs]: the columns in ascending order (the host's and the oracle's order)
    double sx[NR], sy[NR];
#pragma unroll
    for (int q = 0; q < NR; ++q) sx[q] = sy[q] = 0.0;
#pragma unroll 8
    for (int j = 0; j < n; ++j) {
      const double* col = t.inv + size_t(j) * n;
      const double vx = rx[j], vy = ry[j];
#pragma unroll
      for (int q = 0; q < NR; ++q) {
        const double c = col[row[q]];
        sx[q] = sx[q] + c * vx;
        sy[q] = sy[q] + c * vy;
      }
    }
    __syncthreads();  // every read of rx, ry before the next iteration's stores
#pragma unroll
    for (int q = 0; q < NR; ++q) {
      xs[q] = float(sx[q]);
      ys[q] = float(sy[q]);
      const float wc = xs[q] - xw[q], ws = ys[q] - yw[q];
      const float alpha = cr_atan2(ws, wc);
      cr_sincos(alpha, sa[q], ca[q]);
      const float c1 = ca[q] * ca[q] + sa[q] * sa[q];
      const float c2 = wc * ca[q] + ws * sa[q];
      const float dd = c2 / c1;
      d[q] = dd < thr ? dd : thr;
      lx[q] = lx[q] - (wc - d[q] * ca[q]);
      ly[q] = ly[q] - (ws - d[q] * sa[q]);
    }
  }
  // compute_path_parameters on the smoothed points
  float* X = reinterpret_cast<float*>(sD);
  float* Y = X + P;
  float* FX = Y + P;
  float* FY = FX + P;
  float* SEG = FY + P;
  float* ARC = SEG + P;
  float* out = t.path + size_t(g) * 6 * kMaxPath;
#pragma unroll
  for (int q = 0; q < NR; ++q)
    if (ok[q]) {
      X[row[q]] = xs[q];
      Y[row[q]] = ys[q];
    }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < NR; ++q)
    if (ok[q]) {
      const int j = row[q] < 1 ? 1 : row[q];  // Fx_dot[0] = Fx_dot[1]
      FX[row[q]] = X[j] - X[j - 1];
      FY[row[q]] = Y[j] - Y[j - 1];
    }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < NR; ++q)
    if (ok[q]) {
      const int i = row[q], j = i < 1 ? 1 : i;  // Fx_ddot[0] = Fx_ddot[1]
      const float fx = FX[i], fy = FY[i];
      const float fxdd = FX[j] - FX[j - 1], fydd = FY[j] - FY[j - 1];
      const float s2 = fx * fx + fy * fy;
      SEG[i] = sqrtf(s2);
      const float kap = (fydd * fx - fxdd * fy) / float(pow(double(s2), 1.5));
      out[0 * kMaxPath + i] = xs[q];
      out[1 * kMaxPath + i] = ys[q];
      out[3 * kMaxPath + i] = fx;
      out[4 * kMaxPath + i] = fy;
      out[5 * kMaxPath + i] = kap;
    }
  __syncthreads();
  if (tid == 0) {  // the arc length: one sequential fp64 sum, rounded per element
    double acc = 0.0;
    ARC[0] = 0.0f;
    for (int i = 0; i + 1 < P; ++i) {
      acc += double(SEG[i]);
      ARC[i + 1] = float(acc);
    }
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < NR; ++q)
    if (ok[q]) out[2 * kMaxPath + row[q]] = ARC[row[q]];
  for (int i = P + tid; i < kMaxPath; i += nt) {  // the image's zero padding (path_image)
#pragma unroll
    for (int k = 0; k < 6; ++k) out[k * kMaxPath + i] = 0.0f;
  }
}

struct PathLds {
  int P;
  const float *x, *y, *arc, *Fxd, *Fyd, *kappa;
};

struct Frenet6 {
  float x, y, vx, vy, ax, ay;
};

// a - b as the host's subtraction treats a NaN operand: the NaN itself, sign and
// payload kept (the GPU's subtract is an add of the negated operand, which
// flips a NaN's sign).  Finite results are the same IEEE difference.
DEVI float sub_nan(float a, float b) {
  const float r = a - b;
  return a != a ? a : (b != b ? b : r);
}

// -a as a value the compiler cannot fold into a later subtraction: -a * b + c
// stays a multiply and an add, so a NaN in b or c keeps its sign as on the host
DEVI float neg_opaque(float a) {
  float r = -a;
  asm volatile("" : "+v"(r));
  return r;
}

// carla_host.cpp: closest_index and global_to_frenet, operation for operation
// (NaN signs included: a NaN coordinate reaches d, vx and the tracks with the
// bits the host gives it)
DEVI Frenet6 frenet_state(const PathLds& p, float x, float y, float v, float vdot, float psi, float psidot) {
  int idx = 0;
  float bd = 0.0f;
  for (int j = 0; j < p.P; ++j) {
    const float dx = p.x[j] - x, dy = p.y[j] - y;
    const float dj = sqrtf(dx * dx + dy * dy);
    if (dj != dj) {  // jnp.argmin: the first NaN
      idx = j;
      break;
    }
    if (j == 0 || dj < bd) {
      bd = dj;
      idx = j;
    }
  }
  const float s = p.arc[idx];
  const float ki = interp_jnp(s, p.arc, p.kappa, p.P);
  const float kp = interp_jnp(s + 0.001f, p.arc, p.kappa, p.P);
  const float kprime = (kp - ki) / 0.001f;
  const float Fx = interp_jnp(s, p.arc, p.Fxd, p.P);
  const float Fy = interp_jnp(s, p.arc, p.Fyd, p.P);
  const float nx = neg_opaque(Fy), ny = Fx;
  const float nrm = sqrtf(nx * nx + ny * ny);
  const float d = (1.0f / nrm) * (nx * sub_nan(x, p.x[idx]) + ny * sub_nan(y, p.y[idx]));
  float pf = sub_nan(psi, cr_atan2(Fy, Fx));
  float sp, cp;
  cr_sincos(pf, sp, cp);
  pf = cr_atan2(sp, cp);
  cr_sincos(pf, sp, cp);
  const float om = sub_nan(1.0f, d * ki);
  Frenet6 o;
  o.x = s;
  o.y = d;
  o.vx = v * cp / om;
  o.vy = v * sp;
  const float pd = sub_nan(psidot, ki * o.vx);
  o.ay = vdot * sp + v * cp * pd;
  const float ax1 = sub_nan(vdot * cp, v * sp * pd);
  const float ax2 = sub_nan(neg_opaque(o.vy) * ki, d * kprime * o.vx);
  o.ax = sub_nan(ax1 * om, (v * cp) * ax2) / (om * om);
  return o;
}

__global__ __launch_bounds__(kSetupThreads) void k_tick_setup(TickParams t) {
  extern __shared__ float sP[];
  __shared__ float sm[6];
  const int g = blockIdx.x, P = t.P, O = t.O, H = t.H, R = t.R, R0 = t.R0, tid = threadIdx.x, nt = blockDim.x;
  const float* in = t.in + size_t(g) * t.lay.stride;
  {
    const float* pa = t.path + size_t(g) * 6 * kMaxPath;
    for (int i = tid; i < P; i += nt) {
#pragma unroll
      for (int k = 0; k < 6; ++k) sP[k * P + i] = pa[k * kMaxPath + i];
    }
  }
  __syncthreads();
  const PathLds pl{P, sP, sP + P, sP + 2 * P, sP + 3 * P, sP + 4 * P, sP + 5 * P};
  // the obstacles: global_to_frenet_obs, then the constant-velocity tracks on
  // np.linspace(0, 15, 100).astype(float32)
  float* ob = t.obs + size_t(g) * 2 * O * H;
  float* of = t.det ? t.obs_full + size_t(g) * 2 * O * kNum : nullptr;
  for (int o = tid; o < O; o += nt) {
    const float* q = in + t.lay.obs + 5 * o;
    const float vx = q[2], vy = q[3];
    const float v = sqrtf(vx * vx + vy * vy);
    const Frenet6 f = frenet_state(pl, q[0], q[1], v, 0.0f, q[4], 0.0f);
    for (int k = 0; k < kNum; ++k) {
      const float tt = k == kNum - 1 ? 15.0f : float(double(k) * (15.0 / 99.0));
      const float xv = f.x + f.vx * tt, yv = f.y + f.vy * tt;
      if (k < H) {
        ob[size_t(o) * H + k] = xv;
        ob[size_t(O) * H + size_t(o) * H + k] = yv;
      }
      if (of) {
        of[size_t(o) * kNum + k] = xv;
        of[size_t(O) * kNum + size_t(o) * kNum + k] = yv;
      }
    }
  }
  // the noisy initial rows (carla_rows) and their Frenet states
  const float x0 = in[0], y0 = in[1], v0 = in[2], vdot = in[3], psi0 = in[4], psidot = in[5];
  float s0, c0;
  cr_sincos(psi0, s0, c0);
  const float vx = v0 * c0, vy = v0 * s0;
  const float psi = cr_atan2(vy, vx);
  const float vn = sqrtf(vx * vx + vy * vy);
  float* rows = t.st0r + size_t(g) * R0 * 8;
  float* fr = t.fr + size_t(g) * R0 * 6;
  for (int r = tid; r < R0; r += nt) {
    float o8[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (r < R) {
      const float* e = in + t.lay.eps + 4 * r;
      o8[0] = x0 + (e[0] * t.sg_x + t.mu_x);
      o8[1] = y0 + (e[1] * t.sg_y + t.mu_y);
      o8[2] = vx;
      o8[3] = vy;
      o8[4] = psi;
      const Frenet6 f = frenet_state(pl, o8[0], o8[1], vn, vdot, psi, psidot);
      float* w = fr + size_t(r) * 6;
      w[0] = f.x, w[1] = f.y, w[2] = f.vx, w[3] = f.vy, w[4] = f.ax, w[5] = f.ay;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) rows[size_t(r) * 8 + k] = o8[k];
  }
  __threadfence();
  __syncthreads();
  if (tid < 6) {  // sequential fp64 sums in row order (the oracle's cumsum order)
    double sum = 0.0;
    for (int r = 0; r < R; ++r) sum += double(fr[size_t(r) * 6 + tid]);
    sm[tid] = float(sum / double(R));
  }
  __syncthreads();
  if (tid < 4 * kNvar) {  // solve_columns: guess x, guess y, projection x, projection y
    const int c = tid / kNvar;
    const bool isy = c & 1;
    const double b[4] = {double(sm[isy ? 1 : 0]), double(sm[isy ? 3 : 2]), double(sm[isy ? 5 : 4]), 0.0};
    const double* a = t.kcol + size_t(tid) * 4;
    double sc = 0.0;
    const int ne = isy ? 4 : 3;
    for (int e = 0; e < ne; ++e) sc += a[e] * b[e];
    t.solve_c[size_t(g) * 4 * kNvar + tid] = sc;
  }
}

}  // namespace

void launch_tick_path(const TickParams& t, hipStream_t s) {
  const int threads = t.P >= kPathThreads ? kPathThreads : (t.P + 63) / 64 * 64;
  const size_t lds = tick_lds_bytes(t.P);
  if (t.P > kPathThreads) k_tick_path<2><<<t.G, threads, lds, s>>>(t);
  else k_tick_path<1><<<t.G, threads, lds, s>>>(t);
}

void launch_tick_setup(const TickParams& t, hipStream_t s) {
  k_tick_setup<<<t.G, kSetupThreads, tick_lds_bytes(t.P), s>>>(t);
}

}  // namespace mpcmmd
