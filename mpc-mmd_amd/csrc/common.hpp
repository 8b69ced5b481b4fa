// Device helpers shared by the kernels (gfx950, wave64); the cross-lane
// primitives are in lanes.hpp.
// Everything in this library is compiled with -ffp-contract=off: the fp32
// elementwise expressions follow the reference's operation order exactly and
// only explicit fmaf()/fma() fuse.
#pragma once
#include "lanes.hpp"

#define HDI __host__ __device__ __forceinline__

namespace mpcmmd {

// phase timestamp of workgroup 0 into dbg[slot] (profiling only)
#define MPCMMD_STAMP(p, slot)                                                   \
  do {                                                                          \
    if (blockIdx.x == 0 && threadIdx.x == 0 && (p).dbg)                         \
      (p).dbg[(slot)] = __builtin_amdgcn_s_memrealtime();                       \
  } while (0)


// per-workgroup phase timestamp into dbgw[blockIdx.x][slot] (profiling only;
// the workgroups of one launch, slots 0..7)
#define MPCMMD_STAMPW(p, slot)                                                      \
  do {                                                                              \
    const unsigned wg_ = blockIdx.x + gridDim.x * blockIdx.y;                       \
    if (threadIdx.x == 0 && (p).dbgw && wg_ < 65536)                                \
      (p).dbgw[size_t(wg_) * 8 + (slot)] = __builtin_amdgcn_s_memrealtime();        \
  } while (0)

// ---- ordering ----------------------------------------------------------------
// jnp.argsort total order on fp32: -0 == +0, every NaN equal and last.
HDI uint32_t sort_key(float x) {
  if (x == 0.0f) x = 0.0f;
  if (x != x) return 0xFFFFFFFFu;
#ifdef __HIP_DEVICE_COMPILE__
  uint32_t u = __float_as_uint(x);
#else
  uint32_t u;
  __builtin_memcpy(&u, &x, 4);
#endif
  return (u >> 31) ? ~u : (u | 0x80000000u);
}

// sort_key(fabsf(x)) in four VALU operations: |x| has no sign and no -0, so
// the key is its bit pattern with bit 31 set, or ~0 for a NaN (pattern above
// +inf's) -- the same value for every x
DEVI uint32_t sort_key_abs(float x) {
  const uint32_t u = __float_as_uint(x) & 0x7FFFFFFFu;
  return u > 0x7F800000u ? 0xFFFFFFFFu : (u | 0x80000000u);
}

// ---- arithmetic --------------------------------------------------------------
// x / d for a divisor known in advance, r = RN(1/d): one FMA correction of
// RN(x r).  Bit-equal to IEEE division for every x when d = 2.5, and for
// d = 4.25^2, 2.75^2 wherever |x| >= 2^-117 (checked exhaustively on the host;
// below that the caller's "+ 1" absorbs any difference).  For run-time
// divisors it is within 1 ulp (used only where results are tolerance-checked).
DEVI float div_rc(float x, float d, float r) {
  float q = x * r;
  float e = fmaf(-q, d, x);
  return fmaf(e, r, q);
}

}  // namespace mpcmmd
