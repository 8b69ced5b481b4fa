// Cross-lane primitives (gfx950, wave64), each written once: the typed DPP
// move, readlane, the permlane swaps, the quad / row-of-16 / wave reductions,
// the transposing multi-value totals and the intra-wave LDS hand-off.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define DEVI __device__ __forceinline__

namespace mpcmmd {

constexpr int kWave = 64;

// ---- moves -------------------------------------------------------------------
// gfx9 DPP controls: quad_perm(a,b,c,d) a | b << 2 | c << 4 | d << 6 (0xB1 =
// (1,0,3,2), 0x4E = (2,3,0,1), 0x00 / 0x55 / 0xAA / 0xFF broadcast quad lane
// 0..3), row_shl:4 0x104, row_shr:4 0x114, row_ror:4 0x124, row_ror:8 0x128,
// row_mirror 0x140, row_half_mirror 0x141, row_bcast:15 0x142, row_bcast:31
// 0x143.  Rows disabled by ROWS read 0.
// With every row enabled a lane without a source reads 0 through
// bound_ctrl, so no old value is needed (no register to initialise); with
// rows disabled those keep the old value 0.
template <int CTRL, int ROWS = 0xF>
DEVI int dpp_i(int v) {
  if constexpr (ROWS == 0xF)
    return __builtin_amdgcn_mov_dpp(v, CTRL, 0xF, 0xF, true);
  else
    return __builtin_amdgcn_update_dpp(0, v, CTRL, ROWS, 0xF, false);
}

// the 32-bit words of a 4- or 8-byte value and back (bit casts: transport only)
template <class T>
DEVI int lo_word(T v) {
  static_assert(sizeof(T) == 4 || sizeof(T) == 8, "one or two 32-bit words");
  if constexpr (sizeof(T) == 4)
    return __builtin_bit_cast(int, v);
  else
    return int(__builtin_bit_cast(unsigned long long, v));
}
template <class T>
DEVI int hi_word(T v) {
  static_assert(sizeof(T) == 8, "two 32-bit words");
  return int(__builtin_bit_cast(unsigned long long, v) >> 32);
}
template <class T>
DEVI T from_words(int lo, int hi = 0) {
  if constexpr (sizeof(T) == 4)
    return __builtin_bit_cast(T, lo);
  else
    return __builtin_bit_cast(T, (static_cast<unsigned long long>(unsigned(hi)) << 32) | unsigned(lo));
}

// the DPP move of int, uint32_t, float, double or unsigned long long
template <int CTRL, int ROWS = 0xF, class T>
DEVI T dpp(T v) {
  if constexpr (sizeof(T) == 4) {
    return from_words<T>(dpp_i<CTRL, ROWS>(lo_word(v)));
  } else {
    const int lo = dpp_i<CTRL, ROWS>(lo_word(v)), hi = dpp_i<CTRL, ROWS>(hi_word(v));
    return from_words<T>(lo, hi);
  }
}
// the same move where lanes without a source, and rows ROWS disables, read old
template <int CTRL, int ROWS = 0xF, class T>
DEVI T dpp_old(T v, T old) {
  static_assert(sizeof(T) == 4, "32-bit values");
  return from_words<T>(__builtin_amdgcn_update_dpp(lo_word(old), lo_word(v), CTRL, ROWS, 0xF, false));
}
// lane l's value (l wave-uniform)
template <class T>
DEVI T readlane(T v, int l) {
  if constexpr (sizeof(T) == 4) {
    return from_words<T>(__builtin_amdgcn_readlane(lo_word(v), l));
  } else {
    const int lo = __builtin_amdgcn_readlane(lo_word(v), l), hi = __builtin_amdgcn_readlane(hi_word(v), l);
    return from_words<T>(lo, hi);
  }
}

// v_permlane32_swap (W = 32): lanes 32-63 of x <-> lanes 0-31 of y;
// v_permlane16_swap (W = 16): the odd 16-lane rows of x <-> the even rows of y.
// Inline asm: hipcc (ROCm 7.2) may commute the builtins' two operands, which
// exchanges the other halves.  s_nop 1: the VALU-write -> permlane hazard.
template <int W, class T>
DEVI void permlane_swap(T& x, T& y) {
  static_assert(W == 32 || W == 16, "permlane32_swap or permlane16_swap");
  if constexpr (sizeof(T) == 4) {
    float a = from_words<float>(lo_word(x)), b = from_words<float>(lo_word(y));
    if constexpr (W == 32)
      __asm__ volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
    else
      __asm__ volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(a), "+v"(b));
    x = from_words<T>(lo_word(a));
    y = from_words<T>(lo_word(b));
  } else {
    int xl = lo_word(x), xh = hi_word(x), yl = lo_word(y), yh = hi_word(y);
    permlane_swap<W>(xl, yl);
    permlane_swap<W>(xh, yh);
    x = from_words<T>(xl, xh);
    y = from_words<T>(yl, yh);
  }
}

// value of quad lane l (0..3) in every lane of the quad; l is a constant
// after unrolling, so the switch folds
template <class T>
DEVI T quad_bcast(T v, int l) {
  switch (l & 3) {
    case 0: return dpp<0x00>(v);
    case 1: return dpp<0x55>(v);
    case 2: return dpp<0xAA>(v);
    default: return dpp<0xFF>(v);
  }
}

// Intra-wave LDS hand-off: a wave's LDS operations execute in order, so only
// the compiler must be kept from reordering them (no memory-counter waits).
DEVI void wave_sync() {
  __builtin_amdgcn_wave_barrier();
  __asm__ volatile("" ::: "memory");
}

// ---- reductions ----------------------------------------------------------------
// One butterfly over a scope, VALU only (a __shfl_xor butterfly is an
// LDS-crossbar round trip, ds_bpermute, per step): the two quad_perm steps
// (quad: bit-identical in its 4 lanes), the two row_ror steps (row of 16:
// every lane of the row holds the result), and for the wave the row
// broadcasts into lane 63 and one readlane (wave-uniform result).
// What a lane without a source reads is the operation's:
//   LaneSum    v + w; bound_ctrl / old 0, the identity of the sum
//   LaneMax    fmaxf (NaN ignored unless every lane is NaN); old = v: rows a
//              broadcast does not write keep their own value
//   LaneMinU   unsigned minimum; old = ~0, the identity
//   LaneMaxU   unsigned maximum; old = 0, the identity
enum class Scope { Quad, Row16, Wave };
struct LaneSum {
  template <int CTRL, int ROWS, class T>
  static DEVI T step(T v) { return v + dpp<CTRL, ROWS>(v); }
};
struct LaneMax {
  template <int CTRL, int ROWS>
  static DEVI float step(float v) { return fmaxf(v, dpp_old<CTRL, ROWS>(v, v)); }
};
struct LaneMinU {
  template <int CTRL, int ROWS>
  static DEVI uint32_t step(uint32_t v) { return min(v, dpp_old<CTRL, ROWS>(v, ~0u)); }
};
struct LaneMaxU {
  template <int CTRL, int ROWS>
  static DEVI uint32_t step(uint32_t v) { return max(v, dpp_old<CTRL, ROWS>(v, 0u)); }
};
template <Scope S, class Op, class T>
DEVI T lane_reduce(T v) {
  v = Op::template step<0xB1, 0xF>(v);
  v = Op::template step<0x4E, 0xF>(v);
  if constexpr (S != Scope::Quad) {
    v = Op::template step<0x124, 0xF>(v);
    v = Op::template step<0x128, 0xF>(v);
  }
  if constexpr (S == Scope::Wave) {
    v = Op::template step<0x142, 0xA>(v);
    v = Op::template step<0x143, 0xC>(v);
    v = readlane(v, 63);
  }
  return v;
}
template <class T>
DEVI T quad_sum(T v) { return lane_reduce<Scope::Quad, LaneSum>(v); }
template <class T>
DEVI T row16_total(T v) { return lane_reduce<Scope::Row16, LaneSum>(v); }
DEVI float row16_max(float v) { return lane_reduce<Scope::Row16, LaneMax>(v); }
template <class T>
DEVI T wave_total(T v) { return lane_reduce<Scope::Wave, LaneSum>(v); }
DEVI float wave_max(float v) { return lane_reduce<Scope::Wave, LaneMax>(v); }
DEVI uint32_t wave_min_u32(uint32_t v) { return lane_reduce<Scope::Wave, LaneMinU>(v); }

// 64-bit words and the Frenet scan's quad index: shuffles
DEVI unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    unsigned long long w = __shfl_xor(v, o, kWave);
    v = w > v ? w : v;
  }
  return v;
}
DEVI unsigned long long wave_min_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    unsigned long long w = __shfl_xor(v, o, kWave);
    v = w < v ? w : v;
  }
  return v;
}
DEVI int quad_min_i(int v) {
  v = min(v, __shfl_xor(v, 1));
  return min(v, __shfl_xor(v, 2));
}

// ---- transposing totals of several per-lane values -------------------------------
// Each butterfly step halves the values a lane carries and keeps the half
// that the lane bit the pairing flips selects, so k values cost about a third
// of the instructions of k separate reductions.

// Wave totals of up to 16 values (v[n..15] taken as 0): lane l ends with the
// total of v[l >> 2].  permlane32 / permlane16 swaps (lanes < 32 keep values
// 0..7, odd rows the upper four), row_mirror and row_half_mirror, the quad.
template <class T, int n>
DEVI T wave_totals16(const T (&v)[n]) {
  static_assert(n <= 16, "at most 16 values");
  const int lane = threadIdx.x & 63;
  auto at = [&](int i) { return i < n ? v[i] : T(0); };
  T w[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {  // lanes < 32 keep values 0..7, lanes >= 32 values 8..15
    T a = at(i), b = at(i + 8);
    permlane_swap<32>(a, b);
    w[i] = a + b;
  }
  T x[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {  // odd rows keep the upper four
    T a = w[i], b = w[i + 4];
    permlane_swap<16>(a, b);
    x[i] = a + b;
  }
  const bool b3 = lane & 8, b2 = lane & 4;
  T y[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {  // row_mirror pairs l with l ^ 15 (bit 3 flipped)
    const T keep = b3 ? x[i + 2] : x[i], send = b3 ? x[i] : x[i + 2];
    y[i] = keep + dpp<0x140>(send);
  }
  // row_half_mirror pairs l with l ^ 7 (bit 2 flipped)
  T z = (b2 ? y[1] : y[0]) + dpp<0x141>(b2 ? y[0] : y[1]);
  z += dpp<0xB1>(z);
  return z + dpp<0x4E>(z);
}

// Row-of-16 totals of 16 values: lane l of each 16-lane row ends with the
// row's total of v[l & 15].
DEVI float row16_totals16(const float (&v)[16]) {
  const int lane = threadIdx.x & 15;
  const bool b3 = lane & 8, b2 = lane & 4, b1 = lane & 2, b0 = lane & 1;
  float y[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {  // row_mirror: l <-> 15 - l (bit 3 flipped)
    const float keep = b3 ? v[i + 8] : v[i], send = b3 ? v[i] : v[i + 8];
    y[i] = keep + dpp<0x140>(send);
  }
  float z[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {  // row_half_mirror: l <-> l ^ 7 (bit 2 flipped)
    const float keep = b2 ? y[i + 4] : y[i], send = b2 ? y[i] : y[i + 4];
    z[i] = keep + dpp<0x141>(send);
  }
  float w[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {  // quad_perm(2,3,0,1): l <-> l ^ 2
    const float keep = b1 ? z[i + 2] : z[i], send = b1 ? z[i] : z[i + 2];
    w[i] = keep + dpp<0x4E>(send);
  }
  const float keep = b0 ? w[1] : w[0], send = b0 ? w[0] : w[1];  // quad_perm(1,0,3,2): l <-> l ^ 1
  return keep + dpp<0xB1>(send);
}

// Wave totals of 8 values: lanes 8 j + 4 .. 8 j + 7 end with the total of
// v[j] (row_ror:4 moves lane i - 4 into lane i, so an 8-lane group's total
// lands in its upper quad).  lane: the caller's lane index, read as the
// caller reads its thread index (the beta-CEM phase bodies: tidx()).
DEVI float dpp_f_ror8(float v) { return dpp<0x128>(v); }
DEVI float transpose_sum8(const float (&v)[8], int lane) {
  float a[4], c2[2];
#pragma unroll
  for (int i = 0; i < 4; ++i) {  // lanes 0-31: slots 0..3, lanes 32-63: slots 4..7
    float x = v[i], y = v[4 + i];
    permlane_swap<32>(x, y);
    a[i] = x + y;
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {  // lane bit 4 picks slot 4 h + 2 b4 + i
    float x = a[i], y = a[2 + i];
    permlane_swap<16>(x, y);
    c2[i] = x + y;
  }
  const bool b3 = lane & 8;  // lane bit 3 picks slot 4 h + 2 b4 + b3 = lane >> 3
  const float y0 = dpp_f_ror8(c2[0]), y1 = dpp_f_ror8(c2[1]);
  float x = b3 ? c2[1] + y1 : c2[0] + y0;
  x += dpp<0xB1>(x);
  x += dpp<0x4E>(x);
  return x + dpp<0x124>(x);
}

}  // namespace mpcmmd
