// Does VALU / memory work issued between fp64 MFMAs of the same wave run in
// their shadow on gfx950?  (profiling aid for k_bsample, not product code)
// One wave alone on its SIMD issues N rounds of 6 independent
// v_mfma_f64_16x16x4 (6 accumulators, so no MFMA waits on another), with F
// filler instructions after each MFMA; inline asm keeps the order exact.
// Prints clocks per MFMA for each filler kind and count.  Fillers: VALU
// (add_f32, add_f64, both conversions, cndmask, AccVGPR reads and writes),
// SALU (s_add_u32, s_mul_i32) and a store.  k_readback: a VALU read of the
// result of the MFMA issued K MFMAs earlier, with the builtin MFMA so that
// the compiler's hazard recognizer sees the dependency (it does not see into
// asm) and sched barriers to keep the order.
#include <hip/hip_runtime.h>

#include <cstdio>

typedef double d4 __attribute__((ext_vector_type(4)));

#define MF(acc) asm volatile("v_mfma_f64_16x16x4_f64 %0, %1, %2, %0" : "+v"(acc) : "v"(a), "v"(b))

template <int KIND, int F>
__global__ void k_overlap(unsigned long long* out, float* sink, int rounds) {
  d4 c0 = {0, 0, 0, 0}, c1 = c0, c2 = c0, c3 = c0, c4 = c0, c5 = c0;
  const double a = threadIdx.x * 1e-3, b = 1.0 + threadIdx.x * 1e-4;
  float x0 = threadIdx.x, x1 = x0 + 1, x2 = x0 + 2, x3 = x0 + 3;
  double y0 = x0, y1 = x1;
  float* dst = sink + threadIdx.x;
  float g0 = 0, g1 = 0;  // AccVGPRs ("a" constraints)
  int k0 = rounds, k1 = rounds + 1;
  asm volatile("v_accvgpr_write_b32 %0, %1" : "=a"(g0) : "v"(x0));
  asm volatile("s_mov_b64 vcc, exec" ::: "vcc");
  auto fill = [&]() {
#pragma unroll
    for (int f = 0; f < F; ++f) {
      if constexpr (KIND == 0)
        asm volatile("v_add_f32 %0, %0, %1" : "+v"(f & 1 ? x1 : x0) : "v"(x2));
      else if constexpr (KIND == 1)
        asm volatile("v_add_f64 %0, %0, %1" : "+v"(f & 1 ? y1 : y0) : "v"(y0));
      else if constexpr (KIND == 2)
        asm volatile("v_cvt_f32_f64 %0, %1" : "=v"(f & 1 ? x3 : x2) : "v"(y1));
      else if constexpr (KIND == 3)
        asm volatile("global_store_dword %0, %1, off" : : "v"(dst), "v"(x0) : "memory");
      else if constexpr (KIND == 4)
        asm volatile("v_accvgpr_write_b32 %0, %1" : "=a"(f & 1 ? g1 : g0) : "v"(x0));
      else if constexpr (KIND == 5)
        asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(f & 1 ? x3 : x2) : "a"(g0));
      else if constexpr (KIND == 6)
        asm volatile("v_cvt_f64_f32 %0, %1" : "=v"(f & 1 ? y1 : y0) : "v"(x0));
      else if constexpr (KIND == 7)
        asm volatile("v_cndmask_b32 %0, %1, %2, vcc" : "=v"(f & 1 ? x3 : x2) : "v"(x0), "v"(x1) : "vcc");
      else if constexpr (KIND == 8)
        asm volatile("s_add_u32 %0, %0, %1" : "+s"(f & 1 ? k1 : k0) : "s"(rounds) : "scc");
      else
        asm volatile("s_mul_i32 %0, %0, %1" : "+s"(f & 1 ? k1 : k0) : "s"(rounds));
    }
  };
  unsigned long long t0 = __builtin_amdgcn_s_memtime();
  for (int r = 0; r < rounds; ++r) {
    MF(c0); fill();
    MF(c1); fill();
    MF(c2); fill();
    MF(c3); fill();
    MF(c4); fill();
    MF(c5); fill();
  }
  asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 7\n\ts_nop 7" ::);
  const d4 s = c0 + c1 + c2 + c3 + c4 + c5;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  unsigned long long t1 = __builtin_amdgcn_s_memtime();
  if (threadIdx.x == 0) out[0] = t1 - t0;
  asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(x0) : "a"(g1));
  sink[64 + threadIdx.x] = float(s.x + s.y + s.z + s.w) + x0 + x1 + x2 + x3 + float(y0 + y1) + float(k0 + k1);
}

// after each MFMA, one v_add_f64 that reads the result of the MFMA issued K MFMAs earlier (K = 0: the one just issued)
template <int K>
__global__ void k_readback(unsigned long long* out, float* sink, int rounds) {
  d4 c[6];
#pragma unroll
  for (int j = 0; j < 6; ++j) c[j] = d4{0, 0, 0, 0};
  const double a = threadIdx.x * 1e-3, b = 1.0 + threadIdx.x * 1e-4;
  double y[6] = {0, 0, 0, 0, 0, 0};
  unsigned long long t0 = __builtin_amdgcn_s_memtime();
  for (int r = 0; r < rounds; ++r) {
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      c[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c[j], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      y[j] = y[j] + c[(j + 6 - K) % 6][0];
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  unsigned long long t1 = __builtin_amdgcn_s_memtime();
  if (threadIdx.x == 0) out[0] = t1 - t0;
  sink[64 + threadIdx.x] = float(y[0] + y[1] + y[2] + y[3] + y[4] + y[5]);
}

template <int K>
void run_readback(unsigned long long* d_out, float* sink, int rounds) {
  unsigned long long h = 0;
  hipLaunchKernelGGL((k_readback<K>), dim3(1), dim3(64), 0, 0, d_out, sink, rounds);  // warm
  hipLaunchKernelGGL((k_readback<K>), dim3(1), dim3(64), 0, 0, d_out, sink, rounds);
  hipMemcpy(&h, d_out, 8, hipMemcpyDeviceToHost);
  printf("add_f64 of the result %d MFMAs back  clocks per MFMA %.1f\n", K, double(h) / (6.0 * rounds));
}

template <int KIND, int F>
void run(const char* name, unsigned long long* d_out, float* sink, int rounds) {
  unsigned long long h = 0;
  hipLaunchKernelGGL((k_overlap<KIND, F>), dim3(1), dim3(64), 0, 0, d_out, sink, rounds);  // warm
  hipLaunchKernelGGL((k_overlap<KIND, F>), dim3(1), dim3(64), 0, 0, d_out, sink, rounds);
  hipMemcpy(&h, d_out, 8, hipMemcpyDeviceToHost);
  printf("%-10s F=%d  clocks per MFMA %.1f\n", name, F, double(h) / (6.0 * rounds));
}

int main() {
  unsigned long long* d_out;
  float* sink;
  hipMalloc(&d_out, 64);
  hipMalloc(&sink, 4096);
  const int rounds = 2000;
  run<0, 0>("none", d_out, sink, rounds);
  run<0, 4>("add_f32", d_out, sink, rounds);
  run<0, 8>("add_f32", d_out, sink, rounds);
  run<0, 16>("add_f32", d_out, sink, rounds);
  run<1, 4>("add_f64", d_out, sink, rounds);
  run<1, 8>("add_f64", d_out, sink, rounds);
  run<2, 4>("cvt_f32_f64", d_out, sink, rounds);
  run<2, 8>("cvt_f32_f64", d_out, sink, rounds);
  run<3, 1>("store", d_out, sink, rounds);
  run<3, 2>("store", d_out, sink, rounds);
  run<4, 4>("acc_write", d_out, sink, rounds);
  run<4, 8>("acc_write", d_out, sink, rounds);
  run<5, 4>("acc_read", d_out, sink, rounds);
  run<5, 8>("acc_read", d_out, sink, rounds);
  run<6, 4>("cvt_f64_f32", d_out, sink, rounds);
  run<6, 8>("cvt_f64_f32", d_out, sink, rounds);
  run<7, 4>("cndmask", d_out, sink, rounds);
  run<7, 8>("cndmask", d_out, sink, rounds);
  run<8, 4>("s_add_u32", d_out, sink, rounds);
  run<8, 8>("s_add_u32", d_out, sink, rounds);
  run<9, 4>("s_mul_i32", d_out, sink, rounds);
  run<9, 8>("s_mul_i32", d_out, sink, rounds);
  run_readback<0>(d_out, sink, rounds);
  run_readback<1>(d_out, sink, rounds);
  run_readback<2>(d_out, sink, rounds);
  run_readback<3>(d_out, sink, rounds);
  run_readback<5>(d_out, sink, rounds);
  hipDeviceSynchronize();
  return 0;
}
