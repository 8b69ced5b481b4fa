// k_bsample: a beta-iteration's new samples in large launches, one wave per
// candidate walking all six sample tiles (betacem_sample.hpp).
//
// A translation unit of its own for its code generation (Makefile:
// KERNEL_FLAGS of this object).  The wave runs alone on its SIMD, and its VALU instructions do
// not run in the shadow of its fp64 MFMAs (tools/mfma_overlap.hip), so every
// VGPR <-> AccVGPR move costs time.  S and X are MFMA results that the VALU
// reads (St = Sp + S, T's selects) and Y is converted to fp32 before its
// store: with the MFMA C/D operands in arch VGPRs none of them is shuttled.
// k_bsample_chunks and k_bcem_small keep the default AccVGPR form, which suits
// their single tile per wave.
#include "betacem_sample.hpp"

namespace mpcmmd {

namespace {

template <int TPW>
__global__ __launch_bounds__(64 * sample_waves<TPW>()) void k_bsample(Params p, int tb) {
  static_assert(TPW == kSampleTiles, "the one-wave walker");
  const int b = p.b0 + blockIdx.x, M = p.M, Pp = pos_pad(M);
  const int lane = tidx() & 63;
  const int r = lane & 15, h = lane >> 4;
  MPCMMD_STAMP(p, 0);
  const double* G = p.gen + size_t(b) * Pp * kGenStride;
  const double* gm = p.genm + size_t(b) * Pp;
  const float* z = p.beta_z + size_t(tb - 1) * Pp * kBzCols;
  const int ys = ygen_stride(M);
  float* plane = p.ygen + size_t(b) * kBzCols * ys;
  const float* E = gen_elites(p, tb, b);
  d4 S[TPW], Sp[TPW];
#pragma unroll
  for (int t = 0; t < TPW; ++t) {
    S[t] = Sp[t] = d4{0.0, 0.0, 0.0, 0.0};
    Sp[t][2] = h == 3 ? 1.0 : 0.0;  // row 11 of S_pre: the mean's coefficient
  }
  const int cl = sample_chunk(Pp >> 4);
  const __amdgpu_buffer_rsrc_t yr = ygen_rsrc(plane, ys);
  const int vl = (2 * h * ys + r) * 4, v43 = h == 0 ? vl : kDropOffset;
  // An interior block (walk_blocks: q0 + 15 < M) takes block_store_rows, so
  // the pair loop holds neither block_store's clip nor its 64-bit addresses.
  // The walk's last block, sample_blocks(M) - 1 = M >> 4, always holds M.
  auto store = [&](const d4* Yv, int q0, auto interior) {
    if constexpr (decltype(interior)::value)
      block_store_rows(Yv, yr, q0, ys, vl, v43);
    else
      block_store<TPW>(Yv, plane, q0, M, ys, 0, r, h);
  };
  const SampleRsrc srs = sample_rsrc(G, E, gm, z, M, r, h);
  auto load = [&](SampleBlock<TPW>& q, int q0) { load_block_buf(q, srs, q0); };
  walk_blocks<TPW, false>(0, sample_blocks(M), M, r, h, S, Sp, load, store, [&](int c) {
    if ((c + 2) % cl == 0)
#pragma unroll
      for (int t = 0; t < TPW; ++t) fold_chunk(Sp[t], S[t]);
  });
  MPCMMD_STAMP(p, 1);
}

}  // namespace

void launch_bsample(const Params& p, int tb, hipStream_t s) {
  // one wave per candidate when the launch alone holds >= ~half a wave per
  // SIMD; smaller batches one wave per (candidate, tile, chunk)
  if (p.nb >= 384)
    hipLaunchKernelGGL((k_bsample<kSampleTiles>), dim3(p.nb), dim3(64 * sample_waves<kSampleTiles>()), 0, s, p, tb);
  else
    launch_bsample_chunks(p, tb, s);
}

}  // namespace mpcmmd
