// Weight-only e4m3 GEMM on gfx950,
//   y[M, N] bf16 = x[M, K] bf16 . (codes[N, K] e4m3)^T * scale[N] (+ bias[N])
// with any M >= 1 and N >= 1, K % 64 == 0; x rows x_rs elements apart, codes
// contiguous, one fp32 scale per output row (torch_ref.weight_quantize): what
// linear_w8.hip computes, for more than its 64 rows. gemm_wq.h has the tile,
// the staging of x, the pipeline, the split of K and the grid; what this
// format decides:
//   - a step is 64 k. A lane loads 16 bytes = 16 consecutive k of row j of
//     each of its four tiles, two steps per slice, 8 loads per lane and set;
//   - e4m3 -> bf16 is exact (quant_formats.h), and the row scale multiplies
//     the finished sum in `finish`. The 16 codes of a load are the B operands
//     of two MFMAs; slot (g, e) of the first is k = 16 g + e and of the second
//     k = 16 g + 8 + e, as in linear_w8.hip, and the A fragments are the two
//     16-byte halves of 32 consecutive bytes of an x row in LDS. Each of them
//     feeds the four tiles: 8 fragment reads and 32 MFMAs a step.

// linear_skinny.h says why the attribute opens before the includes. The host
// pass does not know the feature, hence the guard.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(                                      \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

#include "common.h"
#include "kernels.h"
#include "gemm_wq.h"
#include "quant_formats.h"

namespace {

using namespace wq;

struct W8 {
  using Scale = float;
  using Finish = e4m3::Finish;
  static constexpr int kStep = 64;
  struct Frag { uint4 w[kTiles]; };
  struct Ptr { const u8* p[kTiles]; };

  static ACCO_DEV Ptr ptrs(const u8* codes, const float*,
                           const long long (&row)[kTiles], int K, int g) {
    Ptr wp;
#pragma unroll
    for (int t = 0; t < kTiles; ++t) wp.p[t] = codes + row[t] * K + 16 * g;
    return wp;
  }

  static ACCO_DEV void load(Frag& f, const Ptr& wp, int k) {
#pragma unroll
    for (int t = 0; t < kTiles; ++t)
      f.w[t] = *reinterpret_cast<const uint4*>(wp.p[t] + k);
  }

  static ACCO_DEV void mma(const Frag& f, const u16* xa, int g,
                           f32x4 (&acc)[kTiles][MT]) {
    short8 blo[kTiles], bhi[kTiles];
#pragma unroll
    for (int t = 0; t < kTiles; ++t)
      e4m3::codes_to_bf16(f.w[t], blo[t], bhi[t]);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const u16* xp = xa + mt * 16 * LS + 16 * g;
      const short8 alo = *reinterpret_cast<const short8*>(xp);
      const short8 ahi = *reinterpret_cast<const short8*>(xp + 8);
#pragma unroll
      for (int t = 0; t < kTiles; ++t)
        acc[t][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            alo, blo[t], acc[t][mt], 0, 0, 0);
#pragma unroll
      for (int t = 0; t < kTiles; ++t)
        acc[t][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            ahi, bhi[t], acc[t][mt], 0, 0, 0);
    }
  }
};

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

}  // namespace

extern "C" void acco_gemm_w8_grid(int M, int N, int K, int* m_blocks,
                                  int* n_blocks, int* n_split, int* k_chunk) {
  const Grid gr = gemm_grid(M, N, K);
  *m_blocks = gr.m_blocks, *n_blocks = gr.n_blocks;
  *n_split = gr.n_split, *k_chunk = gr.k_chunk;
}

extern "C" void acco_gemm_w8(const void* x, const void* codes,
                             const float* scale, const void* bias, void* y,
                             float* workspace, int M, int N, int K,
                             long long x_rs, hipStream_t stream) {
  launch<W8>(e4m3::Finish{scale, (const u16*)bias}, x, codes, scale, y,
             workspace, M, N, K, x_rs, stream);
}
