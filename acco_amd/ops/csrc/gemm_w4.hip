// Weight-only MXFP4 GEMM on gfx950,
//   y[M, N] bf16 = x[M, K] bf16 . dequant(codes, scales)^T (+ bias[N])
// with any M >= 1 and N >= 1, K % 128 == 0; x rows x_rs elements apart, codes
// [N, K / 2] bytes of two e2m1 each and scales [N, K / 32] e8m0 bytes
// (torch_ref.weight_quantize_mxfp4): what linear_w4.hip computes, for more
// than its 64 rows. gemm_wq.h has the tile, the staging of x, the pipeline,
// the split of K and the grid; what this format decides:
//   - a step is 128 k = a slice, and one load is one scale block: lane (j, g)
//     loads the 16 code bytes of block g of the step of row j of each of its
//     four tiles, and that block's scale byte. Every code and scale byte is
//     read once per workgroup, straight into registers; a set is 4 loads of
//     16 bytes and 4 of one byte per lane. (linear_w4.hip gives a lane four
//     consecutive blocks and one dword of scales; here the lane groups of a
//     row share a 64-byte run of codes, a step is a quarter of its 512 k, and
//     a set is 20 registers, not 68);
//   - e2m1 x 2^(s - 127) -> bf16 by v_cvt_scalef32_pk_bf16_fp4 in registers
//     (quant_formats.h), exact. Dword i of a load is the B operand of MFMA i
//     of the step: slot (g, e) is k = 32 g + 8 i + e, and the A fragment is
//     the 16 bytes of an x row at that column in LDS, which feeds the four
//     tiles: 16 fragment reads and 64 MFMAs a step.

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

struct W4 {
  using Scale = u8;
  using Finish = mxfp4::Finish;
  static constexpr int kStep = 128;
  struct Frag {
    uint4 c[kTiles];
    unsigned s[kTiles];
  };
  struct Ptr { const u8 *c[kTiles], *s[kTiles]; };

  static ACCO_DEV Ptr ptrs(const u8* codes, const u8* scales,
                           const long long (&row)[kTiles], int K, int g) {
    Ptr wp;
#pragma unroll
    for (int t = 0; t < kTiles; ++t) {
      wp.c[t] = codes + row[t] * (K / 2) + 16 * g;
      wp.s[t] = scales + row[t] * (K / 32) + g;
    }
    return wp;
  }

  static ACCO_DEV void load(Frag& f, const Ptr& wp, int k) {
#pragma unroll
    for (int t = 0; t < kTiles; ++t) {
      f.c[t] = *reinterpret_cast<const uint4*>(wp.c[t] + k / 2);
      f.s[t] = wp.s[t][k / 32];
    }
  }

  static ACCO_DEV void mma(const Frag& f, const u16* xa, int g,
                           f32x4 (&acc)[kTiles][MT]) {
    float sc[kTiles];
#pragma unroll
    for (int t = 0; t < kTiles; ++t) sc[t] = __uint_as_float(f.s[t] << 23);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      short8 bf[kTiles];
#pragma unroll
      for (int t = 0; t < kTiles; ++t)
        bf[t] = mxfp4::codes_to_bf16(
            reinterpret_cast<const unsigned*>(&f.c[t])[i], sc[t]);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const short8 a = *reinterpret_cast<const short8*>(
            xa + mt * 16 * LS + 32 * g + 8 * i);
#pragma unroll
        for (int t = 0; t < kTiles; ++t)
          acc[t][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a, bf[t], acc[t][mt], 0, 0, 0);
      }
    }
  }
};

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

}  // namespace

extern "C" void acco_gemm_w4_grid(int M, int N, int K, int* m_blocks,
                                  int* n_blocks, int* n_split, int* k_chunk) {
  const Grid gr = gemm_grid(M, N, K);
  *m_blocks = gr.m_blocks, *n_blocks = gr.n_blocks;
  *n_split = gr.n_split, *k_chunk = gr.k_chunk;
}

extern "C" void acco_gemm_w4(const void* x, const void* codes,
                             const void* scales, const void* bias, void* y,
                             float* workspace, int M, int N, int K,
                             long long x_rs, hipStream_t stream) {
  launch<W4>(mxfp4::Finish{(const u16*)bias}, x, codes, (const u8*)scales, y,
             workspace, M, N, K, x_rs, stream);
}
