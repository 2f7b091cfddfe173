// Weight-only e4m3 linear for decode on gfx950,
//   y[M, N] bf16 = x[M, K] bf16 . (codes[N, K] e4m3)^T * scale[N] (+ bias[N])
// with 1 <= M <= 64, K % 64 == 0, any N >= 1; x rows x_rs elements apart,
// codes contiguous, one fp32 scale per output row (torch_ref.weight_quantize).
// The scale multiplies the finished dot product and never enters the K loop.
// linear_skinny.h has the workgroup, the staging of x, the split of K and the
// grid; what this format chose:
//   - memory-bound on the codes, so the structure follows the bytes. A lane
//     loads 16 bytes = 16 consecutive k of row j of each tile; the loads run
//     two 64-k steps ahead of their use, so four loads per lane are in
//     flight;
//   - e4m3 -> bf16 is exact: v_cvt_pk_f32_fp8 and the high halves of the
//     fp32 pairs, in registers. The 16 codes of a load feed two
//     v_mfma_f32_16x16x32_bf16 as the B operand (16 weight rows); the MFMA's
//     k order is free as long as both operands agree, so slot (g, e) of the
//     first MFMA is k = 16 g + e and of the second k = 16 g + 8 + e, and the
//     A operand (16 rows of x) is gathered with the same mapping: 32
//     consecutive bytes of an x row. Exact products, fp32 accumulation;
//   - x is staged about 1024 / MT columns of the chunk at a time (32 to 34 KB
//     for every MT): per 64-k step a workgroup moves 8 KB of codes and 128 M
//     bytes of x (a quarter of the code bytes at M <= 16, as many at M = 64).
// The grid: whole 64-k steps per split, at most K / (16 M) splits (the code
// bytes are N K).

// linear_skinny.h says why the attribute opens before the includes. The host
// pass does not know the feature, hence the guard.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(                                      \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

#include "common.h"
#include "kernels.h"
#include "linear_skinny.h"
#include "quant_formats.h"

namespace {

using namespace skinny;

constexpr int kStep = 64;                       // k per 16-byte load of a tile

using e4m3::codes_to_bf16;             // quant_formats.h
using e4m3::Finish;

template <int MT>
__global__ __launch_bounds__(kThreads)
void linear_w8_kernel(const u16* __restrict__ x, const u8* __restrict__ codes,
                      const float* __restrict__ scale,
                      const u16* __restrict__ bias, u16* __restrict__ y,
                      float* __restrict__ part, int M, int N, int K,
                      int k_chunk, int n_split, long long x_rs) {
  constexpr int KT = 1024 / MT / kStep * kStep;   // x columns staged at a time
  constexpr int LS = KT + kPad;       // LDS row stride, elements
  constexpr int MP = 16 * MT;
  __shared__ __attribute__((aligned(16))) u16 xs[MP * LS];

  const Lane c = lane_coords(N, K, k_chunk);
  const int tid = c.tid, j = c.j, g = c.g, k0 = c.k0, k1 = c.k1;
  const u8* wp[kTiles];
#pragma unroll
  for (int t = 0; t < kTiles; ++t) {
    wp[t] = codes + (long long)c.row[t] * K + k0 + 16 * g;
  }

  zero_pad_rows(xs, M, MP, LS, tid);
  f32x4 acc[kTiles][MT];
#pragma unroll
  for (int t = 0; t < kTiles; ++t)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[t][mt] = f32x4{0.f, 0.f, 0.f, 0.f};

  // step s is the columns [k0 + 64 s, k0 + 64 s + 64), all below k1 <= K
  const int n_steps = (k1 - k0) / kStep;
  auto step = [&](const uint4 (&w)[kTiles], int s) {
    const int kk = s * kStep % KT;
    if (kk == 0) {                    // the next slice of x
      const int kt = k0 + s * kStep;
      const int live = min(KT, k1 - kt);
      stage_x<false>(xs, x, x_rs, M, kt, live, live, LS, tid);
    }
    short8 blo[kTiles], bhi[kTiles];
#pragma unroll
    for (int t = 0; t < kTiles; ++t) codes_to_bf16(w[t], blo[t], bhi[t]);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const u16* xp = xs + (mt * 16 + j) * LS + kk + 16 * g;
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
  };
  auto load = [&](uint4 (&w)[kTiles], int s) {
#pragma unroll
    for (int t = 0; t < kTiles; ++t)
      w[t] = *reinterpret_cast<const uint4*>(wp[t] + s * kStep);
  };

  // the loads run two steps ahead of the MFMAs: while step s is computed the
  // loads of s + 1 and s + 2 are in flight, four per lane. Three register
  // sets take turns, so no loaded value is copied (a copy would wait for it).
  // At the top of the loop wa holds step s and wb step s + 1.
  uint4 wa[kTiles], wb[kTiles], wc[kTiles];
  load(wa, 0);
  if (n_steps > 1) load(wb, 1);
  int s = 0;
  for (; s + 4 < n_steps; s += 3) {   // no branch around a load in here
    load(wc, s + 2);
    step(wa, s);
    load(wa, s + 3);
    step(wb, s + 1);
    load(wb, s + 4);
    step(wc, s + 2);
  }
  // the last n_steps - s <= 4 steps
  if (s + 2 < n_steps) load(wc, s + 2);
  if (s < n_steps) step(wa, s);
  if (s + 3 < n_steps) load(wa, s + 3);
  if (s + 1 < n_steps) step(wb, s + 1);
  if (s + 2 < n_steps) step(wc, s + 2);
  if (s + 3 < n_steps) step(wa, s + 3);

  store_tiles(acc, c.n, g, M, N, n_split, c.split, y, part, Finish{scale, bias});
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

}  // namespace

extern "C" void acco_linear_w8_grid(int M, int N, int K, int* n_split,
                                    int* k_chunk) {
  skinny_grid(M, N, K, kStep, 16, n_split, k_chunk);
}

extern "C" void acco_linear_w8(const void* x, const void* codes,
                               const float* scale, const void* bias, void* y,
                               float* workspace, int M, int N, int K,
                               long long x_rs, hipStream_t stream) {
  const Kernel<float> by_mt[4] = {linear_w8_kernel<1>, linear_w8_kernel<2>,
                                  linear_w8_kernel<3>, linear_w8_kernel<4>};
  launch(by_mt, kStep, 16, Finish{scale, (const u16*)bias}, x, codes, scale,
         bias, y, workspace, M, N, K, x_rs, stream);
}
