// Weight-only MXFP4 linear for decode on gfx950: a handful of activation rows
// against a whole 4-bit weight matrix,
//   y[M, N] bf16 = x[M, K] bf16 . dequant(codes, scales)^T (+ bias[N])
// with 1 <= M <= 64, K % 128 == 0, any N >= 1; x rows x_rs elements apart.
// codes [N, K / 2] bytes hold two e2m1 values each (k = 2 i in the low nibble
// of byte i), scales [N, K / 32] bytes one e8m0 power of two per 32
// consecutive k (torch_ref.weight_quantize_mxfp4). The scale differs per 32
// k, so unlike linear_w8's row scale it cannot wait for the finished sum: it
// rides in with the convert.
//
// What was chosen and why (linear_skinny.h has the workgroup, the staging of
// x, the split of K and the grid; RESULTS.md says where linear_w8.hip, which
// this started from, falls short):
//   - one load is one block. K is walked in super-steps of 512. Lane (j, g)
//     owns, of row j of each tile, the four consecutive scale blocks
//     [128 g, 128 g + 128) of the super-step: 64 contiguous code bytes, four
//     16-byte loads of one block each, and its four scale bytes are one
//     aligned dword load (hence K % 128). Every code byte and every scale
//     byte is read from global memory exactly once, straight into registers;
//   - e2m1 x 2^(s - 127) -> bf16 by v_cvt_scalef32_pk_bf16_fp4, in registers;
//     the scale operand is the byte shifted into an fp32 exponent. The result
//     is the exact weight (a two-bit significand times a power of two). Dword
//     i of a block's load is 8 codes = the B fragment of one
//     v_mfma_f32_16x16x32_bf16, so a load feeds four MFMAs. The MFMA's k
//     order is free as long as both operands agree: slot (g, e) of MFMA i of
//     block b is k = 128 g + 32 b + 8 i + e, and the A operand is the 16
//     bytes of an x row at that column. Exact products, fp32 accumulation,
//     bias added in fp32, one rounding to bf16;
//   - latency. Two register sets of a whole super-step (8 loads of 16 bytes
//     per lane each) take turns: while one is multiplied the other is in
//     flight, and it is reloaded for two super-steps on as soon as it is
//     consumed, so 8 to 16 loads per lane are in flight, 32 to 64 KB per
//     workgroup against linear_w8's 16 KB. At the grid's two workgroups per
//     CU that is 64 to 128 KB per CU; 8 TB/s over 256 CUs is 31 KB per CU per
//     microsecond of latency, so this covers 2 to 4 us. The main loop has no
//     branch around a load; only a chunk's first two and last few super-steps
//     take the predicated form (lanes whose 128 k lie past the chunk's end
//     load nothing and multiply zero codes). Known from the ISA and not yet
//     dealt with: staging a slice of x waits for every load issued before it
//     (s_waitcnt vmcnt(0)), the prefetched set included, so each slice
//     boundary is one exposed round trip with both sets in flight;
//   - the A operand. x is staged KT = 1024 (M <= 16) or 512 columns at a
//     time, 32 KB per 16 rows at most; columns past the chunk's end up to the
//     next multiple of 512 are zeros. Per byte of codes a wave reads 4 MT / 2
//     bytes of x from LDS, twice linear_w8's ratio;
//   - at MT = 4 a super-step of a wave is 128 MFMAs against 8 KB of codes and
//     64 KB of LDS reads: that shape is bound by the MFMA and LDS rates, not
//     by HBM.
// The grid: whole super-steps per split (the last one may end inside a
// super-step), at most K / (32 M) splits (the code bytes are N K / 2).
//
// Guesses that nobody has measured, beyond the grid's: the 1 to 2 us of
// loaded latency behind the prefetch depth; that 64 contiguous bytes per lane
// (half a cache line, the other half being the next lane group's) cost no
// more than linear_w8's 64 bytes per row per instruction; that a b128 LDS
// read is served 16 consecutive lanes at a time; KT.

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

constexpr int kSuper = 512;                     // k per super-step

// the codes and scales of one super-step of a lane: per tile four blocks of 32
// codes and their four scale bytes
struct Frag {
  uint4 c[kTiles][4];
  unsigned s[kTiles];
};

using mxfp4::codes_to_bf16;            // quant_formats.h
using mxfp4::Finish;

template <int MT>
__global__ __launch_bounds__(kThreads)
void linear_w4_kernel(const u16* __restrict__ x, const u8* __restrict__ codes,
                      const u8* __restrict__ scales,
                      const u16* __restrict__ bias, u16* __restrict__ y,
                      float* __restrict__ part, int M, int N, int K,
                      int k_chunk, int n_split, long long x_rs) {
  constexpr int KT = MT == 1 ? 1024 : 512;    // x columns staged at a time
  constexpr int LS = KT + kPad;       // LDS row stride, elements
  constexpr int MP = 16 * MT;
  __shared__ __attribute__((aligned(16))) u16 xs[MP * LS];

  const Lane c = lane_coords(N, K, k_chunk);
  const int tid = c.tid, j = c.j, g = c.g, k0 = c.k0, k1 = c.k1;
  const u8* cp[kTiles];
  const u8* sp[kTiles];
#pragma unroll
  for (int t = 0; t < kTiles; ++t) {
    const long long row = c.row[t];
    cp[t] = codes + row * (K / 2) + (k0 + 128 * g) / 2;
    sp[t] = scales + row * (K / 32) + (k0 + 128 * g) / 32;
  }

  zero_pad_rows(xs, M, MP, LS, tid);
  f32x4 acc[kTiles][MT];
#pragma unroll
  for (int t = 0; t < kTiles; ++t)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[t][mt] = f32x4{0.f, 0.f, 0.f, 0.f};

  // super-step s is the columns [k0 + 512 s, k0 + 512 s + 512); the first
  // n_full of them lie below k1 whole, and the last of n_steps may hold only
  // 128, 256 or 384 columns: the blocks of the lane groups g below that
  const int n_full = (k1 - k0) / kSuper;
  const int n_steps = (k1 - k0 + kSuper - 1) / kSuper;

  auto load_all = [&](Frag& w, int s) {
#pragma unroll
    for (int t = 0; t < kTiles; ++t) {
#pragma unroll
      for (int b = 0; b < 4; ++b)
        w.c[t][b] = *reinterpret_cast<const uint4*>(
            cp[t] + s * (kSuper / 2) + 16 * b);
      w.s[t] = *reinterpret_cast<const unsigned*>(sp[t] + s * (kSuper / 32));
    }
  };
  // a lane whose 128 columns start at or past k1 loads nothing: zero codes
  // under scale byte 127 are zeros, against the zeros staged in x
  auto load = [&](Frag& w, int s) {
    if (k0 + s * kSuper + 128 * g < k1) {
      load_all(w, s);
    } else {
#pragma unroll
      for (int t = 0; t < kTiles; ++t) {
#pragma unroll
        for (int b = 0; b < 4; ++b) w.c[t][b] = make_uint4(0u, 0u, 0u, 0u);
        w.s[t] = 0x7f7f7f7fu;
      }
    }
  };

  auto step = [&](const Frag& w, int s) {
    const int kk = s * kSuper % KT;
    if (kk == 0) {                    // the next slice of x
      const int kt = k0 + s * kSuper;
      const int live = min(KT, k1 - kt);                // columns below k1
      stage_x<true>(xs, x, x_rs, M, kt, live,
                    (live + kSuper - 1) / kSuper * kSuper, LS, tid);
    }
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      float sc[kTiles];
#pragma unroll
      for (int t = 0; t < kTiles; ++t)
        sc[t] = __uint_as_float(((w.s[t] >> (8 * b)) & 0xffu) << 23);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        short8 bf[kTiles];
#pragma unroll
        for (int t = 0; t < kTiles; ++t)
          bf[t] = codes_to_bf16(
              reinterpret_cast<const unsigned*>(&w.c[t][b])[i], sc[t]);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          const short8 a = *reinterpret_cast<const short8*>(
              xs + (mt * 16 + j) * LS + kk + 128 * g + 32 * b + 8 * i);
#pragma unroll
          for (int t = 0; t < kTiles; ++t)
            acc[t][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                a, bf[t], acc[t][mt], 0, 0, 0);
        }
      }
    }
  };

  // At the top of the loops wa holds super-step s and wb s + 1 (landed or in
  // flight); a set is reloaded for two super-steps on right after its use.
  Frag wa, wb;
  load(wa, 0);
  if (n_steps > 1) load(wb, 1);
  int s = 0;
  for (; s + 3 < n_full; s += 2) {    // no branch around a load in here
    step(wa, s);
    load_all(wa, s + 2);
    step(wb, s + 1);
    load_all(wb, s + 3);
  }
  for (; s < n_steps; s += 2) {       // the last few super-steps
    step(wa, s);
    if (s + 2 < n_steps) load(wa, s + 2);
    if (s + 1 < n_steps) step(wb, s + 1);
    if (s + 3 < n_steps) load(wb, s + 3);
  }

  store_tiles(acc, c.n, g, M, N, n_split, c.split, y, part, Finish{bias});
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

}  // namespace

extern "C" void acco_linear_w4_grid(int M, int N, int K, int* n_split,
                                    int* k_chunk) {
  skinny_grid(M, N, K, kSuper, 32, n_split, k_chunk);
}

extern "C" void acco_linear_w4(const void* x, const void* codes,
                               const void* scales, const void* bias, void* y,
                               float* workspace, int M, int N, int K,
                               long long x_rs, hipStream_t stream) {
  const Kernel<u8> by_mt[4] = {linear_w4_kernel<1>, linear_w4_kernel<2>,
                               linear_w4_kernel<3>, linear_w4_kernel<4>};
  launch(by_mt, kSuper, 32, Finish{(const u16*)bias}, x, codes,
         (const u8*)scales, bias, y, workspace, M, N, K, x_rs, stream);
}
