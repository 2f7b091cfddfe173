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
// What was chosen and why (linear_w8.hip is the skeleton this started from;
// RESULTS.md says where that one falls short):
//   - one load is one block. A workgroup of four waves owns 128 weight rows
//     and one K chunk, a wave two tiles of 16 rows. K is walked in super-steps
//     of 512. Lane (j, g) = (lane % 16, lane / 16) owns, of row j of each
//     tile, the four consecutive scale blocks [128 g, 128 g + 128) of the
//     super-step: 64 contiguous code bytes, four 16-byte loads of one block
//     each, and its four scale bytes are one aligned dword load (hence
//     K % 128). Every code byte and every scale byte is read from global
//     memory exactly once, straight into registers, never through LDS;
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
//   - the A operand. x is staged in LDS KT = 1024 (M <= 16) or 512 columns
//     at a time, 32 KB per 16 rows at most; columns past the chunk's end up
//     to the next multiple of 512 and rows >= M are zeros, rows >= M are never
//     loaded. Per byte of codes a wave reads 4 MT / 2 bytes of x from LDS,
//     twice linear_w8's ratio, each fragment serving both weight tiles of the
//     wave. Rows are padded by 16 bytes, so the 16 lanes of one g, which read
//     the same column of 16 rows in one b128 pass, fall into the 16 distinct
//     16-byte bank groups;
//   - M > 16 takes MT = 2 .. 4 accumulator tiles against the same weight
//     fragment, so the weights are still read once. At MT = 4 a super-step of
//     a wave is 128 MFMAs against 8 KB of codes and 64 KB of LDS reads: that
//     shape is bound by the MFMA and LDS rates, not by HBM.
// K is split across gridDim.y workgroups, split i owning k in [i * k_chunk,
// (i + 1) * k_chunk); every split stores its fp32 partial [M, N] by ordinary
// stores and a second kernel sums them in split order, adds the bias and
// rounds once. With one split the kernel's own tail does that. No atomics and
// no inter-workgroup hand-off: the same bits on every run.
//
// Guesses that nobody has measured: the grid's target of two workgroups per
// CU (512); the cap of 64 splits; the limit K / (32 M) on the splits, which
// keeps the partials' traffic (8 M N n_split bytes) under half the code bytes
// (N K / 2); the 1 to 2 us of loaded latency behind the prefetch depth; that
// 64 contiguous bytes per lane (half a cache line, the other half being the
// next lane group's) cost no more than linear_w8's 64 bytes per row per
// instruction; that a b128 LDS read is served 16 consecutive lanes at a time;
// KT. Sizes tried so far: the tests and benchmarks/linear_w4_micro.py.

// Built without the packed fp32 VALU ops, exactly as linear_w8.hip is (see
// there for why the attribute opens before the includes and why the kernels
// read their ids by builtin).
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(                                      \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

#include "common.h"
#include "kernels.h"

namespace {

using u16 = unsigned short;
using u8 = unsigned char;
using short8 = __attribute__((ext_vector_type(8))) short;
using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kTiles = 2;                       // 16-row weight tiles per wave
constexpr int kRows = kWaves * kTiles * 16;     // weight rows per workgroup
constexpr int kSuper = 512;                     // k per super-step
constexpr int kPad = 8;     // LDS row pad: 16 rows of a b128 read, 16 bank groups

// the codes and scales of one super-step of a lane: per tile four blocks of 32
// codes and their four scale bytes
struct Frag {
  uint4 c[kTiles][4];
  unsigned s[kTiles];
};

// 8 codes (one dword, k ascending from the low nibble) times 2^(s - 127) ->
// 8 bf16, the B fragment of one MFMA; `scale` is s << 23 read as fp32
ACCO_DEV short8 codes_to_bf16(unsigned dw, float scale) {
  union { decltype(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(0u, 1.f, 0)) v;
          unsigned u; } p[4];
  p[0].v = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(dw, scale, 0);
  p[1].v = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(dw, scale, 1);
  p[2].v = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(dw, scale, 2);
  p[3].v = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(dw, scale, 3);
  short8 out;
  unsigned* o = reinterpret_cast<unsigned*>(&out);
#pragma unroll
  for (int i = 0; i < 4; ++i) o[i] = p[i].u;
  return out;
}

// the one place a finished dot product becomes an output element
ACCO_DEV u16 finish(float dot, const u16* __restrict__ bias, int n) {
  const float b = bias != nullptr ? bf16_to_f32(bias[n]) : 0.f;
  return f32_to_bf16(dot + b);
}

// grid (ceil(N / 128), n_split); part: fp32 [n_split, M, N], unused with one
// split, which stores y instead
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

  const int tid = __builtin_amdgcn_workitem_id_x();
  const int lane = tid % kWave, wave = tid / kWave;
  const int j = lane % 16, g = lane / 16;
  const int blk = __builtin_amdgcn_workgroup_id_x();
  const int split = __builtin_amdgcn_workgroup_id_y();
  const int k0 = split * k_chunk, k1 = min(K, k0 + k_chunk);

  // A lane of a tile that passes N points at row N - 1: rows >= N are never
  // loaded, and a column of the product depends on its own weight row only,
  // so what such a lane accumulates touches no live column and is not stored.
  int n[kTiles];
  const u8* cp[kTiles];
  const u8* sp[kTiles];
#pragma unroll
  for (int t = 0; t < kTiles; ++t) {
    n[t] = blk * kRows + (wave * kTiles + t) * 16 + j;
    const long long row = min(n[t], N - 1);
    cp[t] = codes + row * (K / 2) + (k0 + 128 * g) / 2;
    sp[t] = scales + row * (K / 32) + (k0 + 128 * g) / 32;
  }

  // rows >= M of x are zeros, written once; the staging below never touches
  // them, and its second barrier orders them before the first read
  for (int i = M * (LS / 8) + tid; i < MP * (LS / 8); i += kThreads)
    reinterpret_cast<uint4*>(xs)[i] = make_uint4(0u, 0u, 0u, 0u);

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
      const int live = min(KT, k1 - kt);                  // columns below k1
      const int per_row = (live + kSuper - 1) / kSuper * kSuper / 8;
      __syncthreads();                // the previous slice has been read
      for (int i = tid; i < M * per_row; i += kThreads) {
        const int m = i / per_row, c = (i % per_row) * 8;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (c < live)
          v = *reinterpret_cast<const uint4*>(x + (long long)m * x_rs + kt + c);
        *reinterpret_cast<uint4*>(xs + m * LS + c) = v;
      }
      __syncthreads();
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

  // C layout: the lane holds weight row j of its tile (n[t]) for the x rows
  // 16 mt + 4 g + r; 16 lanes store 16 adjacent n of one x row
#pragma unroll
  for (int t = 0; t < kTiles; ++t) {
    if (n[t] >= N) continue;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = mt * 16 + 4 * g + r;
        if (m >= M) continue;
        if (n_split == 1)
          y[(long long)m * N + n[t]] = finish(acc[t][mt][r], bias, n[t]);
        else
          part[((long long)split * M + m) * N + n[t]] = acc[t][mt][r];
      }
  }
}

// y[m, n] from the partials [n_split, M, N], summed in split order; one
// thread per element, adjacent threads adjacent n
__global__ __launch_bounds__(kThreads)
void linear_w4_combine_kernel(const float* __restrict__ part,
                              const u16* __restrict__ bias,
                              u16* __restrict__ y, long long MN, int N,
                              int n_split) {
  const long long i = (long long)__builtin_amdgcn_workgroup_id_x() * kThreads +
                      __builtin_amdgcn_workitem_id_x();
  if (i >= MN) return;
  float dot = 0.f;
  for (int s = 0; s < n_split; ++s) dot += part[s * MN + i];
  y[i] = finish(dot, bias, (int)(i % N));
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

}  // namespace

extern "C" void acco_linear_w4_grid(int M, int N, int K, int* n_split,
                                    int* k_chunk) {
  const long long n_blk = ((long long)N + kRows - 1) / kRows;
  const long long steps = ((long long)K + kSuper - 1) / kSuper;
  long long n = 512 / (n_blk > 0 ? n_blk : 1);
  const long long by_part = (long long)K / (32LL * (M > 0 ? M : 1));
  if (n > by_part) n = by_part;
  if (n > 64) n = 64;
  if (n > steps) n = steps;
  if (n < 1) n = 1;
  // whole super-steps per split, no empty split; the last one may be short
  // and may end inside a super-step
  const long long per = (steps + n - 1) / n > 0 ? (steps + n - 1) / n : 1;
  *k_chunk = (int)(per * kSuper);
  *n_split = (int)((steps + per - 1) / per > 0 ? (steps + per - 1) / per : 1);
}

extern "C" void acco_linear_w4(const void* x, const void* codes,
                               const void* scales, const void* bias, void* y,
                               float* workspace, int M, int N, int K,
                               long long x_rs, hipStream_t stream) {
  int n_split, k_chunk;
  acco_linear_w4_grid(M, N, K, &n_split, &k_chunk);
  const dim3 grid((N + kRows - 1) / kRows, n_split);
#define ACCO_W4_MT(MT)                                                       \
  hipLaunchKernelGGL((linear_w4_kernel<MT>), grid, dim3(kThreads), 0,        \
                     stream, (const u16*)x, (const u8*)codes,                \
                     (const u8*)scales, (const u16*)bias, (u16*)y,           \
                     workspace, M, N, K, k_chunk, n_split, x_rs)
  switch ((M + 15) / 16) {      // the binding admits 1 <= M <= 64 only
    case 1: ACCO_W4_MT(1); break;
    case 2: ACCO_W4_MT(2); break;
    case 3: ACCO_W4_MT(3); break;
    case 4: ACCO_W4_MT(4); break;
    default: return;
  }
#undef ACCO_W4_MT
  if (n_split > 1) {
    const long long MN = (long long)M * N;
    hipLaunchKernelGGL(linear_w4_combine_kernel,
                       dim3((unsigned)((MN + kThreads - 1) / kThreads)),
                       dim3(kThreads), 0, stream, workspace,
                       (const u16*)bias, (u16*)y, MN, N, n_split);
  }
}
