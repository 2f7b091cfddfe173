// Weight-only e4m3 linear for decode on gfx950: a handful of activation rows
// against a whole weight matrix,
//   y[M, N] bf16 = x[M, K] bf16 . (codes[N, K] e4m3)^T * scale[N] (+ bias[N])
// with 1 <= M <= 64, K % 64 == 0, any N >= 1; x rows x_rs elements apart,
// codes contiguous, one fp32 scale per output row (torch_ref.weight_quantize).
// The scale multiplies the finished dot product and never enters the K loop.
//
// Memory-bound on the codes, so the structure follows the bytes:
//   - a workgroup of four waves owns 128 weight rows and one K chunk; a wave
//     owns two tiles of 16 rows. Lane (j, g) = (lane % 16, lane / 16) loads
//     16 bytes = 16 consecutive k of row j of each tile straight from global
//     memory to registers, every weight byte exactly once and never through
//     LDS; the loads run two 64-k steps ahead of their use, so four loads
//     per lane are in flight;
//   - e4m3 -> bf16 is exact: v_cvt_pk_f32_fp8 and the high halves of the
//     fp32 pairs, in registers. The 16 codes of a load feed two
//     v_mfma_f32_16x16x32_bf16 as the B operand (16 weight rows); the MFMA's
//     k order is free as long as both operands agree, so slot (g, e) of the
//     first MFMA is k = 16 g + e and of the second k = 16 g + 8 + e, and the
//     A operand (16 rows of x) is gathered with the same mapping: 32
//     consecutive bytes of an x row. Exact products, fp32 accumulation;
//   - M > 16 takes MT = 2 .. 4 accumulator tiles against the same weight
//     fragment, so the weights are still read once;
//   - x is staged in LDS, about 1024 / MT columns of the chunk at a time (32
//     to 34 KB for every MT), once per workgroup, and each A fragment read from
//     LDS serves both weight tiles of the wave: per 64-k step a workgroup
//     moves 8 KB of codes and 128 M bytes of x (a quarter of the code bytes
//     at M <= 16, as many at M = 64). Rows >= M of the LDS tile are zeroed
//     once and never loaded; weight rows >= N are neither loaded nor stored.
// K is split across gridDim.y workgroups, split i owning k in [i * k_chunk,
// (i + 1) * k_chunk); every split stores its fp32 partial [M, N] by ordinary
// stores and a second kernel sums them in split order, applies scale and bias
// and rounds to bf16 once. With one split the kernel's own tail does that. No
// atomics and no inter-workgroup hand-off: the same bits on every run.
//
// The grid is a guess that nobody has measured: about two workgroups per CU
// (512) over the N / 128 row blocks, at most 64 splits, whole 64-k steps per
// split, and at most K / (16 M) splits so that writing and reading the
// partials (8 M N n_split bytes) stays under half the code bytes (N K).
// Sizes tried so far: the tests and benchmarks/linear_w8_micro.py.

// Built without the packed fp32 VALU ops, as attention_extend.hip is. The
// attribute opens before the includes: a function without it cannot be
// inlined into one that has it, and every helper of the HIP headers
// (__syncthreads, min, make_uint4) would stay a call. The device library
// behind threadIdx / blockIdx / gridDim is out of the attribute's reach, so
// the kernels read their ids by builtin and take the split count as an
// argument. The host pass does not know the feature, hence the guard.
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
constexpr int kStep = 64;                       // k per 16-byte load of a tile
constexpr int kPad = 8;     // LDS row pad: 16 rows of a b128 read, 16 bank groups

// 16 e4m3 codes -> 16 bf16, the B fragments of the two MFMAs of a step. An
// e4m3 value has four significant bits, so the high half of its fp32 is the
// value itself in bf16.
ACCO_DEV void codes_to_bf16(const uint4& raw, short8& lo, short8& hi) {
  const int* w = reinterpret_cast<const int*>(&raw);
  unsigned out[8];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const auto a = __builtin_amdgcn_cvt_pk_f32_fp8(w[i], false);
    const auto b = __builtin_amdgcn_cvt_pk_f32_fp8(w[i], true);
    // v_perm_b32: the high halves of two dwords, the first in the low half
    out[2 * i] = __builtin_amdgcn_perm(__float_as_uint(a[1]),
                                       __float_as_uint(a[0]), 0x07060302u);
    out[2 * i + 1] = __builtin_amdgcn_perm(__float_as_uint(b[1]),
                                           __float_as_uint(b[0]), 0x07060302u);
  }
  unsigned* l = reinterpret_cast<unsigned*>(&lo);
  unsigned* h = reinterpret_cast<unsigned*>(&hi);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    l[i] = out[i];
    h[i] = out[4 + i];
  }
}

// the one place a finished dot product becomes an output element
ACCO_DEV u16 finish(float dot, const float* __restrict__ scale,
                    const u16* __restrict__ bias, int n) {
  const float b = bias != nullptr ? bf16_to_f32(bias[n]) : 0.f;
  return f32_to_bf16(__fmaf_rn(dot, scale[n], b));
}

// grid (ceil(N / 128), n_split); part: fp32 [n_split, M, N], unused with one
// split, which stores y instead
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

  const int tid = __builtin_amdgcn_workitem_id_x();
  const int lane = tid % kWave, wave = tid / kWave;
  const int j = lane % 16, g = lane / 16;
  const int blk = __builtin_amdgcn_workgroup_id_x();
  const int split = __builtin_amdgcn_workgroup_id_y();
  const int k0 = split * k_chunk, k1 = min(K, k0 + k_chunk);

  // A lane of a tile that passes N points at row N - 1: rows >= N are never
  // loaded, and a column of the product depends on its own weight row only,
  // so what such a lane accumulates touches no live column and is not stored.
  // That keeps the loop free of branches around its loads.
  int n[kTiles];
  const u8* wp[kTiles];
#pragma unroll
  for (int t = 0; t < kTiles; ++t) {
    n[t] = blk * kRows + (wave * kTiles + t) * 16 + j;
    wp[t] = codes + (long long)min(n[t], N - 1) * K + k0 + 16 * g;
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

  // step s is the columns [k0 + 64 s, k0 + 64 s + 64), all below k1 <= K
  const int n_steps = (k1 - k0) / kStep;
  auto step = [&](const uint4 (&w)[kTiles], int s) {
    const int kk = s * kStep % KT;
    if (kk == 0) {                    // the next slice of x
      const int kt = k0 + s * kStep;
      const int per_row = min(KT, k1 - kt) / 8;
      __syncthreads();                // the previous slice has been read
      for (int i = tid; i < M * per_row; i += kThreads) {
        const int m = i / per_row, c = (i % per_row) * 8;
        *reinterpret_cast<uint4*>(xs + m * LS + c) =
            *reinterpret_cast<const uint4*>(x + (long long)m * x_rs + kt + c);
      }
      __syncthreads();
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
          y[(long long)m * N + n[t]] = finish(acc[t][mt][r], scale, bias, n[t]);
        else
          part[((long long)split * M + m) * N + n[t]] = acc[t][mt][r];
      }
  }
}

// y[m, n] from the partials [n_split, M, N], summed in split order; one
// thread per element, adjacent threads adjacent n
__global__ __launch_bounds__(kThreads)
void linear_w8_combine_kernel(const float* __restrict__ part,
                              const float* __restrict__ scale,
                              const u16* __restrict__ bias,
                              u16* __restrict__ y, long long MN, int N,
                              int n_split) {
  const long long i = (long long)__builtin_amdgcn_workgroup_id_x() * kThreads +
                      __builtin_amdgcn_workitem_id_x();
  if (i >= MN) return;
  float dot = 0.f;
  for (int s = 0; s < n_split; ++s) dot += part[s * MN + i];
  y[i] = finish(dot, scale, bias, (int)(i % N));
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

}  // namespace

extern "C" void acco_linear_w8_grid(int M, int N, int K, int* n_split,
                                    int* k_chunk) {
  const long long n_blk = ((long long)N + kRows - 1) / kRows;
  const long long steps = K / kStep;
  long long n = 512 / (n_blk > 0 ? n_blk : 1);
  const long long by_part = (long long)K / (16LL * (M > 0 ? M : 1));
  if (n > by_part) n = by_part;
  if (n > 64) n = 64;
  if (n > steps) n = steps;
  if (n < 1) n = 1;
  // whole 64-k steps per split, no empty split; the last one may be short
  const long long per = (steps + n - 1) / n > 0 ? (steps + n - 1) / n : 1;
  *k_chunk = (int)(per * kStep);
  *n_split = (int)((steps + per - 1) / per > 0 ? (steps + per - 1) / per : 1);
}

extern "C" void acco_linear_w8(const void* x, const void* codes,
                               const float* scale, const void* bias, void* y,
                               float* workspace, int M, int N, int K,
                               long long x_rs, hipStream_t stream) {
  int n_split, k_chunk;
  acco_linear_w8_grid(M, N, K, &n_split, &k_chunk);
  const dim3 grid((N + kRows - 1) / kRows, n_split);
#define ACCO_W8_MT(MT)                                                       \
  hipLaunchKernelGGL((linear_w8_kernel<MT>), grid, dim3(kThreads), 0,        \
                     stream, (const u16*)x, (const u8*)codes, scale,         \
                     (const u16*)bias, (u16*)y, workspace, M, N, K, k_chunk, \
                     n_split, x_rs)
  switch ((M + 15) / 16) {      // the binding admits 1 <= M <= 64 only
    case 1: ACCO_W8_MT(1); break;
    case 2: ACCO_W8_MT(2); break;
    case 3: ACCO_W8_MT(3); break;
    case 4: ACCO_W8_MT(4); break;
    default: return;
  }
#undef ACCO_W8_MT
  if (n_split > 1) {
    const long long MN = (long long)M * N;
    hipLaunchKernelGGL(linear_w8_combine_kernel,
                       dim3((unsigned)((MN + kThreads - 1) / kThreads)),
                       dim3(kThreads), 0, stream, workspace, scale,
                       (const u16*)bias, (u16*)y, MN, N, n_split);
  }
}
