// Shared skeleton of the weight-only decode linears (linear_w8.hip,
// linear_w4.hip): a handful of activation rows against a whole quantised
// weight matrix,
//   y[M, N] bf16 = x[M, K] bf16 . W[N, K]^T (+ bias[N]),  1 <= M <= 64,
// x rows x_rs elements apart, any N >= 1. Each file keeps what its format
// decides: the convert, the fragment a lane loads, the k mapping and MFMA
// order of a step, the prefetch pipeline, KT and how a finished dot product
// becomes an output element (`finish`). Everything else is here, once:
//   - a workgroup of four waves owns 128 weight rows and one K chunk; a wave
//     owns two tiles of 16 rows, lane (j, g) = (lane % 16, lane / 16) row j
//     of each. The codes go from global memory straight to registers, every
//     byte exactly once and never through LDS. Weight rows >= N are neither
//     loaded nor stored;
//   - M > 16 takes MT = 2 .. 4 accumulator tiles against the same weight
//     fragment, so the weights are still read once;
//   - x is staged in LDS KT columns of the chunk at a time, once per
//     workgroup, and each A fragment read from LDS serves both weight tiles
//     of the wave. Rows are padded by 16 bytes, so the 16 lanes of one g,
//     which read the same column of 16 rows in one b128 pass, fall into the
//     16 distinct 16-byte bank groups. Rows >= M of the LDS tile are zeroed
//     once and never loaded;
//   - K is split across gridDim.y workgroups, split i owning k in
//     [i * k_chunk, (i + 1) * k_chunk); every split stores its fp32 partial
//     [M, N] by ordinary stores and a second kernel sums them in split order
//     and applies `finish` once. With one split the kernel's own tail does
//     that. No atomics and no inter-workgroup hand-off: the same bits on
//     every run.
//
// The grid (skinny_grid) is a guess that nobody has measured: about two
// workgroups per CU (512) over the N / 128 row blocks, at most 64 splits,
// whole steps per split, and at most K / (part_div M) splits so that writing
// and reading the partials (8 M N n_split bytes) stays under half the code
// bytes. Sizes tried so far: the tests and benchmarks/linear_w?_micro.py.
//
// Both files are built without the packed fp32 VALU ops, as
// attention_extend.hip is, and include this header inside that attribute's
// region. The attribute opens before the includes: a function without it
// cannot be inlined into one that has it, and every helper of the HIP headers
// (__syncthreads, min, make_uint4) would stay a call. So this header includes
// nothing but common.h. The device library behind threadIdx / blockIdx /
// gridDim is out of the attribute's reach, so the kernels read their ids by
// builtin and take the split count as an argument.
#pragma once

#include "common.h"

namespace skinny {

using u16 = unsigned short;
using u8 = unsigned char;
using short8 = __attribute__((ext_vector_type(8))) short;
using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kTiles = 2;                       // 16-row weight tiles per wave
constexpr int kRows = kWaves * kTiles * 16;     // weight rows per workgroup
constexpr int kPad = 8;     // LDS row pad: 16 rows of a b128 read, 16 bank groups

// where a thread stands: its chunk [k0, k1) of K and, per tile, its weight
// row n and the row its loads point at
struct Lane {
  int tid, j, g, split, k0, k1;
  int n[kTiles], row[kTiles];
};

// A lane of a tile that passes N points at row N - 1: rows >= N are never
// loaded, and a column of the product depends on its own weight row only,
// so what such a lane accumulates touches no live column and is not stored.
// That keeps the loops free of branches around their loads.
ACCO_DEV Lane lane_coords(int N, int K, int k_chunk) {
  Lane c;
  c.tid = __builtin_amdgcn_workitem_id_x();
  const int lane = c.tid % kWave, wave = c.tid / kWave;
  c.j = lane % 16, c.g = lane / 16;
  const int blk = __builtin_amdgcn_workgroup_id_x();
  c.split = __builtin_amdgcn_workgroup_id_y();
  c.k0 = c.split * k_chunk, c.k1 = min(K, c.k0 + k_chunk);
#pragma unroll
  for (int t = 0; t < kTiles; ++t) {
    c.n[t] = blk * kRows + (wave * kTiles + t) * 16 + c.j;
    c.row[t] = min(c.n[t], N - 1);
  }
  return c;
}

// rows >= M of x [MP, LS] are zeros, written once; stage_x never touches
// them, and its second barrier orders them before the first read
ACCO_DEV void zero_pad_rows(u16* xs, int M, int MP, int LS, int tid) {
  for (int i = M * (LS / 8) + tid; i < MP * (LS / 8); i += kThreads)
    reinterpret_cast<uint4*>(xs)[i] = make_uint4(0u, 0u, 0u, 0u);
}

template <int MT>
ACCO_DEV void zero_acc(f32x4 (&acc)[kTiles][MT]) {
#pragma unroll
  for (int t = 0; t < kTiles; ++t)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[t][mt] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// The next slice of x: columns [kt, kt + live) of its M rows into xs, and with
// kFill zeros in [live, cols); without it cols == live. Multiples of 8 all.
// No __restrict__ here: it changes the ISA of the callers.
template <bool kFill>
ACCO_DEV void stage_x(u16* xs, const u16* x, long long x_rs, int M, int kt,
                      int live, int cols, int LS, int tid) {
  const int per_row = cols / 8;
  __syncthreads();                // the previous slice has been read
  for (int i = tid; i < M * per_row; i += kThreads) {
    const int m = i / per_row, c = (i % per_row) * 8;
    const uint4* src =
        reinterpret_cast<const uint4*>(x + (long long)m * x_rs + kt + c);
    uint4* dst = reinterpret_cast<uint4*>(xs + m * LS + c);
    if constexpr (kFill) {
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (c < live) v = *src;
      *dst = v;
    } else {
      *dst = *src;
    }
  }
  __syncthreads();
}

// C layout: the lane holds weight row j of its tile (n[t]) for the x rows
// 16 mt + 4 g + r; 16 lanes store 16 adjacent n of one x row. part: fp32
// [n_split, M, N], unused with one split, which stores y instead
template <int MT, class Finish>
ACCO_DEV void store_tiles(const f32x4 (&acc)[kTiles][MT],
                          const int (&n)[kTiles], int g, int M, int N,
                          int n_split, int split, u16* y, float* part,
                          const Finish& finish) {
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
          y[(long long)m * N + n[t]] = finish(acc[t][mt][r], n[t]);
        else
          part[((long long)split * M + m) * N + n[t]] = acc[t][mt][r];
      }
  }
}

// y[m, n] from the partials [n_split, M, N], summed in split order; one
// thread per element, adjacent threads adjacent n
template <class Finish>
__global__ __launch_bounds__(kThreads)
void combine_kernel(const float* __restrict__ part, Finish finish,
                    u16* __restrict__ y, long long MN, int N, int n_split) {
  const long long i = (long long)__builtin_amdgcn_workgroup_id_x() * kThreads +
                      __builtin_amdgcn_workitem_id_x();
  if (i >= MN) return;
  float dot = 0.f;
  for (int s = 0; s < n_split; ++s) dot += part[s * MN + i];
  y[i] = finish(dot, (int)(i % N));
}

// (n_split, k_chunk) for steps of `step` k: whole steps per split, no empty
// split; the last one may be short
inline void skinny_grid(int M, int N, int K, int step, int part_div,
                        int* n_split, int* k_chunk) {
  const long long n_blk = ((long long)N + kRows - 1) / kRows;
  const long long steps = ((long long)K + step - 1) / step;
  long long n = 512 / (n_blk > 0 ? n_blk : 1);
  const long long by_part =
      (long long)K / ((long long)part_div * (M > 0 ? M : 1));
  if (n > by_part) n = by_part;
  if (n > 64) n = 64;
  if (n > steps) n = steps;
  if (n < 1) n = 1;
  const long long per = (steps + n - 1) / n > 0 ? (steps + n - 1) / n : 1;
  *k_chunk = (int)(per * step);
  *n_split = (int)((steps + per - 1) / per > 0 ? (steps + per - 1) / per : 1);
}

// a format's main kernel, S its scale type; grid (ceil(N / 128), n_split)
template <class S>
using Kernel = void (*)(const u16* x, const u8* codes, const S* scales,
                        const u16* bias, u16* y, float* part, int M, int N,
                        int K, int k_chunk, int n_split, long long x_rs);

// by_mt[MT - 1] is the kernel for MT = ceil(M / 16) accumulator tiles
template <class S, class Finish>
void launch(const Kernel<S> (&by_mt)[4], int step, int part_div,
            const Finish& finish, const void* x, const void* codes,
            const S* scales, const void* bias, void* y, float* workspace,
            int M, int N, int K, long long x_rs, hipStream_t stream) {
  if (M < 1 || M > 64) return;      // the binding admits 1 <= M <= 64 only
  int n_split, k_chunk;
  skinny_grid(M, N, K, step, part_div, &n_split, &k_chunk);
  hipLaunchKernelGGL(by_mt[(M + 15) / 16 - 1],
                     dim3((N + kRows - 1) / kRows, n_split), dim3(kThreads), 0,
                     stream, (const u16*)x, (const u8*)codes, scales,
                     (const u16*)bias, (u16*)y, workspace, M, N, K, k_chunk,
                     n_split, x_rs);
  if (n_split > 1) {
    const long long MN = (long long)M * N;
    hipLaunchKernelGGL(combine_kernel<Finish>,
                       dim3((unsigned)((MN + kThreads - 1) / kThreads)),
                       dim3(kThreads), 0, stream, workspace, finish, (u16*)y,
                       MN, N, n_split);
  }
}

}  // namespace skinny
