// Shared skeleton of the tiled weight-only GEMMs (gemm_w8.hip, gemm_w4.hip):
// any number of activation rows against a whole quantised weight matrix,
//   y[M, N] bf16 = x[M, K] bf16 . W[N, K]^T (+ bias[N]),  M >= 1, N >= 1,
// x rows x_rs elements apart, W stored as the skinny linears store it. Each
// format file keeps what its format decides: the convert, the fragment a lane
// loads, the k mapping of a step and `finish` (quant_formats.h). Everything
// else is here, once.
//
// The tile. A workgroup of four waves owns BM = 64 rows of x by BN = 256
// weight rows and walks its K chunk in slices of KT = 128 columns. A wave
// owns four tiles of 16 weight rows and all 64 rows of x: a 64 x 64 wave
// tile, 16 accumulator tiles, 64 accumulator registers. Lane (j, g) =
// (lane % 16, lane / 16) holds row j of each weight tile.
//   - The codes go from global memory straight to registers as codes, 16
//     bytes per lane and tile, every byte once per workgroup, that is once
//     per block of 64 rows of x, and are converted in registers on the way to
//     the B operand. Nothing of size N K is written anywhere; weight rows >= N
//     are neither loaded nor stored (their lanes point at row N - 1, as in
//     linear_skinny.h).
//   - x goes through LDS, and every A fragment read from it (one ds_read_b128,
//     1024 B per wave) feeds the four weight tiles of the wave: four
//     v_mfma_f32_16x16x32_bf16, 256 B of LDS per MFMA against the skinny
//     kernels' 512. A slice of a wave is 16 fragment reads and 64 MFMAs: at
//     16 cycles an MFMA that is 1024 cycles of the SIMD's matrix unit against
//     64 KB of LDS reads of the four waves together, 512 cycles at 128 B per
//     clock, so the tile is bound by the MFMA rate and not by LDS. (Both
//     rates are from the public CDNA4 figures, not measured here.)
//   - Why BM = 64 and not 128: the wave tile and so the LDS bytes per MFMA
//     are the same, 128 rows double the accumulators to 128 registers and
//     halve the tiles that fill the chip at mid M, and what they save, the
//     second read of the codes, is served by L2 when the workgroups that
//     share weight rows run together (below).
//   - LDS layout: two buffers of [64][KT + 8] bf16, 34 KB. Rows are padded by
//     16 bytes as in linear_skinny.h, not XOR-swizzled as in gemm_nt.hip: the
//     swizzle exists for global_load_lds, whose destination is lane-linear;
//     here the slice passes through registers (below), the ds_write address is
//     free, and a pad costs no address arithmetic on either side. The row
//     stride is 272 B = 16 mod 256, so the 16 lanes of one g, which read the
//     same column of 16 rows in one b128 pass, fall into the 16 distinct
//     16-byte groups of the 64 banks. Rows >= M of a tile are stored as zeros
//     and never loaded; columns at or past the chunk's end likewise.
//   - The pipeline. While slice i is multiplied, slice i + 1 is in flight:
//     its x (4 loads of 16 bytes per thread, issued first) and its codes (4
//     or 8 loads per lane, a second register set). After the MFMAs the x
//     registers are written to the other LDS buffer, and one barrier per slice
//     orders that write before its reads and the reads of this buffer before
//     its next write. What the barrier drains: the ds_writes (lgkmcnt), and
//     the x loads, which are the oldest in the queue; the barrier is
//     s_barrier behind an LDS-only fence, so the code loads of slice i + 1
//     issued after them may stay in flight across it, unlike the
//     __syncthreads of the skinny kernels' stage_x, which waits for vmcnt(0).
//     The compiler's output decides whether they do; RESULTS.md records it.
//   - Registers: 64 accumulators, two code sets (2 x 32 for fp8, 2 x 20 for
//     fp4), 16 of staged x, 32 of converted B fragments, 8 of A fragments and
//     the addresses: under 256, so two waves per SIMD, two workgroups per CU
//     (70 KB of its LDS). RESULTS.md has the compiler's own numbers.
//
// The grid (gemm_grid) is a host function of (M, N, K). Tiles alone seldom
// fill 256 CUs at mid M (N = 4096, M = 128 is 32 tiles), so K is split across
// n_split workgroups, split i owning k in [i k_chunk, (i + 1) k_chunk), whole
// slices per split; every split stores its fp32 partial [M, N] by ordinary
// stores and skinny::combine_kernel sums them in split order and applies
// `finish` once. With one split the kernel's own tail does that. No atomics:
// the same bits on every run. The workgroups are numbered with the row block
// fastest and remapped (the bijection of gemm_nt.hip) so that consecutive
// numbers fall on one XCD: the workgroups that share a block of weight rows
// and a K chunk are dispatched next to each other on one XCD and the second
// to last of them find the codes in its L2.
// Guesses that nobody has measured: kCUs workgroups as the target (one per
// CU, not the two that fit), kMinSlices, kMaxSplit, KT, BM.
#pragma once

#include "common.h"
#include "linear_skinny.h"

namespace wq {

using skinny::f32x4;
using skinny::short8;
using skinny::u16;
using skinny::u8;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kTiles = 4;                       // 16-row weight tiles per wave
constexpr int BN = kWaves * kTiles * 16;        // weight rows per workgroup
constexpr int MT = 4;                           // 16-row tiles of x
constexpr int BM = MT * 16;                     // rows of x per workgroup
constexpr int KT = 128;                         // columns per slice
constexpr int LS = KT + skinny::kPad;           // LDS row stride, elements
constexpr int kXLoads = BM * KT / 8 / kThreads; // 16-byte x loads per thread
constexpr int kCUs = 256;       // guess: workgroups the grid aims at
constexpr int kMinSlices = 2;   // guess: a split has a slice to prefetch
constexpr int kMaxSplit = 32;   // guess

struct Grid { int m_blocks, n_blocks, n_split, k_chunk; };

inline Grid gemm_grid(int M, int N, int K) {
  Grid gr;
  gr.m_blocks = (M + BM - 1) / BM;
  gr.n_blocks = (N + BN - 1) / BN;
  const long long tiles = (long long)gr.m_blocks * gr.n_blocks;
  const long long slices = ((long long)K + KT - 1) / KT;
  long long n = kCUs / (tiles > 0 ? tiles : 1);
  if (n > slices / kMinSlices) n = slices / kMinSlices;
  if (n > kMaxSplit) n = kMaxSplit;
  if (n < 1) n = 1;
  const long long per = (slices + n - 1) / n > 0 ? (slices + n - 1) / n : 1;
  gr.k_chunk = (int)(per * KT);
  gr.n_split = (int)((slices + per - 1) / per > 0 ? (slices + per - 1) / per : 1);
  return gr;
}

// s_barrier behind a fence of LDS only: global loads stay in flight
ACCO_DEV void lds_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// workgroup `flat` of nwg runs on XCD flat % 8: give each XCD a contiguous
// range of the numbering (row block fastest, then weight block, then split)
ACCO_DEV int xcd_remap(int flat, int nwg) {
  const int q = nwg / 8, r = nwg % 8;
  const int xcd = flat % 8, idx = flat / 8;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

// A format F gives: Scale, Finish, kStep (k per 16-byte load of a tile, KT a
// multiple of it), Frag (a step's codes of the lane's four tiles), Ptr and
// ptrs (where the lane's loads start), load(frag, ptr, k) and
// mma(frag, xa, g, acc): the step's MFMAs, xa the LDS address of row j of the
// x tile at the step's first column.
template <class F>
__global__ __launch_bounds__(kThreads, 2)   // two waves per SIMD: 256 registers
void gemm_kernel(const u16* __restrict__ x, const u8* __restrict__ codes,
                 const typename F::Scale* __restrict__ scales,
                 typename F::Finish finish, u16* __restrict__ y,
                 float* __restrict__ part, int M, int N, int K, int k_chunk,
                 int n_split, int m_blocks, int n_blocks, long long x_rs) {
  constexpr int kSteps = KT / F::kStep;
  __shared__ __attribute__((aligned(16))) u16 xs[2][BM * LS];

  const int tid = __builtin_amdgcn_workitem_id_x();
  const int lane = tid % kWave, wave = tid / kWave;
  const int j = lane % 16, g = lane / 16;

  const int flat = xcd_remap(__builtin_amdgcn_workgroup_id_x(),
                             m_blocks * n_blocks * n_split);
  const int bm = flat % m_blocks, bn = flat / m_blocks % n_blocks;
  const int split = flat / m_blocks / n_blocks;
  const int m0 = bm * BM, m_live = min(BM, M - m0);
  const int k0 = split * k_chunk, k1 = min(K, k0 + k_chunk);

  int n[kTiles];
  long long row[kTiles];
#pragma unroll
  for (int t = 0; t < kTiles; ++t) {
    n[t] = bn * BN + (wave * kTiles + t) * 16 + j;
    row[t] = min(n[t], N - 1);
  }
  const typename F::Ptr wp = F::ptrs(codes, scales, row, K, g);

  f32x4 acc[kTiles][MT];
#pragma unroll
  for (int t = 0; t < kTiles; ++t)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[t][mt] = f32x4{0.f, 0.f, 0.f, 0.f};

  // a thread stages column group c8 (8 columns) of the rows r0 + 16 q
  const int c8 = tid % (KT / 8), r0 = tid / (KT / 8);
  const u16* xb = x + (long long)m0 * x_rs + 8 * c8;
  auto load_x = [&](uint4 (&xr)[kXLoads], int kt) {
#pragma unroll
    for (int q = 0; q < kXLoads; ++q) {
      const int r = r0 + q * (kThreads / (KT / 8));
      xr[q] = make_uint4(0u, 0u, 0u, 0u);
      if (r < m_live && kt + 8 * c8 < k1)
        xr[q] = *reinterpret_cast<const uint4*>(xb + (long long)r * x_rs + kt);
    }
  };
  auto store_x = [&](const uint4 (&xr)[kXLoads], u16* buf) {
#pragma unroll
    for (int q = 0; q < kXLoads; ++q)
      *reinterpret_cast<uint4*>(
          buf + (r0 + q * (kThreads / (KT / 8))) * LS + 8 * c8) = xr[q];
  };
  // the steps of a slice that begin below k1 (a whole number of them does);
  // the condition is the same for the whole workgroup
  struct Set { typename F::Frag f[kSteps]; };
  auto load_codes = [&](Set& w, int kt) {
#pragma unroll
    for (int s = 0; s < kSteps; ++s)
      if (kt + s * F::kStep < k1) F::load(w.f[s], wp, kt + s * F::kStep);
  };
  auto multiply = [&](const Set& w, const u16* buf, int kt) {
#pragma unroll
    for (int s = 0; s < kSteps; ++s)
      if (kt + s * F::kStep < k1)
        F::mma(w.f[s], buf + j * LS + s * F::kStep, g, acc);
  };

  uint4 xr[kXLoads];
  Set wa, wb;
  // a slice of the chunk: `cur` and `buf` hold it; the one after it goes to
  // `next` and the other buffer while it is multiplied
  auto slice = [&](const Set& cur, Set& next, const u16* buf, u16* other,
                   int kt) {
    const bool more = kt + KT < k1;
    if (more) {
      load_x(xr, kt + KT);
      load_codes(next, kt + KT);
    }
    multiply(cur, buf, kt);
    if (more) store_x(xr, other);
    lds_barrier();
  };

  load_x(xr, k0);
  load_codes(wa, k0);
  store_x(xr, xs[0]);
  lds_barrier();
  for (int kt = k0; kt < k1; kt += 2 * KT) {
    slice(wa, wb, xs[0], xs[1], kt);
    if (kt + KT < k1) slice(wb, wa, xs[1], xs[0], kt + KT);
  }

  // C layout: the lane holds weight row j of its tile (n[t]) for the x rows
  // m0 + 16 mt + 4 g + r; 16 lanes store 16 adjacent n of one x row. part:
  // fp32 [n_split, M, N], unused with one split, which stores y instead
#pragma unroll
  for (int t = 0; t < kTiles; ++t) {
    if (n[t] >= N) continue;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + mt * 16 + 4 * g + r;
        if (m >= M) continue;
        if (n_split == 1)
          y[(long long)m * N + n[t]] = finish(acc[t][mt][r], n[t]);
        else
          part[((long long)split * M + m) * N + n[t]] = acc[t][mt][r];
      }
  }
}

template <class F>
void launch(const typename F::Finish& finish, const void* x,
            const void* codes, const typename F::Scale* scales, void* y,
            float* workspace, int M, int N, int K, long long x_rs,
            hipStream_t stream) {
  if (M < 1 || N < 1) return;       // the binding admits neither
  const Grid gr = gemm_grid(M, N, K);
  hipLaunchKernelGGL(gemm_kernel<F>,
                     dim3((unsigned)gr.m_blocks * gr.n_blocks * gr.n_split),
                     dim3(kThreads), 0, stream, (const u16*)x,
                     (const u8*)codes, scales, finish, (u16*)y, workspace, M,
                     N, K, gr.k_chunk, gr.n_split, gr.m_blocks, gr.n_blocks,
                     x_rs);
  if (gr.n_split > 1) {
    const long long MN = (long long)M * N;
    hipLaunchKernelGGL(skinny::combine_kernel<typename F::Finish>,
                       dim3((unsigned)((MN + kThreads - 1) / kThreads)),
                       dim3(kThreads), 0, stream, workspace, finish, (u16*)y,
                       MN, N, gr.n_split);
  }
}

}  // namespace wq
