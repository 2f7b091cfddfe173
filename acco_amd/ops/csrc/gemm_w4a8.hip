// MXFP4 x MXFP8 GEMM on the block-scaled MFMA of gfx950,
//   y[M, N] bf16 = dequant(xq, xs) . dequant(codes, scales)^T (+ bias[N])
// with any M >= 1 and N >= 1, K % 128 == 0: xq [M, K] e4m3 codes and xs
// [M, K / 32] e8m0 bytes as act_quant.hip stores them, codes [N, K / 2] bytes
// of two e2m1 each and scales [N, K / 32] e8m0 bytes as gemm_w4.hip reads
// them. Where gemm_w4.hip converts every code to bf16 in VALU and feeds
// v_mfma_f32_16x16x32_bf16, this kernel hands both code sets to
// v_mfma_scale_f32_16x16x128_f8f6f4 as they lie in memory: no convert, four
// times the k per instruction, the block scales applied by the matrix unit.
//
// The operands of the 16x16x128 instruction (CDNA4 ISA, "MFMA with block
// exponent scaling"; LLVM's llvm.amdgcn.mfma.scale.f32.16x16x128.f8f6f4), as
// this kernel relies on them and as tests/test_gpu_gemm_w4a8.py fixes them
// bit for bit (every weight code and every activation code in every k slot):
//   - lane (j, g) = (lane % 16, lane / 16) holds row j of A (of B: column j).
//     Registers 0 .. 3 of an operand are 16 bytes, chunk g of the first run of
//     64 bytes of the row's codes, registers 4 .. 7 chunk g of the second run.
//     e2m1 has one run: the lane's 16 bytes are the 32 consecutive k of block
//     g, k = 32 g + e (k even in the low nibble), the layout in memory. e4m3
//     has two: registers 0 .. 3 are k = 16 g + e, registers 4 .. 7 are
//     k = 64 + 16 g + e, e = 0 .. 15, NOT the 32 consecutive k of a block.
//     (The first version of this kernel read 32 consecutive bytes; the
//     identity tests then matched exactly where k % 64 < 16.);
//   - cbsz = 0 says A is e4m3, blgp = 4 says B is e2m1;
//   - the scale operand of a side is one register per lane whose byte op_sel
//     (an immediate) is the e8m0 scale of block g, k in [32 g, 32 g + 32), of
//     row j: for e2m1 the lane's own 32 k, for e4m3 not the lane's own data;
//   - C is the 16x16 layout of every other MFMA here: lane (j, g) holds
//     C[4 g + r][j], r = 0 .. 3.
// A is x and B the weight, so the epilogue is gemm_wq.h's.
//
// The tile is gemm_wq.h's. A workgroup of four waves owns BM = 64 rows of x by
// BN = 256 weight rows and walks its K chunk in slices of KT = 128 columns,
// here one MFMA deep. A wave owns four tiles of 16 weight rows and all 64
// rows of x: 16 accumulator tiles, 64 accumulator registers.
//   - Weights: lane (j, g) loads the 16 code bytes of block g of row j of
//     each of its four tiles, straight from global memory into the B operand,
//     never through LDS, every byte once per workgroup. Rows >= N point at
//     row N - 1 and are not stored. The lane's scale is byte g of the aligned
//     dword of scales[n] for the slice. A byte load puts it in bits 0 .. 7
//     with nothing to do before the MFMA (op_sel 0); loading the dword would
//     cost the same one load instruction per tile and a v_lshrrev by 8 g on
//     top, and the four lanes of a row hit one 4-byte word either way. So: a
//     byte load, as gemm_w4.hip has it.
//   - Activations go through LDS, double-buffered: rows of 128 code bytes,
//     then the row's four scale bytes for the slice, padded to a stride of
//     144 bytes; two buffers of 64 rows are 18 KB, half of gemm_wq.h's. An A
//     fragment is two ds_read_b128 (bytes 16 g + 64 h of row j) and one
//     ds_read_u8. A b128 pass serves the 16 lanes of one g: their addresses
//     are 144 j + const, 144 = 9 * 16 and 9 is odd, so the 16 rows fall into
//     the 16 distinct 16-byte groups of the 64 banks: no conflict, and no
//     address arithmetic beyond a constant stride. The x scales are staged
//     with the slice (one dword per row, loaded by the first 64 threads)
//     rather than read from global per fragment: 256 B a slice, and the
//     fragment's scale then comes from the same LDS row as its codes with no
//     global latency inside the MFMA loop. Rows >= M of a tile are zeros
//     (scale byte 0 times zero codes) and are never loaded.
//   - LDS per unit of matrix work: a fragment read (2 KB a wave) feeds four
//     MFMAs of 16 x 16 x 128, 512 B per MFMA against gemm_w4's 256 B per
//     16 x 16 x 32: a quarter of the bytes per multiply-add. A slice is 4
//     fragment reads and 16 MFMAs per wave; at 32 cycles an MFMA (twice the
//     bf16 rate with an e4m3 operand) that is 512 cycles of the matrix unit
//     against 32 KB of LDS reads of the four waves, 256 cycles at 128 B per
//     clock. Both rates are from the public CDNA4 figures, not measured here.
//   - Why BM stays 64: 128 rows were built first (kMT = 8: 128 accumulators,
//     two code sets of 20, 17 of staged x). They would halve the times a
//     weight byte comes from L2, which at M = 4096 is what this tile lacks.
//     The compiler hoists all eight A fragment reads of a slice (72
//     registers) in front of the MFMAs, with or without a scheduling barrier
//     between the row tiles, and reports 256 registers and 184 bytes of
//     scratch per lane. With kMT = 4 it reports no scratch and the two waves
//     per SIMD planned for (RESULTS.md, "MXFP4 x MXFP8 GEMM", has the
//     numbers). A kernel with scratch in its K loop is not the experiment;
//     128 rows need the fragment reads pinned by hand and are left open.
//   - The pipeline is gemm_wq.h's: while slice i is multiplied, the x codes
//     and scales and the weight codes of slice i + 1 are in flight into a
//     second register set; after the MFMAs the x registers go to the other
//     LDS buffer, and one lds_barrier per slice orders both directions.
// wq::gemm_grid, the XCD remap, the split of K with fp32 partials by ordinary
// stores summed in split order by skinny::combine_kernel, and mxfp4::Finish
// are the shared ones: no atomics, the same bits on every run. The grid's
// constants are the guesses gemm_wq.h names, not measured for this kernel
// either.

// Built like gemm_w4.hip, without the packed fp32 VALU ops, so that the
// shared skinny::combine_kernel<mxfp4::Finish> is the same code in every file
// that instantiates it. linear_skinny.h says why the attribute opens before
// the includes; the host pass does not know the feature, hence the guard.
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
using i32x8 = __attribute__((ext_vector_type(8))) int;

constexpr int kMT = MT;                           // 16-row tiles of x
constexpr int kBM = BM;                           // rows of x per workgroup
constexpr int kLS = KT + 16;                      // LDS row stride, bytes
constexpr int kXL = kBM * KT / 16 / kThreads;     // 16-byte x loads per thread
static_assert(kBM <= kThreads, "one thread per row stages the x scales");

__global__ __launch_bounds__(kThreads, 2)   // two waves per SIMD: 256 registers
void gemm_w4a8_kernel(const u8* __restrict__ xq, const u8* __restrict__ xsc,
                      const u8* __restrict__ codes,
                      const u8* __restrict__ scales, mxfp4::Finish finish,
                      u16* __restrict__ y, float* __restrict__ part, int M,
                      int N, int K, int k_chunk, int n_split, int m_blocks,
                      int n_blocks) {
  __shared__ __attribute__((aligned(16))) u8 xs[2][kBM * kLS];

  const int tid = __builtin_amdgcn_workitem_id_x();
  const int lane = tid % kWave, wave = tid / kWave;
  const int j = lane % 16, g = lane / 16;

  const int flat = xcd_remap(__builtin_amdgcn_workgroup_id_x(),
                             m_blocks * n_blocks * n_split);
  const int bm = flat % m_blocks, bn = flat / m_blocks % n_blocks;
  const int split = flat / m_blocks / n_blocks;
  const int m0 = bm * kBM, m_live = min(kBM, M - m0);
  const int k0 = split * k_chunk, k1 = min(K, k0 + k_chunk);

  int n[kTiles];
  const u8 *wc[kTiles], *wsc[kTiles];
#pragma unroll
  for (int t = 0; t < kTiles; ++t) {
    n[t] = bn * BN + (wave * kTiles + t) * 16 + j;
    const long long row = min(n[t], N - 1);
    wc[t] = codes + row * (K / 2) + 16 * g;
    wsc[t] = scales + row * (K / 32) + g;
  }

  f32x4 acc[kTiles][kMT];
#pragma unroll
  for (int t = 0; t < kTiles; ++t)
#pragma unroll
    for (int mt = 0; mt < kMT; ++mt) acc[t][mt] = f32x4{0.f, 0.f, 0.f, 0.f};

  // a thread stages 16-byte group c16 of the rows r0 + 32 q, and thread r the
  // scale dword of row r
  const int c16 = tid % (KT / 16), r0 = tid / (KT / 16);
  const u8* xb = xq + (long long)m0 * K + 16 * c16;
  const u8* sb = xsc + (long long)(m0 + tid) * (K / 32);
  struct XRegs { uint4 c[kXL]; unsigned s; };
  auto load_x = [&](XRegs& xr, int kt) {
#pragma unroll
    for (int q = 0; q < kXL; ++q) {
      const int r = r0 + q * (kThreads / (KT / 16));
      xr.c[q] = make_uint4(0u, 0u, 0u, 0u);
      if (r < m_live)
        xr.c[q] = *reinterpret_cast<const uint4*>(xb + (long long)r * K + kt);
    }
    xr.s = 0u;
    if (tid < m_live) xr.s = *reinterpret_cast<const unsigned*>(sb + kt / 32);
  };
  auto store_x = [&](const XRegs& xr, u8* buf) {
#pragma unroll
    for (int q = 0; q < kXL; ++q)
      *reinterpret_cast<uint4*>(
          buf + (r0 + q * (kThreads / (KT / 16))) * kLS + 16 * c16) = xr.c[q];
    if (tid < kBM) *reinterpret_cast<unsigned*>(buf + tid * kLS + KT) = xr.s;
  };
  struct Set { uint4 c[kTiles]; int s[kTiles]; };
  auto load_codes = [&](Set& w, int kt) {
#pragma unroll
    for (int t = 0; t < kTiles; ++t) {
      w.c[t] = *reinterpret_cast<const uint4*>(wc[t] + kt / 2);
      w.s[t] = wsc[t][kt / 32];
    }
  };
  auto multiply = [&](const Set& w, const u8* buf) {
    i32x8 b[kTiles];
#pragma unroll
    for (int t = 0; t < kTiles; ++t)
      b[t] = i32x8{(int)w.c[t].x, (int)w.c[t].y, (int)w.c[t].z,
                   (int)w.c[t].w, 0, 0, 0, 0};      // e2m1 reads four of them
    const u8* xa = buf + j * kLS;
#pragma unroll
    for (int mt = 0; mt < kMT; ++mt) {
      const u8* row = xa + mt * 16 * kLS;
      const uint4 lo = *reinterpret_cast<const uint4*>(row + 16 * g);
      const uint4 hi = *reinterpret_cast<const uint4*>(row + 64 + 16 * g);
      const int sa = row[KT + g];
      const i32x8 a{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w,
                    (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
#pragma unroll
      for (int t = 0; t < kTiles; ++t)
        acc[t][mt] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
            a, b[t], acc[t][mt], 0 /* A e4m3 */, 4 /* B e2m1 */, 0, sa, 0,
            w.s[t]);
    }
  };

  XRegs xr;
  Set wa, wb;
  auto slice = [&](const Set& cur, Set& next, const u8* buf, u8* other,
                   int kt) {
    const bool more = kt + KT < k1;
    if (more) {
      load_x(xr, kt + KT);
      load_codes(next, kt + KT);
    }
    multiply(cur, buf);
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

  // gemm_wq.h's tail: the lane holds weight row n[t] for the x rows
  // m0 + 16 mt + 4 g + r; part is fp32 [n_split, M, N]
#pragma unroll
  for (int t = 0; t < kTiles; ++t) {
    if (n[t] >= N) continue;
#pragma unroll
    for (int mt = 0; mt < kMT; ++mt)
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

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

}  // namespace

extern "C" void acco_gemm_w4a8_grid(int M, int N, int K, int* m_blocks,
                                    int* n_blocks, int* n_split,
                                    int* k_chunk) {
  const Grid gr = gemm_grid(M, N, K);
  *m_blocks = gr.m_blocks, *n_blocks = gr.n_blocks;
  *n_split = gr.n_split, *k_chunk = gr.k_chunk;
}

extern "C" void acco_gemm_w4a8(const void* xq, const void* xs,
                               const void* codes, const void* scales,
                               const void* bias, void* y, float* workspace,
                               int M, int N, int K, hipStream_t stream) {
  if (M < 1 || N < 1) return;       // the binding admits neither
  const Grid gr = gemm_grid(M, N, K);
  const mxfp4::Finish finish{(const u16*)bias};
  hipLaunchKernelGGL(gemm_w4a8_kernel,
                     dim3((unsigned)gr.m_blocks * gr.n_blocks * gr.n_split),
                     dim3(kThreads), 0, stream, (const u8*)xq, (const u8*)xs,
                     (const u8*)codes, (const u8*)scales, finish, (u16*)y,
                     workspace, M, N, K, gr.k_chunk, gr.n_split, gr.m_blocks,
                     gr.n_blocks);
  if (gr.n_split > 1) {
    const long long MN = (long long)M * N;
    hipLaunchKernelGGL(skinny::combine_kernel<mxfp4::Finish>,
                       dim3((unsigned)((MN + kThreads - 1) / kThreads)),
                       dim3(kThreads), 0, stream, workspace, finish, (u16*)y,
                       MN, N, gr.n_split);
  }
}
