// Shared device code of the four attention files (attention_fwd.hip,
// attention_fwd32.hip, attention_bwd.hip, attention_bwd32.hip): tile
// constants, LDS staging, the 32x32 C-layout helpers, the causal/window tile
// ranges, every kernel's LDS layout and the host-side choice of kernel
// generation, and the order in which a grid's workgroups take their (row
// block, head). Device-only apart from that order and the two path
// predicates at the end.
#pragma once

#include "common.h"

namespace attn {

using u16 = unsigned short;
using short8 = __attribute__((ext_vector_type(8))) short;
using f32x4 = __attribute__((ext_vector_type(4))) float;
using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int TILE = 64;           // rows of a staged tile (kv or q)
constexpr int PAD = 8;
constexpr int LST = TILE + PAD;    // 72: row stride of transposed / P tiles
                                   // (144 B: 16 rows hit 16 distinct bank
                                   // groups for ds_read_b128)
// 32x32 generation: 8 waves of 32 rows = 256 rows per workgroup
constexpr int QW32 = 32, NW32 = 8, BT32 = QW32 * NW32;

#define MFMA(a, b, c) \
  __builtin_amdgcn_mfma_f32_16x16x32_bf16((a), (b), (c), 0, 0, 0)
#define MFMA32(a, b, c) \
  __builtin_amdgcn_mfma_f32_32x32x16_bf16((a), (b), (c), 0, 0, 0)

// ------------------------------------------------------------ LDS staging
// NT is the block's thread count (256 or 512). No __restrict__ on these
// parameters: it changes the ISA of the callers.

// stage a [TILE × D] global tile TRANSPOSED into LDS [D][LST]
// (paired-row ushort2 writes: half the instructions of scalar b16)
template <int D, int NT>
ACCO_DEV void stage_transposed(const u16* src, long long row_stride,
                               u16* dst) {
  const int r2 = (threadIdx.x & 31) * 2;            // tile row pair
  for (int dg = threadIdx.x >> 5; dg < D / 8; dg += NT / 32) {
    ushort4 a0 = reinterpret_cast<const ushort4*>(
        src + (long long)r2 * row_stride + dg * 8)[0];
    ushort4 a1 = reinterpret_cast<const ushort4*>(
        src + (long long)r2 * row_stride + dg * 8)[1];
    ushort4 b0 = reinterpret_cast<const ushort4*>(
        src + (long long)(r2 + 1) * row_stride + dg * 8)[0];
    ushort4 b1 = reinterpret_cast<const ushort4*>(
        src + (long long)(r2 + 1) * row_stride + dg * 8)[1];
    u16 av[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
    u16 bv[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
    for (int i = 0; i < 8; ++i)
      *reinterpret_cast<ushort2*>(dst + (dg * 8 + i) * LST + r2) =
          make_ushort2(av[i], bv[i]);
  }
}

// stage a [TILE × D] global tile ROW-MAJOR into LDS [TILE][D+8]
template <int D, int NT>
ACCO_DEV void stage_rowmajor(const u16* src, long long row_stride, u16* dst) {
  for (int c = threadIdx.x; c < TILE * (D / 8); c += NT) {
    const int r = c / (D / 8), dc = c % (D / 8);
    reinterpret_cast<uint4*>(dst + r * (D + 8))[dc] =
        *reinterpret_cast<const uint4*>(src + (long long)r * row_stride + dc * 8);
  }
}

// ---------------------------------------------------- 32x32 C-layout helpers
ACCO_DEV unsigned pack_bf16(float lo, float hi) {
  // v_cvt_pk_bf16_f32 (RNE, no builtin on gfx950 — guide T12): one
  // instruction replaces ~9 VALU of manual round-to-nearest-even
  // bit-twiddling per packed dword. The trailing s_nop 1 covers the
  // VALU-write → v_permlane32_swap hazard window for the consumer
  // (guide T21 hazard note; hipcc pads nothing inside asm).
  unsigned r;
  asm("v_cvt_pk_bf16_f32 %0, %1, %2\n\ts_nop 1"
      : "=v"(r) : "v"(lo), "v"(hi));
  return r;
}

// row of C register r within a 32-row mfma_32x32 sub-tile, for the lane's
// half-wave hi = lane >> 5 (the column is lane & 31)
ACCO_DEV int c32_row(int r, int hi) { return (r & 3) + 8 * (r >> 2) + 4 * hi; }

// C-layout floats (the 16 registers of one 32-row sub-tile, a float[] or an
// f32x16) → A fragment for K-step kk (16 of the 32 C rows), in registers.
// The A fragment's 4 dwords are row pairs (4*hi + j), j=0..3 (pair = row/2
// within the 16). The lane's own packed dwords su_j = pack(c[8kk+2j],
// c[8kk+2j+1]) carry pairs {2hi, 2hi+1, 4+2hi, 5+2hi}; swapping su0↔su2 and
// su1↔su3 across half-waves (v_permlane32_swap) yields exactly pairs
// 4hi+{0,2} and 4hi+{1,3}. kk must be a constant of an unrolled loop so an
// f32x16's element reads stay in VGPRs.
template <class C>
ACCO_DEV short8 c_to_afrag(const C& c, int kk) {
  const int b = kk * 8;
  unsigned su0 = pack_bf16(c[b + 0], c[b + 1]);
  unsigned su1 = pack_bf16(c[b + 2], c[b + 3]);
  unsigned su2 = pack_bf16(c[b + 4], c[b + 5]);
  unsigned su3 = pack_bf16(c[b + 6], c[b + 7]);
  auto r02 = __builtin_amdgcn_permlane32_swap(su0, su2, false, false);
  auto r13 = __builtin_amdgcn_permlane32_swap(su1, su3, false, false);
  short8 pa;
  reinterpret_cast<unsigned*>(&pa)[0] = r02[0];
  reinterpret_cast<unsigned*>(&pa)[1] = r13[0];
  reinterpret_cast<unsigned*>(&pa)[2] = r02[1];
  reinterpret_cast<unsigned*>(&pa)[3] = r13[1];
  return pa;
}

// ------------------------------------------------- causal / window ranges
// Ranges are inclusive, in TILE-row tiles.
// first / last kv tile a block of `rows` q rows starting at q_blk0 attends to
ACCO_DEV int kv_tile_lo(int q_blk0, int window) {
  int j_lo = 0;
  if (window > 0) {
    int kv_min = q_blk0 - window + 1;
    if (kv_min > 0) j_lo = kv_min / TILE;
  }
  return j_lo;
}
ACCO_DEV int kv_tile_hi(int q_blk0, int rows) {
  return (q_blk0 + rows - 1) / TILE;                 // causal
}

// first / last q tile that attends to a block of `rows` kv rows at kv_blk0
ACCO_DEV int q_tile_lo(int kv_blk0) { return kv_blk0 / TILE; }
ACCO_DEV int q_tile_hi(int kv_blk0, int rows, int S, int window) {
  int qt_hi = S / TILE - 1;
  if (window > 0) {
    const int q_lim = kv_blk0 + rows - 1 + window;
    qt_hi = min(qt_hi, q_lim / TILE);
  }
  return qt_hi;
}

// does query q_g attend to key kv_g (causal, window > 0: banded)
ACCO_DEV bool attends(int kv_g, int q_g, int window) {
  bool valid = (kv_g <= q_g);
  if (window > 0) valid = valid && (kv_g > q_g - window);
  return valid;
}

// ------------------------------------------------- document boundaries
// Packed rows: doc_start[b, s] is the first token of the document that holds
// token s, doc_end[b, s] the exclusive end of it; both int32 [B, S] and
// non-decreasing along s. Query i attends key j iff doc_start[i] <= j <= i
// (and j > i - window), or from the key's side j <= i < doc_end[j]. In the
// 32x32 kernels a lane's column is ONE query (forward, dq) or ONE key (dkv),
// so the document and the window bound fold into one int per lane and the
// mask stays two compares per element. The arrays are data: every tile
// index derived from them is clamped into [0, S/TILE - 1], so their content
// can change numbers but never an address.
ACCO_DEV int clamp_tile(int t, int S) { return max(0, min(t, S / TILE - 1)); }

// lowest key that query q_g attends to (its lane's doc_start value ds_q)
ACCO_DEV int doc_lo(int ds_q, int q_g, int window) {
  return window > 0 ? max(ds_q, q_g - window + 1) : ds_q;
}
// exclusive upper end of the queries that attend to key kv_g (doc_end de_k)
ACCO_DEV int doc_hi(int de_k, int kv_g, int window) {
  return window > 0 ? min(de_k, kv_g + window) : de_k;
}
ACCO_DEV bool attends_lo(int kv_g, int q_g, int lo) {
  return kv_g <= q_g && kv_g >= lo;
}
ACCO_DEV bool attends_hi(int kv_g, int q_g, int hi) {
  return kv_g <= q_g && q_g < hi;
}

// kv_tile_lo joined with the document of the block's first q row (ds_first =
// doc_start there; the rows after it start no earlier)
ACCO_DEV int kv_tile_lo_doc(int q_blk0, int window, int ds_first, int S) {
  return max(kv_tile_lo(q_blk0, window), clamp_tile(ds_first / TILE, S));
}
// q_tile_hi joined with the document of the block's last kv row (de_last =
// doc_end there; the rows before it end no later)
ACCO_DEV int q_tile_hi_doc(int kv_blk0, int rows, int S, int window,
                           int de_last) {
  return min(q_tile_hi(kv_blk0, rows, S, window),
             clamp_tile((max(de_last, 1) - 1) / TILE, S));
}

// ------------------------------------------------------------ block order
// Every attention kernel runs on a 1-D grid of n_blk * BH workgroups
// (n_blk row blocks of q or kv rows, BH = B * H heads) and takes its
// (row block, head) from this one function. Workgroups are dealt round-robin
// over the 8 XCDs in linear id order, so ids with the same id % 8 share an
// XCD, and a grid starts first to last. Causal cost grows with the row block
// (forward, dq: heavy_last) or shrinks with it (dkv), so:
//  - the head is the fast dimension: 8 consecutive ids are 8 heads of ONE
//    row block, i.e. every XCD gets the same work (exactly when BH % 8 == 0,
//    within one block otherwise);
//  - levels go heaviest first, so the light blocks fill in the tail.
// Placement is an observed property used for speed only: no kernel depends
// on it for its result. (Permuting the heads of a level so that the query
// heads of one kv group share an XCD was measured too: dq got slower in the
// training step, see RESULTS.md, so heads stay in plain order.)
struct BlockPos { int row_block, bh; };

__host__ __device__ __forceinline__ BlockPos block_order(
    unsigned id, unsigned n_blk, unsigned BH, bool heavy_last) {
  const unsigned level = id / BH;
  return {(int)(heavy_last ? n_blk - 1 - level : level),
          (int)(id - level * BH)};
}

inline unsigned block_order_grid(int n_blk, int B, int H) {
  return (unsigned)n_blk * (unsigned)(B * H);
}

// ------------------------------------------------------------ LDS layouts
// Offsets in u16 elements and the total in bytes; the kernel carves its
// dynamic LDS from the offsets, its launcher passes `bytes`.
constexpr int t_tile(int D) { return D * LST; }          // transposed [D][LST]
constexpr int r_tile(int D) { return TILE * (D + 8); }   // row-major [TILE][D+8]
constexpr int w_tile(int NW) { return NW * 16 * LST; }   // NW × per-wave [16][LST]

template <int D, int NW> struct FwdLds {         // attn_fwd_kernel
  static constexpr int v_t = 0, k_row = v_t + t_tile(D),
                       p = k_row + r_tile(D),            // p: per wave
                       bytes = (p + w_tile(NW)) * sizeof(u16);
};
template <int D> struct Fwd32Lds {               // attn_fwd32_kernel
  static constexpr int k_row = 0, v_t = k_row + r_tile(D),
                       bytes = (v_t + t_tile(D)) * sizeof(u16);
};
template <int D, int NW> struct BwdDqLds {       // attn_bwd_dq_kernel
  static constexpr int k_t = 0, k_row = k_t + t_tile(D),
                       v_row = k_row + r_tile(D),
                       ds = v_row + r_tile(D),           // ds: per wave
                       bytes = (ds + w_tile(NW)) * sizeof(u16);
};
template <int D, int NW> struct BwdDkvLds {      // attn_bwd_dkv_kernel
  static constexpr int q_t = 0, do_t = q_t + t_tile(D),
                       q_row = do_t + t_tile(D), do_row = q_row + r_tile(D),
                       p = do_row + r_tile(D),   // per wave: NW P^T tiles,
                                                 // then NW dS^T tiles
                       bytes = (p + 2 * w_tile(NW)) * sizeof(u16);
};
template <int D> struct Bwd32DqLds {             // attn_bwd32_dq_kernel
  static constexpr int k_row = 0, v_row = k_row + r_tile(D),
                       k_t = v_row + r_tile(D),
                       bytes = (k_t + t_tile(D)) * sizeof(u16);
};
template <int D> struct Bwd32DkvLds {            // attn_bwd32_dkv_kernel
  static constexpr int q_row = 0, do_row = q_row + r_tile(D),
                       q_t = do_row + r_tile(D), do_t = q_t + t_tile(D),
                       stats = do_t + t_tile(D),   // float [2][TILE]: the q
                                                   // tile's lse·log2e, delta·scale
                       bytes = stats * sizeof(u16) + 2 * TILE * sizeof(float);
  static_assert(stats * sizeof(u16) % 16 == 0, "stats rows are read as float4");
};

// ------------------------------------------------- host: choice of kernels
// the 32x32 generation (attention_*32.hip) takes whole 256-row blocks
inline bool use_mfma32(int S, int D) {
  return (D == 64 || D == 128) && S % BT32 == 0;
}
// 16x16 generation: 32 rows per wave instead of 16. D=128 at QW=32 needs
// ~197 VGPR -> 1 wave/SIMD; keep QW=16 there
inline bool wide(int S, int D) { return (S % 128 == 0) && (D == 64); }

}  // namespace attn
