// Flash attention forward v4 for gfx950 — 32×32 MFMA structure with fully
// in-register softmax (guide §B "8-warp 32×32 ladder" + T12).
//
// Differences vs attention_fwd.hip (the 16×16 v3, kept as fallback):
// - mfma_f32_32x32x16_bf16: the swapped QK^T puts a q row's 64 scores in
//   TWO half-waves (col = lane&31, row = c32_row(reg, lane>>5)),
//   so the softmax row reduce is 31 in-lane ops + ONE shfl_xor(32);
// - P never touches LDS: the C-layout → A-fragment redistribution is two
//   v_permlane32_swap per 16-kv K-step (pairs su0↔su2, su1↔su3 — see the
//   pair-index derivation at c_to_afrag in attention_common.h);
// - 8 waves per workgroup (256 q rows): K/V staged once per kv tile for
//   all 8 waves; fully-causal-masked tiles skip compute per wave (barriers
//   kept);
// - D ∈ {64, 128} and S % 256 == 0 only (the dispatch falls back to v3
//   else).

#include "attention_common.h"
#include "kernels.h"

namespace {

using namespace attn;

// D=64 is capped at 128 VGPR: 2 co-resident 8-wave blocks per CU (4
// waves/SIMD) out-weigh scheduling freedom — measured faster than the
// uncapped 159-VGPR build and than a 204-VGPR T14 double-buffered variant.
//
// DOC: document-boundary masking for packed rows (attention_common.h). The
// lane's column is one query, so doc_start[b, q_g] joined with the window is
// ONE lower bound per lane; the block's first row shortens the tile range,
// the wave's first / last row extend the whole-tile skip and the interior
// shortcut. DOC = false compiles to the kernel without any of it.
template <int D, bool DOC>
__global__ __launch_bounds__(512, D == 64 ? 4 : 2)
void attn_fwd32_kernel(const u16* __restrict__ q, const u16* __restrict__ k,
                       const u16* __restrict__ v, u16* __restrict__ o,
                       float* __restrict__ lse,        // [B, H, S]
                       int S, int H, int Hkv, float scale, int window,
                       long long q_rs, long long kv_rs, long long o_rs,
                       const int* __restrict__ doc_start) {  // [B, S], DOC
  constexpr int KS = D / 16;       // QK^T K-steps over head dim (16 each)
  constexpr int DT = D / 32;       // 32-wide d tiles of the output
  const BlockPos pos = block_order(
      blockIdx.x, S / BT32, gridDim.x / (S / BT32), true);
  const int qt = pos.row_block, bh = pos.bh;
  const int b = bh / H, h = bh % H;
  const int hkv = h / (H / Hkv);
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int lq = lane & 31;        // q col (swapped QK^T) / d col (PV out)
  const int hi = lane >> 5;        // half-wave

  extern __shared__ __attribute__((aligned(16))) u16 smem[];
  u16* k_lds = smem + Fwd32Lds<D>::k_row;   // [TILE][D+8]
  u16* v_lds = smem + Fwd32Lds<D>::v_t;     // V^T: [D][LST]
  constexpr int KROW = D + 8;

  const int q0 = qt * BT32 + wave * QW32;
  const long long qs = q_rs;           // token-row strides (packed-qkv aware)
  const long long ks = kv_rs;
  const u16* Qp = q + ((long long)b * S + q0) * qs + (long long)h * D;
  const u16* Kb = k + (long long)b * S * ks + (long long)hkv * D;
  const u16* Vb = v + (long long)b * S * ks + (long long)hkv * D;

  // Q as B operand of the swapped QK^T: lane holds Q[q=lq][d=hi*8+i+16s]
  short8 qf[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s)
    qf[s] = *reinterpret_cast<const short8*>(
        Qp + (long long)lq * qs + s * 16 + hi * 8);

  float m_c = -1e30f, l_c = 0.0f;      // per q col = lq (dup over hi)
  f32x16 acc_o[DT] = {};

  int j_lo = kv_tile_lo(qt * BT32, window);
  const int j_hi = kv_tile_hi(qt * BT32, BT32);
  const int q_wave_max = q0 + QW32 - 1;
  // DOC: lo_q = lowest key of the lane's query; ds_w0 / ds_w1 = doc_start of
  // the wave's first / last row (wave-uniform)
  int lo_q = 0, ds_w0 = 0, ds_w1 = 0;
  if constexpr (DOC) {
    const int* ds = doc_start + (long long)b * S;
    lo_q = doc_lo(ds[q0 + lq], q0 + lq, window);
    ds_w0 = __builtin_amdgcn_readfirstlane(ds[q0]);
    ds_w1 = __builtin_amdgcn_readfirstlane(ds[q_wave_max]);
    j_lo = kv_tile_lo_doc(qt * BT32, window,
                          __builtin_amdgcn_readfirstlane(ds[qt * BT32]), S);
  }
  const float scale2 = scale * 1.4426950408889634f;   // log2 domain
  constexpr float THR2 = 8.0f * 1.4426950408889634f;  // defer-max (T13)

  for (int j = j_lo; j <= j_hi; ++j) {
    // ---- stage K (row-major copy) + V (transposed) for all 8 waves
    __syncthreads();
    stage_rowmajor<D, 512>(Kb + (long long)(j * TILE) * ks, ks, k_lds);
    stage_transposed<D, 512>(Vb + (long long)(j * TILE) * ks, ks, v_lds);
    __syncthreads();

    // fully-masked tile for this wave (kv all future, or all outside the
    // local window): skip compute
    if (j * TILE > q_wave_max ||
        (window > 0 && j * TILE + TILE - 1 <= q0 - window))
      continue;
    if constexpr (DOC)      // all kv before the wave's first document
      if (j * TILE + TILE - 1 < ds_w0) continue;

    // ---- S^T: st[m32] per 32-kv sub-tile (C: col=q=lq, row=kv spread)
    f32x16 st[2];
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int m32 = 0; m32 < 2; ++m32) {
      f32x16 acc = {};
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        short8 kf = *reinterpret_cast<const short8*>(
            k_lds + (m32 * 32 + lq) * KROW + s * 16 + hi * 8);
        acc = MFMA32(kf, qf[s], acc);
      }
      st[m32] = acc;
    }
    __builtin_amdgcn_s_setprio(0);

    // ---- mask + online softmax (per q col = lq), log2 domain: scores are
    // s·scale·log2e and raw v_exp_f32 (= 2^x) replaces mul+exp per element.
    // WAVE-level mask class: interior tiles (all kv ≤ all q, all in window)
    // skip the per-element predicates entirely.
    const int q_g = q0 + lq;
    bool need_mask = (j * TILE + TILE - 1 > q0) ||
                     (window > 0 && j * TILE <= q_wave_max - window);
    if constexpr (DOC) need_mask = need_mask || (j * TILE < ds_w1);
    float p[32];
    float tmax = -1e30f;
    if constexpr (!DOC) {
#pragma unroll
      for (int m32 = 0; m32 < 2; ++m32)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int kv_g = j * TILE + m32 * 32 + c32_row(r, hi);
          float x = st[m32][r] * scale2;
          if (need_mask) {
            x = attends(kv_g, q_g, window) ? x : -1e30f;
          }
          p[m32 * 16 + r] = x;
          tmax = fmaxf(tmax, x);
        }
    } else {
      // DOC: ONE wave-uniform branch per tile that masks the raw scores in
      // place; -inf survives the scaling (the bindings require scale > 0
      // with document bounds) and the exp2 below yields the same exact zero
      // as the plain kernel's -1e30. Left inside the element loop, the
      // two-compare predicate is turned into 32 unconditional selects and
      // interior tiles pay for them (forward 20% slower than the plain
      // kernel on one document); the empty volatile asm keeps the compiler
      // from doing that here too. Masking after the scaling instead costs
      // the D=64 build 12 B of scratch.
      if (__builtin_amdgcn_readfirstlane((int)need_mask)) {
        asm volatile("");
#pragma unroll
        for (int m32 = 0; m32 < 2; ++m32)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int kv_g = j * TILE + m32 * 32 + c32_row(r, hi);
            st[m32][r] =
                attends_lo(kv_g, q_g, lo_q) ? st[m32][r] : -INFINITY;
          }
      }
#pragma unroll
      for (int m32 = 0; m32 < 2; ++m32)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float x = st[m32][r] * scale2;
          p[m32 * 16 + r] = x;
          tmax = fmaxf(tmax, x);
        }
    }
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));

    // ---- T13 defer-max: skip the O-rescale pass (16 shfl + 32 mul) while
    // the wave's max grows ≤ 8 natural units (P bounded by e^8, fine in
    // f32 accumulation). Decision precedes this tile's exponentials and
    // the previous tile's PV is complete — the safe textbook order.
    float m_new = m_c;
    if (!__all(tmax <= m_c + THR2)) {
      m_new = fmaxf(m_c, tmax);
      const float alpha = __builtin_amdgcn_exp2f(m_c - m_new);
      l_c *= alpha;
      float alpha_row[16];
#pragma unroll
      for (int r = 0; r < 16; ++r)
        alpha_row[r] = __shfl(alpha, c32_row(r, hi), 64);
#pragma unroll
      for (int t = 0; t < DT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc_o[t][r] *= alpha_row[r];
      m_c = m_new;
    }
    float rsum = 0.0f;
#pragma unroll
    for (int i = 0; i < 32; ++i) {
      const float e =
          (p[i] > -9e29f) ? __builtin_amdgcn_exp2f(p[i] - m_new) : 0.0f;
      p[i] = e;
      rsum += e;
    }
    rsum += __shfl_xor(rsum, 32, 64);
    l_c += rsum;

    // ---- P (C layout) → A fragments in-register (c_to_afrag), then PV
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int m32 = 0; m32 < 2; ++m32) {
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        short8 pa = c_to_afrag(p + m32 * 16, kk);
#pragma unroll
        for (int t = 0; t < DT; ++t) {
          short8 vb = *reinterpret_cast<const short8*>(
              v_lds + (t * 32 + lq) * LST + m32 * 32 + kk * 16 + hi * 8);
          acc_o[t] = MFMA32(pa, vb, acc_o[t]);
        }
      }
    }
    __builtin_amdgcn_s_setprio(0);
  }

  // ---- epilogue: O rows q = c32_row(r, hi), col d = t*32 + lq
  float l_row[16];
#pragma unroll
  for (int r = 0; r < 16; ++r)
    l_row[r] = __shfl(l_c, c32_row(r, hi), 64);
  u16* Op = o + ((long long)b * S + q0) * o_rs + (long long)h * D;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const float inv_l = (l_row[r] > 0.f) ? 1.0f / l_row[r] : 0.0f;
    const int qrow = c32_row(r, hi);
#pragma unroll
    for (int t = 0; t < DT; ++t)
      Op[(long long)qrow * o_rs + t * 32 + lq] =
          f32_to_bf16(acc_o[t][r] * inv_l);
  }
  // lse stays in NATURAL units (the backward consumes exp(s·scale − lse));
  // the running m_c/l_c are log2-domain, so lse = ln2·(m2 + log2 l)
  if (hi == 0)
    lse[((long long)bh) * S + q0 + lq] =
        (m_c + __builtin_amdgcn_logf(fmaxf(l_c, 1e-30f))) *
        0.6931471805599453f;
}

}  // namespace

extern "C" void acco_attn_fwd32(const void* q, const void* k, const void* v,
                                void* o, float* lse, int B, int S, int H,
                                int Hkv, int D, float scale, int window,
                                long long q_rs, long long kv_rs,
                                long long o_rs, const int* doc_start,
                                hipStream_t stream) {
  dim3 grid(block_order_grid(S / BT32, B, H));
  // doc_start given: the DOC build; a window >= S bounds nothing, and
  // capping it keeps doc_lo / doc_hi free of overflow
#define LA(DD, DOC) hipLaunchKernelGGL((attn_fwd32_kernel<DD, DOC>), grid, \
    dim3(512), Fwd32Lds<DD>::bytes, stream, (const u16*)q, (const u16*)k, \
    (const u16*)v, (u16*)o, lse, S, H, Hkv, scale, \
    DOC ? (window < S ? window : S) : window, q_rs, kv_rs, o_rs, doc_start)
  if (doc_start != nullptr) {
    if (D == 64) LA(64, true); else LA(128, true);
  } else {
    if (D == 64) LA(64, false); else LA(128, false);
  }
#undef LA
}
