// Flash attention backward v4 for gfx950 — 32×32 MFMA structure with
// in-register P/dS redistribution (no per-wave LDS round trips), mirroring
// attention_fwd32.hip. D ∈ {64, 128} and S % 256 == 0 (v3 fallback else);
// the D=128 dkv build trades K/V register residency and T14 staging for
// accumulator headroom (see KV_RES) — 256 VGPRs, none spilled, occupancy 2.
//
//   dq kernel : grid over 256-row Q blocks (8 waves × 32 q rows);
//               per 64-kv tile recompute S^T = K·Q^T and dP^T = V·dO^T
//               (swapped: C col = q), dS^T in registers, dQ += dS·K with
//               dS redistributed C→A by two v_permlane32_swap per K-step.
//   dkv kernel: grid over 256-row KV blocks (8 waves × 32 kv rows);
//               per 64-q tile S = Q·K^T, dP = dO·V^T (C col = kv),
//               dV += P^T·dO and dK += dS^T·Q via the same redistribution.
//               The q tile's lse/delta are staged into LDS with the tile
//               and read back as float4 per four C rows (no cross-lane
//               shuffles).

#include "attention_common.h"
#include "kernels.h"

namespace {

using namespace attn;

// ------------------------------------------------------------------- dQ
// D=64 capped at 128 VGPR: 2 co-resident 8-wave blocks per CU, matching
// the forward kernel's occupancy choice.
// DOC (document boundaries, attention_common.h): as in the forward kernel
// the lane's column is one query, so its doc_start joined with the window
// is one lower bound per lane. DOC = false compiles to the kernel without it.
template <int D, bool DOC>
__global__ __launch_bounds__(512, D == 64 ? 4 : 2)
void attn_bwd32_dq_kernel(const u16* __restrict__ q, const u16* __restrict__ k,
                          const u16* __restrict__ v, const u16* __restrict__ dO,
                          const float* __restrict__ lse,
                          const float* __restrict__ delta,
                          u16* __restrict__ dq,
                          int S, int H, int Hkv, float scale, int window,
                          long long q_rs, long long kv_rs, long long do_rs,
                          long long dq_rs,
                          const float* __restrict__ rope_cos,   // [S, D] or
                          const float* __restrict__ rope_sin,   // null = off
                          const int* __restrict__ doc_start) {  // [B,S], DOC
  constexpr int KS = D / 16;
  constexpr int DT = D / 32;
  constexpr int KROW = D + 8;
  const BlockPos pos = block_order(
      blockIdx.x, S / BT32, gridDim.x / (S / BT32), true);
  const int qt = pos.row_block, bh = pos.bh;
  const int b = bh / H, h = bh % H, hkv = h / (H / Hkv);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int lq = lane & 31, hi = lane >> 5;

  extern __shared__ __attribute__((aligned(16))) u16 smem[];
  using L = Bwd32DqLds<D>;
  u16* k_row = smem + L::k_row;            // [TILE][KROW]
  u16* v_row = smem + L::v_row;            // [TILE][KROW]
  u16* kT_lds = smem + L::k_t;             // [D][LST]

  const long long qs = q_rs, ks = kv_rs;
  const int q0 = qt * BT32 + wave * QW32;
  const u16* Qp = q + ((long long)b * S + q0) * qs + (long long)h * D;
  const u16* dOp = dO + ((long long)b * S + q0) * do_rs + (long long)h * D;
  const u16* Kb = k + (long long)b * S * ks + (long long)hkv * D;
  const u16* Vb = v + (long long)b * S * ks + (long long)hkv * D;

  short8 qf[KS], dof[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    qf[s] = *reinterpret_cast<const short8*>(
        Qp + (long long)lq * qs + s * 16 + hi * 8);
    dof[s] = *reinterpret_cast<const short8*>(
        dOp + (long long)lq * do_rs + s * 16 + hi * 8);
  }
  // log2-domain P recompute: lse pre-scaled by log2e, delta by ·scale so
  // the per-element work is one mul, one exp2 and one fma
  const float lse2_c = lse[(long long)bh * S + q0 + lq] * 1.4426950408889634f;
  const float delta_s = delta[(long long)bh * S + q0 + lq] * scale;
  const float scale2 = scale * 1.4426950408889634f;

  f32x16 acc_dq[DT] = {};

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

  for (int j = j_lo; j <= j_hi; ++j) {
    __syncthreads();
    stage_rowmajor<D, 512>(Kb + (long long)(j * TILE) * ks, ks, k_row);
    stage_rowmajor<D, 512>(Vb + (long long)(j * TILE) * ks, ks, v_row);
    stage_transposed<D, 512>(Kb + (long long)(j * TILE) * ks, ks, kT_lds);
    __syncthreads();
    if (j * TILE > q_wave_max) continue;
    if constexpr (DOC)      // all kv before the wave's first document
      if (j * TILE + TILE - 1 < ds_w0) continue;

#pragma unroll
    for (int m32 = 0; m32 < 2; ++m32) {
      f32x16 st = {}, dpt = {};
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        short8 kf = *reinterpret_cast<const short8*>(
            k_row + (m32 * 32 + lq) * KROW + s * 16 + hi * 8);
        short8 vf = *reinterpret_cast<const short8*>(
            v_row + (m32 * 32 + lq) * KROW + s * 16 + hi * 8);
        st = MFMA32(kf, qf[s], st);
        dpt = MFMA32(vf, dof[s], dpt);
      }
      __builtin_amdgcn_s_setprio(0);

      // dS^T (C: col=q=lq, row=kv spread); interior tiles (all kv ≤ all q,
      // all within the window) skip the per-element mask predicates
      const int q_g = q0 + lq;
      bool need_mask = (j * TILE + TILE - 1 > q0) ||
                       (window > 0 && j * TILE <= q_wave_max - window);
      if constexpr (DOC) need_mask = need_mask || (j * TILE < ds_w1);
      // DOC: one wave-uniform branch per sub-tile masks the raw scores in
      // place with -inf (scale > 0 with document bounds, see the bindings):
      // exp2 gives the plain kernel's exact zero. The empty volatile asm
      // keeps it a branch, as in the forward kernel.
      if constexpr (DOC)
        if (__builtin_amdgcn_readfirstlane((int)need_mask)) {
          asm volatile("");
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int kv_g = j * TILE + m32 * 32 + c32_row(r, hi);
            st[r] = attends_lo(kv_g, q_g, lo_q) ? st[r] : -INFINITY;
          }
        }
      float ds16[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float x = st[r] * scale2 - lse2_c;
        if constexpr (!DOC)
          if (need_mask) {
            const int kv_g = j * TILE + m32 * 32 + c32_row(r, hi);
            x = attends(kv_g, q_g, window) ? x : -1e30f;
          }
        const float pval = __builtin_amdgcn_exp2f(x);
        ds16[r] = pval * __builtin_fmaf(dpt[r], scale, -delta_s);
      }

      // dQ += dS·K (A = dS[row=q][k=kv] via swap; B = K^T from kT_lds)
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        short8 dsa = c_to_afrag(ds16, kk);
#pragma unroll
        for (int t = 0; t < DT; ++t) {
          short8 kb = *reinterpret_cast<const short8*>(
              kT_lds + (t * 32 + lq) * LST + m32 * 32 + kk * 16 + hi * 8);
          acc_dq[t] = MFMA32(dsa, kb, acc_dq[t]);
        }
      }
      __builtin_amdgcn_s_setprio(0);
    }
  }

  u16* dQp = dq + ((long long)b * S + q0) * dq_rs + (long long)h * D;
  // Fused inverse RoPE (rotation by -theta): column d = t*32 + lq and its
  // partner d + D/2 are acc_dq[t][r] / acc_dq[t + DT/2][r] of the SAME lane,
  // so the rotation is lane-local — the separate read-modify-write pass
  // over dq disappears. The accumulators are rounded to bf16 first and the
  // rotation runs on the rounded values, exactly as the stand-alone
  // rope_kernel<true> pass over the stored dq did: results stay bit-equal.
  if (rope_cos != nullptr) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int qrow = c32_row(r, hi);
      const float* cr = rope_cos + (long long)(q0 + qrow) * D + lq;
      const float* sr = rope_sin + (long long)(q0 + qrow) * D + lq;
#pragma unroll
      for (int t = 0; t < DT / 2; ++t) {
        const float c = cr[t * 32], sn = sr[t * 32];
        const float g1 = bf16_to_f32(f32_to_bf16(acc_dq[t][r]));
        const float g2 = bf16_to_f32(f32_to_bf16(acc_dq[t + DT / 2][r]));
        // explicit contraction, the one rope_kernel<true> compiles to
        // (sin product rounded, cos product fused)
        acc_dq[t][r] = __fmaf_rn(g1, c, __fmul_rn(g2, sn));
        acc_dq[t + DT / 2][r] = __fmaf_rn(g2, c, -__fmul_rn(g1, sn));
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int qrow = c32_row(r, hi);
#pragma unroll
    for (int t = 0; t < DT; ++t)
      dQp[(long long)qrow * dq_rs + t * 32 + lq] = f32_to_bf16(acc_dq[t][r]);
  }
}

// ---------------------------------------------------------------- dK, dV
// DOC: the lane's column is one KEY here, so the mask comes from the key's
// side: q_g < doc_end[b, kv_g], joined with the window into one exclusive
// upper bound per lane. The block's last row shortens qt_hi (the T14
// prefetch follows it), the wave's last / first row extend the whole-tile
// skip and the interior shortcut.
template <int D, bool DOC>
__global__ __launch_bounds__(512)
void attn_bwd32_dkv_kernel(const u16* __restrict__ q, const u16* __restrict__ k,
                           const u16* __restrict__ v,
                           const u16* __restrict__ dO,
                           const float* __restrict__ lse,
                           const float* __restrict__ delta,
                           u16* __restrict__ dk, u16* __restrict__ dv,
                           int S, int H, int Hkv, float scale, int window,
                           long long q_rs, long long kv_rs, long long do_rs,
                           const int* __restrict__ doc_end) {  // [B,S], DOC
  constexpr int KS = D / 16;
  constexpr int DT = D / 32;
  constexpr int KROW = D + 8;
  const BlockPos pos = block_order(
      blockIdx.x, S / BT32, gridDim.x / (S / BT32), false);
  const int jb = pos.row_block, bh = pos.bh;
  const int b = bh / H, h = bh % H, hkv = h / (H / Hkv);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int lq = lane & 31, hi = lane >> 5;

  extern __shared__ __attribute__((aligned(16))) u16 smem[];
  using L = Bwd32DkvLds<D>;
  u16* q_row = smem + L::q_row;             // [TILE][KROW]
  u16* do_row = smem + L::do_row;           // [TILE][KROW]
  u16* qT_lds = smem + L::q_t;              // [D][LST]
  u16* doT_lds = smem + L::do_t;            // [D][LST]
  // the q tile's row statistics, pre-scaled for the log2-domain recompute:
  // [0, TILE) lse·log2e, [TILE, 2·TILE) delta·scale
  float* stat_lds = reinterpret_cast<float*>(smem + L::stats);

  const long long qs = q_rs, ks = kv_rs;
  const long long od = (long long)H * D;   // dk/dv temps: contiguous [B,S,H,D]
  const int kv0 = jb * BT32 + wave * QW32;
  const u16* Kp = k + ((long long)b * S + kv0) * ks + (long long)hkv * D;
  const u16* Vp = v + ((long long)b * S + kv0) * ks + (long long)hkv * D;
  const u16* Qb = q + (long long)b * S * qs + (long long)h * D;
  const u16* dOb = dO + (long long)b * S * do_rs + (long long)h * D;

  // K^T / V^T as B operands: lane = K[kv=lq][d=hi*8+i+16s].
  // Register-resident at D=64 (64 VGPRs); at D=128 that residency pushes
  // the kernel to 91 spilled VGPRs, so the fragments are re-read from the
  // L2-hot global rows inside the K-step loop instead.
  constexpr bool KV_RES = (D == 64);
  short8 kTf[KV_RES ? KS : 1], vTf[KV_RES ? KS : 1];
  if constexpr (KV_RES) {
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      kTf[s] = *reinterpret_cast<const short8*>(
          Kp + (long long)lq * ks + s * 16 + hi * 8);
      vTf[s] = *reinterpret_cast<const short8*>(
          Vp + (long long)lq * ks + s * 16 + hi * 8);
    }
  }

  f32x16 acc_dk[DT] = {}, acc_dv[DT] = {};

  const int qt_lo = q_tile_lo(jb * BT32);
  int qt_hi = q_tile_hi(jb * BT32, BT32, S, window);
  const int kv_wave_min = kv0;
  // DOC: hi_k = exclusive end of the queries of the lane's key; de_w0 /
  // de_w1 = doc_end of the wave's first / last row (wave-uniform)
  int hi_k = 0, de_w0 = 0, de_w1 = 0;
  if constexpr (DOC) {
    const int* de = doc_end + (long long)b * S;
    hi_k = doc_hi(de[kv0 + lq], kv0 + lq, window);
    de_w0 = __builtin_amdgcn_readfirstlane(de[kv0]);
    de_w1 = __builtin_amdgcn_readfirstlane(de[kv0 + QW32 - 1]);
    qt_hi = q_tile_hi_doc(
        jb * BT32, BT32, S, window,
        __builtin_amdgcn_readfirstlane(de[jb * BT32 + BT32 - 1]));
  }

  // T14 async staging: hold the next q tile's Q/dO loads in registers
  // across the barrier; the loads stay in flight under the MFMA work.
  // Transpose staging uses a (d-pair, kv-oct) item scheme of its own:
  // 8 coalesced uint row loads → two ds_write_b128
  // (replaces 8 narrow ushort2 writes per tensor — 2.4× fewer LDS write
  // cycles). Threads < half stage Q^T, the other half dO^T.
  const bool t_q = (threadIdx.x < 256);   // D=64 only: 256 items per tensor
  const int t_id = threadIdx.x & 255;
  const int t_d0 = (t_id % 32) * 2;
  const int t_kv8 = (t_id / 32) * 8;
  unsigned streg[8];
  // row-major staging piece: one uint4 per thread per tensor (TILE*D/8/512)
  static_assert(TILE * (D / 8) % 512 == 0, "rowmajor chunks");
  constexpr int RCH = TILE * (D / 8) / 512;
  uint4 rq[RCH], rdo[RCH];
  // waves 0 / 1 stage the tile's 64 lse / delta values (one per thread)
  const bool st_on = (threadIdx.x < 2 * TILE);
  const float* st_src = (threadIdx.x < TILE ? lse : delta) +
                        (long long)bh * S + (threadIdx.x & (TILE - 1));
  const float st_mul = (threadIdx.x < TILE) ? 1.4426950408889634f : scale;
  float streg_stat = 0.0f;

  auto load_qtile = [&](int qt) {
    const u16* Qs = Qb + (long long)(qt * TILE) * qs;
    const u16* Ds = dOb + (long long)(qt * TILE) * do_rs;
    if (st_on) streg_stat = st_src[qt * TILE];
    if (D == 64) {
      // half the threads stage Q^T items, half dO^T items
      const u16* Ts = t_q ? Qs : Ds;
      const long long tstride = t_q ? qs : do_rs;
#pragma unroll
      for (int r = 0; r < 8; ++r)
        streg[r] = *reinterpret_cast<const unsigned*>(
            Ts + (long long)(t_kv8 + r) * tstride + t_d0);
    }
#pragma unroll
    for (int c = 0; c < RCH; ++c) {
      const int cc = threadIdx.x + c * 512;
      const int r = cc / (D / 8), dc = cc % (D / 8);
      rq[c] = *reinterpret_cast<const uint4*>(Qs + (long long)r * qs + dc * 8);
      rdo[c] = *reinterpret_cast<const uint4*>(Ds + (long long)r * do_rs + dc * 8);
    }
  };
  auto write_qtile = [&]() {
    if (st_on) stat_lds[threadIdx.x] = streg_stat * st_mul;
    if (D == 64) {
      uint4 lo, hi4;
      lo.x = (streg[0] & 0xffffu) | (streg[1] << 16);
      lo.y = (streg[2] & 0xffffu) | (streg[3] << 16);
      lo.z = (streg[4] & 0xffffu) | (streg[5] << 16);
      lo.w = (streg[6] & 0xffffu) | (streg[7] << 16);
      hi4.x = (streg[0] >> 16) | (streg[1] & 0xffff0000u);
      hi4.y = (streg[2] >> 16) | (streg[3] & 0xffff0000u);
      hi4.z = (streg[4] >> 16) | (streg[5] & 0xffff0000u);
      hi4.w = (streg[6] >> 16) | (streg[7] & 0xffff0000u);
      u16* dst = t_q ? qT_lds : doT_lds;
      *reinterpret_cast<uint4*>(dst + t_d0 * LST + t_kv8) = lo;
      *reinterpret_cast<uint4*>(dst + (t_d0 + 1) * LST + t_kv8) = hi4;
    }
#pragma unroll
    for (int c = 0; c < RCH; ++c) {
      const int cc = threadIdx.x + c * 512;
      const int r = cc / (D / 8), dc = cc % (D / 8);
      reinterpret_cast<uint4*>(q_row + r * KROW)[dc] = rq[c];
      reinterpret_cast<uint4*>(do_row + r * KROW)[dc] = rdo[c];
    }
  };

  // direct (non-T14) staging for the !KV_RES (D=128) build: the
  // cross-barrier register staging holds 32 VGPRs for the whole loop and
  // tips the 128-VGPR accumulator build into spilling
  auto stage_qtile_direct = [&](int qt) {
    const u16* Qs = Qb + (long long)(qt * TILE) * qs;
    const u16* Ds = dOb + (long long)(qt * TILE) * do_rs;
    stage_transposed<D, 512>(Qs, qs, qT_lds);
    stage_transposed<D, 512>(Ds, do_rs, doT_lds);
    stage_rowmajor<D, 512>(Qs, qs, q_row);
    stage_rowmajor<D, 512>(Ds, do_rs, do_row);
    if (st_on) stat_lds[threadIdx.x] = st_src[qt * TILE] * st_mul;
  };

  if constexpr (KV_RES) load_qtile(qt_lo);
  for (int qt = qt_lo; qt <= qt_hi; ++qt) {
    __syncthreads();
    if constexpr (KV_RES) {
      write_qtile();
    } else {
      stage_qtile_direct(qt);
    }
    __syncthreads();
    if constexpr (KV_RES)
      if (qt < qt_hi) load_qtile(qt + 1);  // in flight under the MFMAs
    // tile fully before this wave's kv rows → all masked: skip compute
    if (qt * TILE + TILE - 1 < kv_wave_min) continue;
    if constexpr (DOC)      // all q after the wave's last document
      if (qt * TILE >= de_w1) continue;

#pragma unroll
    for (int m32 = 0; m32 < 2; ++m32) {
      f32x16 st = {}, dpt = {};
      __builtin_amdgcn_s_setprio(1);
      if constexpr (KV_RES) {
#pragma unroll
        for (int s = 0; s < KS; ++s) {
          short8 qfr = *reinterpret_cast<const short8*>(
              q_row + (m32 * 32 + lq) * KROW + s * 16 + hi * 8);
          short8 dofr = *reinterpret_cast<const short8*>(
              do_row + (m32 * 32 + lq) * KROW + s * 16 + hi * 8);
          st = MFMA32(qfr, kTf[s], st);
          dpt = MFMA32(dofr, vTf[s], dpt);
        }
      } else {
        // non-resident K/V (D=128): bounded unroll keeps the in-flight
        // global loads from ballooning the register file (full unroll of
        // 8 K-steps spills)
#pragma unroll 2
        for (int s = 0; s < KS; ++s) {
          short8 qfr = *reinterpret_cast<const short8*>(
              q_row + (m32 * 32 + lq) * KROW + s * 16 + hi * 8);
          short8 dofr = *reinterpret_cast<const short8*>(
              do_row + (m32 * 32 + lq) * KROW + s * 16 + hi * 8);
          short8 kf = *reinterpret_cast<const short8*>(
              Kp + (long long)lq * ks + s * 16 + hi * 8);
          short8 vf = *reinterpret_cast<const short8*>(
              Vp + (long long)lq * ks + s * 16 + hi * 8);
          st = MFMA32(qfr, kf, st);
          dpt = MFMA32(dofr, vf, dpt);
        }
      }
      __builtin_amdgcn_s_setprio(0);

      // P and dS (C: col = kv = lq, row = q spread) — written back into
      // st/dpt in place: separate p16/ds16 arrays cost 32 VGPRs and spill
      // the D=128 instantiation
      const int kv_g = kv0 + lq;
      const float scale2_ = scale * 1.4426950408889634f;
      // interior q tiles (all q ≥ all kv of this wave, all within window)
      // skip the per-element mask predicates; (q_g < S) holds by S % TILE == 0
      bool need_mask =
          (qt * TILE < kv0 + QW32 - 1) ||
          (window > 0 && kv0 + window <= qt * TILE + TILE - 1);
      if constexpr (DOC)
        need_mask = need_mask || (qt * TILE + TILE - 1 >= de_w0);
      // row statistics from LDS: C registers 4g..4g+3 are the consecutive
      // rows 8g + 4hi + 0..3 (c32_row), one float4 each; a half-wave reads
      // one address, a conflict-free broadcast
      const float* lse_r = stat_lds + m32 * 32 + 4 * hi;
      const float* del_r = lse_r + TILE;
      // DOC: one wave-uniform branch, raw scores masked in place (see dq)
      if constexpr (DOC)
        if (__builtin_amdgcn_readfirstlane((int)need_mask)) {
          asm volatile("");
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int q_g = qt * TILE + m32 * 32 + c32_row(r, hi);
            st[r] = attends_hi(kv_g, q_g, hi_k) ? st[r] : -INFINITY;
          }
        }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int rr = c32_row(r, hi);
        const float lse_q =
            (*reinterpret_cast<const f32x4*>(lse_r + 8 * (r >> 2)))[r & 3];
        const float del_q =
            (*reinterpret_cast<const f32x4*>(del_r + 8 * (r >> 2)))[r & 3];
        float x = st[r] * scale2_ - lse_q;
        if constexpr (!DOC)
          if (need_mask) {
            const int q_g = qt * TILE + m32 * 32 + rr;
            x = attends(kv_g, q_g, window) ? x : -1e30f;
          }
        const float pval = __builtin_amdgcn_exp2f(x);
        st[r] = pval;
        dpt[r] = pval * __builtin_fmaf(dpt[r], scale, -del_q);
      }

      // dV += P^T·dO ; dK += dS^T·Q   (A rows = kv via swap; B from LDS^T)
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        short8 pa = c_to_afrag(st, kk);
        short8 dsa = c_to_afrag(dpt, kk);
        // NOTE: must stay fully unrolled — t indexes the accumulator
        // register arrays (guide rule 20: runtime indexing demotes them
        // to scratch; a partial-unroll experiment cost 576 B/lane)
#pragma unroll
        for (int t = 0; t < DT; ++t) {
          short8 dob = *reinterpret_cast<const short8*>(
              doT_lds + (t * 32 + lq) * LST + m32 * 32 + kk * 16 + hi * 8);
          short8 qb = *reinterpret_cast<const short8*>(
              qT_lds + (t * 32 + lq) * LST + m32 * 32 + kk * 16 + hi * 8);
          acc_dv[t] = MFMA32(pa, dob, acc_dv[t]);
          acc_dk[t] = MFMA32(dsa, qb, acc_dk[t]);
        }
      }
      __builtin_amdgcn_s_setprio(0);
    }
  }

  u16* dKp = dk + ((long long)b * S + kv0) * od + (long long)h * D;
  u16* dVp = dv + ((long long)b * S + kv0) * od + (long long)h * D;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int krow = c32_row(r, hi);
#pragma unroll
    for (int t = 0; t < DT; ++t) {
      dKp[(long long)krow * od + t * 32 + lq] = f32_to_bf16(acc_dk[t][r]);
      dVp[(long long)krow * od + t * 32 + lq] = f32_to_bf16(acc_dv[t][r]);
    }
  }
}

}  // namespace

extern "C" {

void acco_attn_bwd32_dq(const void* q, const void* k, const void* v,
                        const void* dO, const float* lse, const float* delta,
                        void* dq, int B, int S, int H, int Hkv, int D,
                        float scale, int window, long long q_rs,
                        long long kv_rs, long long do_rs, long long dq_rs,
                        const float* rope_cos, const float* rope_sin,
                        const int* doc_start, hipStream_t stream) {
  dim3 grid(block_order_grid(S / BT32, B, H));
  // doc_start given: the DOC build; a window >= S bounds nothing, and
  // capping it keeps doc_lo / doc_hi free of overflow
#define LQ(DD, DOC) hipLaunchKernelGGL((attn_bwd32_dq_kernel<DD, DOC>), grid, \
    dim3(512), Bwd32DqLds<DD>::bytes, stream, (const u16*)q, (const u16*)k, \
    (const u16*)v, (const u16*)dO, lse, delta, (u16*)dq, S, H, Hkv, scale, \
    DOC ? (window < S ? window : S) : window, q_rs, kv_rs, do_rs, dq_rs, \
    rope_cos, rope_sin, doc_start)
  if (doc_start != nullptr) {
    if (D == 64) LQ(64, true); else LQ(128, true);
  } else {
    if (D == 64) LQ(64, false); else LQ(128, false);
  }
#undef LQ
}

void acco_attn_bwd32_dkv(const void* q, const void* k, const void* v,
                         const void* dO, const float* lse,
                         const float* delta, void* dk, void* dv, int B,
                         int S, int H, int Hkv, int D, float scale,
                         int window, long long q_rs, long long kv_rs,
                         long long do_rs, const int* doc_end,
                         hipStream_t stream) {
  dim3 grid(block_order_grid(S / BT32, B, H));
#define LK(DD, DOC) hipLaunchKernelGGL((attn_bwd32_dkv_kernel<DD, DOC>), grid, \
    dim3(512), Bwd32DkvLds<DD>::bytes, stream, (const u16*)q, (const u16*)k, \
    (const u16*)v, (const u16*)dO, lse, delta, (u16*)dk, (u16*)dv, S, H, Hkv, \
    scale, DOC ? (window < S ? window : S) : window, q_rs, kv_rs, do_rs, \
    doc_end)
  if (doc_end != nullptr) {
    if (D == 64) LK(64, true); else LK(128, true);
  } else {
    if (D == 64) LK(64, false); else LK(128, false);
  }
#undef LK
}

}  // extern "C"
