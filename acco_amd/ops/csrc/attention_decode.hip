// Single-token (decode) attention against a KV cache for gfx950: one query
// token per sequence, q [B, H, D] bf16, caches [B, Hkv, Smax, D] bf16,
// cache_len int32 [B] on the device. The query of sequence b sits at position
// L - 1 and attends keys [max(0, L - window), L), L = clamp(cache_len[b], 0,
// Smax) (window 0 = none). cache_len is data: it is clamped, then only
// compared, and no row at or beyond L is ever loaded.
//
// Memory-bound work, so the structure follows the bytes:
//   - one workgroup serves all rep = H / Hkv query heads of one kv head, so
//     each K / V row is read once;
//   - D / 8 adjacent lanes own one key: each loads 16 bytes of the K row and
//     16 bytes of the V row straight from global memory to registers (no LDS
//     staging: every byte is used once), holds the matching 8 dims of all rep
//     queries in registers, and the partial dots are summed over the D / 8
//     lanes by xor shuffles; a wave covers 512 / D keys per step, two steps
//     are in flight;
//   - fp32 scores in the log2 domain, online softmax per lane group, P stays
//     fp32 (there is no second MFMA to round it for).
// The key range is split across gridDim.x workgroups (flash-decoding): split
// i owns keys [i * chunk, (i + 1) * chunk), a host function of (B * Hkv, Smax)
// only, since cache_len cannot be read without a sync. Every split stores an
// fp32 partial (m, l, o[D]) per head by ordinary stores, empty splits
// included (m = kNegBig, l = 0, o = 0), so the workspace is never zeroed; a
// second kernel combines the partials in split order. No atomics and no
// inter-workgroup hand-off: the result is the same bits on every run.
// The running max starts at the finite kNegBig, never -inf, so an empty group,
// wave or split merges as weight exp2(kNegBig - m) = 0 (or 1 against another
// empty one, times l = 0) and never as exp2(-inf - (-inf)). L = 0 gives o = 0.
//
// The split count is a guess that nobody has measured: about two workgroups
// per CU (512) over B * Hkv, at least 256 keys per split, at most 64 splits.
// Sizes tried so far: Smax 256 .. 4096 with B * Hkv 1 .. 64 (the tests and
// benchmarks/decode_micro.py), for correctness and one timing run only.

#include "common.h"
#include "kernels.h"

namespace {

using u16 = unsigned short;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr float kNegBig = -1e30f;
constexpr float kLog2e = 1.4426950408889634f;

ACCO_DEV float exp2_fast(float x) { return __builtin_amdgcn_exp2f(x); }

ACCO_DEV void unpack8(const uint4& raw, float* f) {
  const u16* p = reinterpret_cast<const u16*>(&raw);
#pragma unroll
  for (int i = 0; i < 8; ++i) f[i] = bf16_to_f32(p[i]);
}

// workspace layout, fp32: ml [B*H, n_split, 2] then o [B*H, n_split, D]
template <int D, int REP>
__global__ __launch_bounds__(kThreads)
void attn_decode_kernel(const u16* __restrict__ q,
                        const u16* __restrict__ k_cache,
                        const u16* __restrict__ v_cache,
                        const int* __restrict__ cache_len,
                        float* __restrict__ part_ml,
                        float* __restrict__ part_o, int Hkv, int Smax,
                        int window, int chunk, float scale_log2,
                        long long q_rs) {
  constexpr int G = D / 8;            // lanes per key row
  constexpr int NG = kThreads / G;    // key rows per block step
  constexpr int GPW = kWave / G;      // lane groups per wave
  const int split = blockIdx.x, n_split = gridDim.x;
  const int bk = blockIdx.y;          // b * Hkv + kv head
  const int b = bk / Hkv, kvh = bk % Hkv;
  const int tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave;
  const int g = tid / G, c8 = (tid % G) * 8;

  const int L = min(max(cache_len[b], 0), Smax);
  const int lo = window > 0 ? max(L - window, 0) : 0;
  const long long c0 = (long long)split * chunk;
  const int start = (int)max((long long)lo, min(c0, (long long)L));
  const int end = (int)min((long long)L, c0 + chunk);

  float qf[REP][8];
  const u16* qp = q + (long long)b * q_rs + (long long)kvh * REP * D + c8;
#pragma unroll
  for (int h = 0; h < REP; ++h)
    unpack8(*reinterpret_cast<const uint4*>(qp + h * D), qf[h]);

  float m[REP], l[REP], o[REP][8];
#pragma unroll
  for (int h = 0; h < REP; ++h) {
    m[h] = kNegBig;
    l[h] = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) o[h][i] = 0.f;
  }

  const long long base = (long long)bk * Smax * D + c8;
  auto step = [&](const uint4& kraw, const uint4& vraw) {
    float kf[8], vf[8];
    unpack8(kraw, kf);
    unpack8(vraw, vf);
#pragma unroll
    for (int h = 0; h < REP; ++h) {
      float a = 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i) a = __fmaf_rn(qf[h][i], kf[i], a);
#pragma unroll
      for (int off = G / 2; off > 0; off >>= 1) a += __shfl_xor(a, off);
      const float s = a * scale_log2;
      const float m_new = fmaxf(m[h], s);
      const float alpha = exp2_fast(m[h] - m_new);
      const float p = exp2_fast(s - m_new);
      m[h] = m_new;
      l[h] = __fmaf_rn(l[h], alpha, p);
#pragma unroll
      for (int i = 0; i < 8; ++i)
        o[h][i] = __fmaf_rn(o[h][i], alpha, p * vf[i]);
    }
  };

  // every j below satisfies start <= j < end <= L <= Smax
  int j = start + g;
  for (; j + NG < end; j += 2 * NG) {
    const long long r0 = base + (long long)j * D;
    const long long r1 = r0 + (long long)NG * D;
    const uint4 k0 = *reinterpret_cast<const uint4*>(k_cache + r0);
    const uint4 k1 = *reinterpret_cast<const uint4*>(k_cache + r1);
    const uint4 v0 = *reinterpret_cast<const uint4*>(v_cache + r0);
    const uint4 v1 = *reinterpret_cast<const uint4*>(v_cache + r1);
    step(k0, v0);
    step(k1, v1);
  }
  if (j < end) {
    const long long r0 = base + (long long)j * D;
    const uint4 k0 = *reinterpret_cast<const uint4*>(k_cache + r0);
    const uint4 v0 = *reinterpret_cast<const uint4*>(v_cache + r0);
    step(k0, v0);
  }

  // merge the lane groups of a wave (same dims, other keys): xor over the
  // group index bits, every lane ends with the wave's (m, l, o)
#pragma unroll
  for (int h = 0; h < REP; ++h) {
    float mw = m[h];
#pragma unroll
    for (int off = G; off < kWave; off <<= 1)
      mw = fmaxf(mw, __shfl_xor(mw, off));
    const float w = exp2_fast(m[h] - mw);
    float lw = l[h] * w;
#pragma unroll
    for (int off = G; off < kWave; off <<= 1) lw += __shfl_xor(lw, off);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      float x = o[h][i] * w;
#pragma unroll
      for (int off = G; off < kWave; off <<= 1) x += __shfl_xor(x, off);
      o[h][i] = x;
    }
    m[h] = mw;
    l[h] = lw;
  }
  static_assert(GPW >= 1 && NG % GPW == 0, "whole lane groups per wave");

  // the four waves meet in LDS; the block's partial goes out in wave order
  __shared__ float s_m[kWaves][REP], s_l[kWaves][REP];
  __shared__ float s_o[kWaves][REP][D];
  if (lane < G) {
#pragma unroll
    for (int h = 0; h < REP; ++h) {
      if (lane == 0) {
        s_m[wave][h] = m[h];
        s_l[wave][h] = l[h];
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) s_o[wave][h][c8 + i] = o[h][i];
    }
  }
  __syncthreads();
  const long long head0 = (long long)bk * REP;    // b * H + kvh * REP
  for (int t = tid; t < REP * D; t += kThreads) {
    const int h = t / D, d = t % D;
    float mb = s_m[0][h];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) mb = fmaxf(mb, s_m[w][h]);
    float lb = 0.f, ob = 0.f;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      const float wt = exp2_fast(s_m[w][h] - mb);
      lb = __fmaf_rn(s_l[w][h], wt, lb);
      ob = __fmaf_rn(s_o[w][h][d], wt, ob);
    }
    const long long slot = (head0 + h) * n_split + split;
    part_o[slot * D + d] = ob;
    if (d == 0) {
      part_ml[slot * 2] = mb;
      part_ml[slot * 2 + 1] = lb;
    }
  }
}

// o[b, h, :] = sum_i exp2(m_i - M) o_i / sum_i exp2(m_i - M) l_i over the
// splits i in order; l = 0 (no key at all) stores 0. One block per (b, h),
// one thread per dim.
__global__ void attn_decode_combine_kernel(const float* __restrict__ part_ml,
                                           const float* __restrict__ part_o,
                                           u16* __restrict__ o, int n_split,
                                           int D) {
  const long long bh = blockIdx.x;
  const int d = threadIdx.x;
  const float* ml = part_ml + bh * n_split * 2;
  float M = kNegBig;
  for (int i = 0; i < n_split; ++i) M = fmaxf(M, ml[2 * i]);
  float l = 0.f, acc = 0.f;
  for (int i = 0; i < n_split; ++i) {
    const float w = exp2_fast(ml[2 * i] - M);
    l = __fmaf_rn(ml[2 * i + 1], w, l);
    acc = __fmaf_rn(part_o[(bh * n_split + i) * D + d], w, acc);
  }
  o[bh * D + d] = f32_to_bf16(l > 0.f ? acc / l : 0.f);
}

template <int D>
void launch_decode(int rep, dim3 grid, hipStream_t stream, const u16* q,
                   const u16* kc, const u16* vc, const int* len, float* ml,
                   float* po, int Hkv, int Smax, int window, int chunk,
                   float scale_log2, long long q_rs) {
#define ACCO_DECODE_REP(R)                                                   \
  case R:                                                                    \
    hipLaunchKernelGGL((attn_decode_kernel<D, R>), grid, dim3(kThreads), 0,  \
                       stream, q, kc, vc, len, ml, po, Hkv, Smax, window,    \
                       chunk, scale_log2, q_rs);                             \
    break;
  switch (rep) {
    ACCO_DECODE_REP(1) ACCO_DECODE_REP(2) ACCO_DECODE_REP(3)
    ACCO_DECODE_REP(4) ACCO_DECODE_REP(5) ACCO_DECODE_REP(6)
    ACCO_DECODE_REP(7) ACCO_DECODE_REP(8)
    default: break;   // the binding admits 1 <= rep <= 8 only
  }
#undef ACCO_DECODE_REP
}

}  // namespace

extern "C" void acco_attn_decode_grid(long long BHkv, int Smax, int* n_split,
                                      int* chunk) {
  long long n = 512 / (BHkv > 0 ? BHkv : 1);
  const long long by_len = ((long long)Smax + 255) / 256;
  if (n > by_len) n = by_len;
  if (n > 64) n = 64;
  if (n < 1) n = 1;
  // whole 64-key steps per split; the last split may be short or empty
  long long c = (((long long)Smax + n - 1) / n + 63) / 64 * 64;
  if (c < 64) c = 64;
  *n_split = (int)n;
  *chunk = (int)c;
}

extern "C" void acco_attn_decode(const void* q, const void* k_cache,
                                 const void* v_cache, const int* cache_len,
                                 void* o, float* workspace, int B, int H,
                                 int Hkv, int D, int Smax, float scale,
                                 int window, long long q_rs,
                                 hipStream_t stream) {
  int n_split, chunk;
  acco_attn_decode_grid((long long)B * Hkv, Smax, &n_split, &chunk);
  float* ml = workspace;
  float* po = workspace + (long long)B * H * n_split * 2;
  const dim3 grid(n_split, B * Hkv);
  const float scale_log2 = scale * kLog2e;
  if (D == 64)
    launch_decode<64>(H / Hkv, grid, stream, (const u16*)q,
                      (const u16*)k_cache, (const u16*)v_cache, cache_len, ml,
                      po, Hkv, Smax, window, chunk, scale_log2, q_rs);
  else
    launch_decode<128>(H / Hkv, grid, stream, (const u16*)q,
                       (const u16*)k_cache, (const u16*)v_cache, cache_len,
                       ml, po, Hkv, Smax, window, chunk, scale_log2, q_rs);
  hipLaunchKernelGGL(attn_decode_combine_kernel, dim3(B * H), dim3(D), 0,
                     stream, ml, po, (u16*)o, n_split, D);
}
