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
//   - D / E adjacent lanes own one key, E = 8 dims per lane for a bf16 cache:
//     each loads 16 bytes of the K row and 16 bytes of the V row straight
//     from global memory to registers (no LDS staging: every byte is used
//     once), holds the matching E dims of all rep queries in registers, and
//     the partial dots are summed over the D / E lanes by xor shuffles; a
//     wave covers 64 E / D keys per step, two steps are in flight;
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
// An e4m3 cache (acco_kv_append_fp8) holds codes of one byte, row value =
// code * scale with k_scale / v_scale fp32 [B, Hkv, Smax]. The bytes halve,
// so the lanes regroup: a 16-byte load holds E = 16 dims, D / 16 adjacent
// lanes own one key and a wave covers 1024 / D keys per step. A lane then
// holds 16 dims of q and of o per head, 32 * REP registers: up to REP = 3
// that fits the 256 VGPRs, from REP = 4 it does not (the compiler parks the
// rest in AGPRs and, at REP = 8, in scratch), so those group sizes take E = 8
// dims per lane by 8-byte loads, the lane layout and register budget of the
// bf16 cache. Each lane group also loads its key's two scales (one address in
// all its lanes). The K scale multiplies the finished dot, s = (q . codes) *
// (k_scale * scale_log2); the V scale is folded into p once per key, o +=
// (p * v_scale) * code. No row at or beyond L is loaded, codes or scale.
//
// decode_body is the kernel for both caches; a Cache policy carries the
// element and load types, E, the unpack and whether rows have scales. The two
// __global__ wrappers differ in their build: attn_decode_fp8_kernel is built
// without the packed fp32 VALU ops (see attention_extend.hip), while
// attn_decode_kernel keeps the build it was measured with. The body is
// force-inlined and takes its caller's target features.
//
// The split count is a guess that nobody has measured: about two workgroups
// per CU (512) over B * Hkv, at least 256 keys per split, at most 64 splits.
// Sizes tried so far: Smax 256 .. 4096 with B * Hkv 1 .. 64 (the tests and
// benchmarks/decode_micro.py), for correctness and one timing run only.

#include "common.h"
#include <type_traits>

#include "kernels.h"
#include "quant_formats.h"

namespace {

using u16 = unsigned short;
using u8 = unsigned char;

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

// The end of both decode kernels: a lane holds (m, l, o[E dims]) per head for
// the keys its lane group took, G = D / E lanes per group, dims c0 .. c0 + E.
// Merges the groups of a wave, then the four waves through LDS, and stores
// the block's partial in wave order.
template <int D, int REP, int E>
ACCO_DEV void decode_finish(float (&m)[REP], float (&l)[REP],
                            float (&o)[REP][E], int c0, int bk, int split,
                            int n_split, float* __restrict__ part_ml,
                            float* __restrict__ part_o) {
  constexpr int G = D / E;
  constexpr int NG = kThreads / G;
  constexpr int GPW = kWave / G;
  const int tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave;
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
    for (int i = 0; i < E; ++i) {
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
      for (int i = 0; i < E; ++i) s_o[wave][h][c0 + i] = o[h][i];
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

// What a cache format brings to decode_body: the element and 16- or 8-byte
// load types of a row, E dims per lane, their widening to fp32, and whether
// rows carry scales.
struct Bf16Cache {
  using Elem = u16;
  using Raw = uint4;
  static constexpr int E = 8;
  static constexpr bool kScales = false;
  static ACCO_DEV void unpack(const Raw& raw, float* f) { unpack8(raw, f); }
};

template <int E_>
struct Fp8Cache {
  using Elem = u8;
  using Raw = typename std::conditional<E_ == 16, uint4, uint2>::type;
  static constexpr int E = E_;
  static constexpr bool kScales = true;
  static ACCO_DEV void unpack(const Raw& raw, float* f) {
    e4m3::unpack_fp8<E>(raw, f);
  }
};

// workspace layout, fp32: ml [B*H, n_split, 2] then o [B*H, n_split, D].
// k_scale / v_scale are read only if Cache::kScales.
template <class Cache, int D, int REP>
ACCO_DEV void decode_body(const u16* __restrict__ q,
                          const typename Cache::Elem* __restrict__ k_cache,
                          const typename Cache::Elem* __restrict__ v_cache,
                          const float* __restrict__ k_scale,
                          const float* __restrict__ v_scale,
                          const int* __restrict__ cache_len,
                          float* __restrict__ part_ml,
                          float* __restrict__ part_o, int Hkv, int Smax,
                          int window, int chunk, float scale_log2,
                          long long q_rs) {
  using Raw = typename Cache::Raw;
  constexpr int E = Cache::E;
  constexpr int G = D / E;            // lanes per key row
  constexpr int NG = kThreads / G;    // key rows per block step
  const int split = blockIdx.x, n_split = gridDim.x;
  const int bk = blockIdx.y;          // b * Hkv + kv head
  const int b = bk / Hkv, kvh = bk % Hkv;
  const int tid = threadIdx.x;
  const int g = tid / G, ce = (tid % G) * E;

  const int L = min(max(cache_len[b], 0), Smax);
  const int lo = window > 0 ? max(L - window, 0) : 0;
  const long long c0 = (long long)split * chunk;
  const int start = (int)max((long long)lo, min(c0, (long long)L));
  const int end = (int)min((long long)L, c0 + chunk);

  float qf[REP][E];
  const u16* qp = q + (long long)b * q_rs + (long long)kvh * REP * D + ce;
#pragma unroll
  for (int h = 0; h < REP; ++h)
#pragma unroll
    for (int i = 0; i < E; i += 8)
      unpack8(*reinterpret_cast<const uint4*>(qp + h * D + i), qf[h] + i);

  float m[REP], l[REP], o[REP][E];
#pragma unroll
  for (int h = 0; h < REP; ++h) {
    m[h] = kNegBig;
    l[h] = 0.f;
#pragma unroll
    for (int i = 0; i < E; ++i) o[h][i] = 0.f;
  }

  const long long srow = (long long)bk * Smax;    // the pair's first row
  const long long base = srow * D + ce;
  // one key: ks and vs are its scales (unused without)
  auto step = [&](const Raw& kraw, const Raw& vraw, float ks, float vs)
                  __attribute__((always_inline)) {
    float kf[E], vf[E];
    Cache::unpack(kraw, kf);
    Cache::unpack(vraw, vf);
    float kss = scale_log2;
    if constexpr (Cache::kScales) kss = ks * scale_log2;
#pragma unroll
    for (int h = 0; h < REP; ++h) {
      float a = 0.f;
#pragma unroll
      for (int i = 0; i < E; ++i) a = __fmaf_rn(qf[h][i], kf[i], a);
#pragma unroll
      for (int off = G / 2; off > 0; off >>= 1) a += __shfl_xor(a, off);
      const float s = a * kss;
      const float m_new = fmaxf(m[h], s);
      const float alpha = exp2_fast(m[h] - m_new);
      const float p = exp2_fast(s - m_new);
      m[h] = m_new;
      l[h] = __fmaf_rn(l[h], alpha, p);
      float pv = p;
      if constexpr (Cache::kScales) pv = p * vs;
#pragma unroll
      for (int i = 0; i < E; ++i)
        o[h][i] = __fmaf_rn(o[h][i], alpha, pv * vf[i]);
    }
  };

  // every j below satisfies start <= j < end <= L <= Smax
  int j = start + g;
  for (; j + NG < end; j += 2 * NG) {
    const long long r0 = base + (long long)j * D;
    const long long r1 = r0 + (long long)NG * D;
    const Raw k0 = *reinterpret_cast<const Raw*>(k_cache + r0);
    const Raw k1 = *reinterpret_cast<const Raw*>(k_cache + r1);
    const Raw v0 = *reinterpret_cast<const Raw*>(v_cache + r0);
    const Raw v1 = *reinterpret_cast<const Raw*>(v_cache + r1);
    float ks0 = 0.f, ks1 = 0.f, vs0 = 0.f, vs1 = 0.f;
    if constexpr (Cache::kScales) {
      ks0 = k_scale[srow + j], ks1 = k_scale[srow + j + NG];
      vs0 = v_scale[srow + j], vs1 = v_scale[srow + j + NG];
    }
    step(k0, v0, ks0, vs0);
    step(k1, v1, ks1, vs1);
  }
  if (j < end) {
    const long long r0 = base + (long long)j * D;
    const Raw k0 = *reinterpret_cast<const Raw*>(k_cache + r0);
    const Raw v0 = *reinterpret_cast<const Raw*>(v_cache + r0);
    float ks0 = 0.f, vs0 = 0.f;
    if constexpr (Cache::kScales)
      ks0 = k_scale[srow + j], vs0 = v_scale[srow + j];
    step(k0, v0, ks0, vs0);
  }

  decode_finish<D, REP, E>(m, l, o, ce, bk, split, n_split, part_ml, part_o);
}

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
  decode_body<Bf16Cache, D, REP>(q, k_cache, v_cache, nullptr, nullptr,
                                 cache_len, part_ml, part_o, Hkv, Smax,
                                 window, chunk, scale_log2, q_rs);
}

// The host pass does not know the feature, hence the guard.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(                                      \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

template <int D, int REP, int E = (REP <= 3 ? 16 : 8)>
__global__ __launch_bounds__(kThreads)
void attn_decode_fp8_kernel(const u16* __restrict__ q,
                            const u8* __restrict__ k_cache,
                            const u8* __restrict__ v_cache,
                            const float* __restrict__ k_scale,
                            const float* __restrict__ v_scale,
                            const int* __restrict__ cache_len,
                            float* __restrict__ part_ml,
                            float* __restrict__ part_o, int Hkv, int Smax,
                            int window, int chunk, float scale_log2,
                            long long q_rs) {
  decode_body<Fp8Cache<E>, D, REP>(q, k_cache, v_cache, k_scale, v_scale,
                                   cache_len, part_ml, part_o, Hkv, Smax,
                                   window, chunk, scale_log2, q_rs);
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

// o[row, :] = sum_i exp2(m_i - M) o_i / sum_i exp2(m_i - M) l_i over the
// splits i in order; l = 0 (no key at all) stores 0. One block per row of o
// ((b, h) here, (b, t, h) in attention_extend.hip), one thread per dim.
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

namespace {

// both entry points: k_scale == nullptr is the bf16 cache
void launch_decode(const void* q, const void* k_cache, const void* v_cache,
                   const float* k_scale, const float* v_scale,
                   const int* cache_len, void* o, float* workspace, int B,
                   int H, int Hkv, int D, int Smax, float scale, int window,
                   long long q_rs, hipStream_t stream) {
  int n_split, chunk;
  acco_attn_decode_grid((long long)B * Hkv, Smax, &n_split, &chunk);
  float* ml = workspace;
  float* po = workspace + (long long)B * H * n_split * 2;
  const dim3 grid(n_split, B * Hkv);
  const float scale_log2 = scale * kLog2e;
#define ACCO_DECODE_REP(DD, R)                                                \
  case R:                                                                     \
    if (k_scale == nullptr)                                                   \
      hipLaunchKernelGGL((attn_decode_kernel<DD, R>), grid, dim3(kThreads),   \
                         0, stream, (const u16*)q, (const u16*)k_cache,       \
                         (const u16*)v_cache, cache_len, ml, po, Hkv, Smax,   \
                         window, chunk, scale_log2, q_rs);                    \
    else                                                                      \
      hipLaunchKernelGGL((attn_decode_fp8_kernel<DD, R>), grid,               \
                         dim3(kThreads), 0, stream, (const u16*)q,            \
                         (const u8*)k_cache, (const u8*)v_cache, k_scale,     \
                         v_scale, cache_len, ml, po, Hkv, Smax, window,       \
                         chunk, scale_log2, q_rs);                            \
    break;
#define ACCO_DECODE(DD)                                                       \
  switch (H / Hkv) {                                                          \
    ACCO_DECODE_REP(DD, 1) ACCO_DECODE_REP(DD, 2) ACCO_DECODE_REP(DD, 3)      \
    ACCO_DECODE_REP(DD, 4) ACCO_DECODE_REP(DD, 5) ACCO_DECODE_REP(DD, 6)      \
    ACCO_DECODE_REP(DD, 7) ACCO_DECODE_REP(DD, 8)                             \
    default: break;   /* the binding admits 1 <= rep <= 8 only */             \
  }
  if (D == 64) ACCO_DECODE(64)
  else ACCO_DECODE(128)
#undef ACCO_DECODE
#undef ACCO_DECODE_REP
  acco_attn_split_combine(ml, po, o, (long long)B * H, n_split, D, stream);
}

}  // namespace

extern "C" void acco_attn_decode(const void* q, const void* k_cache,
                                 const void* v_cache, const int* cache_len,
                                 void* o, float* workspace, int B, int H,
                                 int Hkv, int D, int Smax, float scale,
                                 int window, long long q_rs,
                                 hipStream_t stream) {
  launch_decode(q, k_cache, v_cache, nullptr, nullptr, cache_len, o,
                workspace, B, H, Hkv, D, Smax, scale, window, q_rs, stream);
}

extern "C" void acco_attn_decode_fp8(const void* q, const void* k_cache,
                                     const void* v_cache,
                                     const float* k_scale,
                                     const float* v_scale,
                                     const int* cache_len, void* o,
                                     float* workspace, int B, int H, int Hkv,
                                     int D, int Smax, float scale, int window,
                                     long long q_rs, hipStream_t stream) {
  launch_decode(q, k_cache, v_cache, k_scale, v_scale, cache_len, o,
                workspace, B, H, Hkv, D, Smax, scale, window, q_rs, stream);
}

extern "C" void acco_attn_split_combine(const float* part_ml,
                                        const float* part_o, void* o,
                                        long long rows, int n_split, int D,
                                        hipStream_t stream) {
  hipLaunchKernelGGL(attn_decode_combine_kernel, dim3((unsigned)rows),
                     dim3(D), 0, stream, part_ml, part_o, (u16*)o, n_split,
                     D);
}
