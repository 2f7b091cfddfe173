// Rotary position embedding (HF-Llama rotate_half convention) fwd + bwd for
// gfx950. Operates on the projections' natural [B, S, H, D] contiguous
// layout (no transpose copies); cos/sin are HOST-precomputed fp32 tables
// [S, D] (guide Appendix B: no on-device sinf/cosf on the hot path).
// Forward:  y1 = x1*cos - x2*sin ; y2 = x2*cos + x1*sin   (x2 = x[d+D/2])
// Backward: rotation by -theta:  dx1 = dy1*cos + dy2*sin ;
//           dx2 = dy2*cos - dy1*sin.
// Also home of the KV-cache append of generation (kv_append_kernel), which
// rotates K at its absolute position with the same rot8.

#include "common.h"
#include "kernels.h"

namespace {

using u16 = unsigned short;

template <bool BWD>
__global__ void rope_kernel(const u16* __restrict__ x, u16* __restrict__ y,
                            const float* __restrict__ cos_t,
                            const float* __restrict__ sin_t,
                            long long total_q,   // B*S*H*(D/8)
                            int H, int D, int S,
                            long long row_stride) {  // elements per token row
  const long long i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long stride = (long long)gridDim.x * blockDim.x;
  const int qph = D / 8;                 // 4-pair quads per half-head
  for (long long i = i0; i < total_q; i += stride) {
    const int q = (int)(i % qph);        // which 4-pair group in the head
    long long th = i / qph;              // token*H + h
    const long long tok = th / H;
    const int h = (int)(th % H);
    const int s = (int)(tok % S);
    const long long base = tok * row_stride + (long long)h * D + q * 4;
    const long long base2 = base + D / 2;           // x2 offset
    ushort4 x1 = *reinterpret_cast<const ushort4*>(x + base);
    ushort4 x2 = *reinterpret_cast<const ushort4*>(x + base2);
    float4 c = *reinterpret_cast<const float4*>(cos_t + (long long)s * D + q * 4);
    float4 sn = *reinterpret_cast<const float4*>(sin_t + (long long)s * D + q * 4);
    float a[4] = {bf16_to_f32(x1.x), bf16_to_f32(x1.y), bf16_to_f32(x1.z),
                  bf16_to_f32(x1.w)};
    float b[4] = {bf16_to_f32(x2.x), bf16_to_f32(x2.y), bf16_to_f32(x2.z),
                  bf16_to_f32(x2.w)};
    float cc[4] = {c.x, c.y, c.z, c.w};
    float ss[4] = {sn.x, sn.y, sn.z, sn.w};
    u16 o1[4], o2[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float y1, y2;
      if constexpr (!BWD) {
        y1 = a[k] * cc[k] - b[k] * ss[k];
        y2 = b[k] * cc[k] + a[k] * ss[k];
      } else {
        y1 = a[k] * cc[k] + b[k] * ss[k];
        y2 = b[k] * cc[k] - a[k] * ss[k];
      }
      o1[k] = f32_to_bf16(y1);
      o2[k] = f32_to_bf16(y2);
    }
    *reinterpret_cast<ushort4*>(y + base) = make_ushort4(o1[0], o1[1], o1[2], o1[3]);
    *reinterpret_cast<ushort4*>(y + base2) = make_ushort4(o2[0], o2[1], o2[2], o2[3]);
  }
}

ACCO_DEV void rot8(uint4& v1, uint4& v2, const float* c, const float* s) {
  u16* a = reinterpret_cast<u16*>(&v1);
  u16* b = reinterpret_cast<u16*>(&v2);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const float x1 = bf16_to_f32(a[k]), x2 = bf16_to_f32(b[k]);
    // explicit contraction, the one rope_kernel<false> compiles to (sin
    // product rounded, cos product fused): outputs stay bit-equal to it
    a[k] = f32_to_bf16(__fmaf_rn(x1, c[k], -__fmul_rn(x2, s[k])));
    b[k] = f32_to_bf16(__fmaf_rn(x2, c[k], __fmul_rn(x1, s[k])));
  }
}

// Forward rotation of the q AND k sections of the packed [T, W] projection
// output IN PLACE, one launch. One thread owns 8 pairs of one head: a
// 16-byte access at d and one at d + D/2 (the separate q / k launches of
// rope_kernel moved the same bytes at ~1.3 TB/s with 8-byte accesses and
// 64-bit div/mod per item). All index math is 32-bit; heads [0, H) sit at
// q_off, heads [H, H+Hkv) at k_off; the V section is never touched.
__global__ __launch_bounds__(256)
void rope_qk_inplace_kernel(u16* __restrict__ qkv,
                            const float* __restrict__ cos_t,
                            const float* __restrict__ sin_t,
                            unsigned total,   // T*(H+Hkv)*(D/16)
                            unsigned H, unsigned Hkv, unsigned D, unsigned S,
                            long long W, long long q_off, long long k_off) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= total) return;
  const unsigned cph = D / 16;              // 8-pair chunks per head
  const unsigned ipt = (H + Hkv) * cph;     // items per token row
  const unsigned tok = i / ipt, r = i % ipt;
  const unsigned hh = r / cph, c8 = (r % cph) * 8;
  const unsigned s = tok % S;
  const long long sec = hh < H ? q_off + (long long)hh * D
                               : k_off + (long long)(hh - H) * D;
  u16* p1 = qkv + (long long)tok * W + sec + c8;
  u16* p2 = p1 + D / 2;
  uint4 v1 = *reinterpret_cast<const uint4*>(p1);
  uint4 v2 = *reinterpret_cast<const uint4*>(p2);
  const float4* cp = reinterpret_cast<const float4*>(cos_t + (size_t)s * D + c8);
  const float4* sp = reinterpret_cast<const float4*>(sin_t + (size_t)s * D + c8);
  const float4 c0 = cp[0], c1 = cp[1], s0 = sp[0], s1 = sp[1];
  const float cc[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
  const float ss[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
  rot8(v1, v2, cc, ss);
  *reinterpret_cast<uint4*>(p1) = v1;
  *reinterpret_cast<uint4*>(p2) = v2;
}

// KV-cache append: T new tokens per sequence from the projection's natural
// layout (q / k / v base pointers with a row stride each, so the packed
// q|k|v or k|v|q output and separate tensors are read in place) into the
// caches [B, Hkv, Smax, D]. Token t of sequence b goes to cache row
// p = clamp(cache_len[b], 0, Smax) + t; a row at or beyond Smax is dropped.
// cache_len is data: it is clamped, then only compared. With tables K is
// rotated by row p of the table (rot8: the bits a full forward computes for
// that position) and the rotated q goes to q_out [B, T, H, D]; a dropped
// token's q takes the table's last row (p < rows otherwise: rows >= Smax).
// Without tables K is copied and q is not touched (Hq = 0). One thread owns
// 8 pairs of one head, as in rope_qk_inplace_kernel.
__global__ __launch_bounds__(256)
void kv_append_kernel(const u16* __restrict__ q, const u16* __restrict__ k,
                      const u16* __restrict__ v, u16* __restrict__ q_out,
                      u16* __restrict__ k_cache, u16* __restrict__ v_cache,
                      const int* __restrict__ cache_len,
                      const float* __restrict__ cos_t,
                      const float* __restrict__ sin_t, unsigned total,
                      unsigned T, unsigned Hq, unsigned Hkv, unsigned D,
                      int Smax, int rows, long long q_rs, long long k_rs,
                      long long v_rs) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= total) return;
  const unsigned cph = D / 16;                  // 8-pair chunks per head
  const unsigned ipt = (Hq + 2 * Hkv) * cph;    // items per token
  const unsigned tok = i / ipt, r = i % ipt;
  const unsigned b = tok / T, t = tok % T;
  const unsigned hh = r / cph, c8 = (r % cph) * 8;
  const int len = min(max(cache_len[b], 0), Smax);
  const long long p = (long long)len + t;       // absolute position
  const bool is_q = hh < Hq, is_k = !is_q && hh < Hq + Hkv;
  if (!is_q && p >= Smax) return;               // dropped, never written
  const unsigned h = is_q ? hh : (is_k ? hh - Hq : hh - Hq - Hkv);
  const u16* src = is_q ? q + (long long)tok * q_rs
                 : is_k ? k + (long long)tok * k_rs
                        : v + (long long)tok * v_rs;
  src += (long long)h * D + c8;
  uint4 v1 = *reinterpret_cast<const uint4*>(src);
  uint4 v2 = *reinterpret_cast<const uint4*>(src + D / 2);
  if (cos_t != nullptr && (is_q || is_k)) {
    const size_t row = (size_t)min(p, (long long)rows - 1);
    const float4* cp = reinterpret_cast<const float4*>(cos_t + row * D + c8);
    const float4* sp = reinterpret_cast<const float4*>(sin_t + row * D + c8);
    const float4 c0 = cp[0], c1 = cp[1], s0 = sp[0], s1 = sp[1];
    const float cc[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
    const float ss[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
    rot8(v1, v2, cc, ss);
  }
  u16* dst = is_q ? q_out + ((long long)tok * Hq + h) * D
                  : (is_k ? k_cache : v_cache) +
                        (((long long)b * Hkv + h) * Smax + p) * D;
  dst += c8;
  *reinterpret_cast<uint4*>(dst) = v1;
  *reinterpret_cast<uint4*>(dst + D / 2) = v2;
}

}  // namespace

extern "C" void acco_kv_append(const void* q, const void* k, const void* v,
                               void* q_out, void* k_cache, void* v_cache,
                               const int* cache_len, const float* cos_t,
                               const float* sin_t, int B, int T, int H,
                               int Hkv, int D, int Smax, int table_rows,
                               long long q_rs, long long k_rs, long long v_rs,
                               hipStream_t stream) {
  // q is read and written only with tables; without them it is the caller's
  const int Hq = (cos_t != nullptr && q != nullptr) ? H : 0;
  const unsigned total = (unsigned)((long long)B * T * (Hq + 2 * Hkv) *
                                    (D / 16));
  if (total == 0) return;
  hipLaunchKernelGGL(kv_append_kernel, dim3((total + 255) / 256), dim3(256),
                     0, stream, (const u16*)q, (const u16*)k, (const u16*)v,
                     (u16*)q_out, (u16*)k_cache, (u16*)v_cache, cache_len,
                     cos_t, sin_t, total, (unsigned)T, (unsigned)Hq,
                     (unsigned)Hkv, (unsigned)D, Smax, table_rows, q_rs, k_rs,
                     v_rs);
}

extern "C" void acco_rope_qk_inplace(void* qkv, const float* cos_t,
                                     const float* sin_t, long long T, int S,
                                     int H, int Hkv, int D, long long W,
                                     long long q_off, long long k_off,
                                     hipStream_t stream) {
  const unsigned total = (unsigned)(T * (H + Hkv) * (D / 16));
  if (total == 0) return;
  hipLaunchKernelGGL(rope_qk_inplace_kernel, dim3((total + 255) / 256),
                     dim3(256), 0, stream, (u16*)qkv, cos_t, sin_t, total,
                     (unsigned)H, (unsigned)Hkv, (unsigned)D, (unsigned)S, W,
                     q_off, k_off);
}

extern "C" void acco_rope(const void* x, void* y, const float* cos_t,
                          const float* sin_t, long long B, int S, int H,
                          int D, bool bwd, long long row_stride,
                          hipStream_t stream) {
  const long long total_q = B * (long long)S * H * (D / 8);
  const int grid = elementwise_grid(total_q, 256);
  if (bwd)
    hipLaunchKernelGGL(rope_kernel<true>, dim3(grid), dim3(256), 0, stream,
                       (const u16*)x, (u16*)y, cos_t, sin_t, total_q, H, D, S,
                       row_stride);
  else
    hipLaunchKernelGGL(rope_kernel<false>, dim3(grid), dim3(256), 0, stream,
                       (const u16*)x, (u16*)y, cos_t, sin_t, total_q, H, D, S,
                       row_stride);
}
