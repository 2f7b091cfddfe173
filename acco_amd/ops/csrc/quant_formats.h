// What the kernels that read one quantised format share: for e4m3 the widening
// of codes to fp32 (the fp8 KV cache of attention_decode.hip) and to the bf16
// MFMA operand (attention_extend.hip, linear_w8.hip, gemm_w8.hip), for MXFP4
// the bf16 convert of linear_w4.hip and gemm_w4.hip; and `finish`, the one
// place a finished dot product of a weight-only kernel becomes an output
// element. v_cvt_pk_f32_fp8 is named here and nowhere else. Included inside
// the no-packed-fp32-ops region of some of those files (linear_skinny.h says
// why), so this header includes nothing but common.h.
#pragma once

#include "common.h"

namespace e4m3 {

using short8 = __attribute__((ext_vector_type(8))) short;

// E e4m3 codes (E / 4 dwords) -> fp32 by v_cvt_pk_f32_fp8, two values per
// instruction
template <int E, class Raw>
ACCO_DEV void unpack_fp8(const Raw& raw, float* f) {
  const int* w = reinterpret_cast<const int*>(&raw);
#pragma unroll
  for (int i = 0; i < E / 4; ++i) {
    const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8(w[i], false);
    const auto hi = __builtin_amdgcn_cvt_pk_f32_fp8(w[i], true);
    f[4 * i] = lo[0];
    f[4 * i + 1] = lo[1];
    f[4 * i + 2] = hi[0];
    f[4 * i + 3] = hi[1];
  }
}

// 16 e4m3 codes -> 16 bf16, the B fragments of two MFMAs. An e4m3 value has
// four significant bits, so the high half of its fp32 is the value itself in
// bf16.
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

// The same by shift and mask, for the staging of attention_extend.hip: with
// the v_perm_b32 form one of its kernels' register counts moved (RESULTS.md).
ACCO_DEV void codes_to_bf16_shift(const uint4& raw, short8& lo, short8& hi) {
  const int* w = reinterpret_cast<const int*>(&raw);
  unsigned out[8];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const auto a = __builtin_amdgcn_cvt_pk_f32_fp8(w[i], false);
    const auto b = __builtin_amdgcn_cvt_pk_f32_fp8(w[i], true);
    out[2 * i] = (__float_as_uint(a[0]) >> 16) |
                 (__float_as_uint(a[1]) & 0xffff0000u);
    out[2 * i + 1] = (__float_as_uint(b[0]) >> 16) |
                     (__float_as_uint(b[1]) & 0xffff0000u);
  }
  unsigned* l = reinterpret_cast<unsigned*>(&lo);
  unsigned* h = reinterpret_cast<unsigned*>(&hi);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    l[i] = out[i];
    h[i] = out[4 + i];
  }
}

// the row scale multiplies the finished sum and never enters the K loop
struct Finish {
  const float* scale;
  const unsigned short* bias;
  ACCO_DEV unsigned short operator()(float dot, int n) const {
    const float b = bias != nullptr ? bf16_to_f32(bias[n]) : 0.f;
    return f32_to_bf16(__fmaf_rn(dot, scale[n], b));
  }
};

}  // namespace e4m3

namespace mxfp4 {

using short8 = __attribute__((ext_vector_type(8))) short;

// 8 codes (one dword, k ascending from the low nibble) times 2^(s - 127) ->
// 8 bf16, the B fragment of one MFMA; `scale` is s << 23 read as fp32
ACCO_DEV short8 codes_to_bf16(unsigned dw, float scale) {
  union { decltype(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(0u, 1.f, 0)) v;
          unsigned u; } p[4];
  p[0].v = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(dw, scale, 0);
  p[1].v = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(dw, scale, 1);
  p[2].v = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(dw, scale, 2);
  p[3].v = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(dw, scale, 3);
  short8 out;
  unsigned* o = reinterpret_cast<unsigned*>(&out);
#pragma unroll
  for (int i = 0; i < 4; ++i) o[i] = p[i].u;
  return out;
}

struct Finish {
  const unsigned short* bias;
  ACCO_DEV unsigned short operator()(float dot, int n) const {
    const float b = bias != nullptr ? bf16_to_f32(bias[n]) : 0.f;
    return f32_to_bf16(dot + b);
  }
};

}  // namespace mxfp4
