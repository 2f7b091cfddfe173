// What sample.hip and spec_verify.hip share: the keying of bf16 logits, the
// walk over a row, the Philox draw and the mass of an element. Together with
// torch_ref.sample_logits / spec_verify these define what the sampler and the
// verifier agree on, so there is one copy. spec_verify.hip includes this
// inside its no-packed-fp32-ops region, so the header includes nothing but
// common.h and <cstdint>.
//
// Values and keys. On load -0 becomes +0, +-inf the largest finite bf16 of
// that sign, and NaN the lowest key (0), which no threshold admits. Every
// other value maps to an order-preserving 16-bit key (sign bit flipped for
// x >= 0, all bits flipped for x < 0), so finite values have keys in
// [0x0080, 0xff7f]. Comparisons of keys are integer compares and exact.
#pragma once

#include <cstdint>

#include "common.h"

namespace sampling {

using u16 = unsigned short;
using u32 = unsigned int;
using u64 = unsigned long long;

constexpr int BLOCK = 1024;
constexpr int NWAVE = BLOCK / 64;
constexpr u32 kKeyMin = 0x0080u;  // key of the lowest finite bf16
constexpr u32 kKeyZero = 0x8000u;

typedef unsigned int w4_ __attribute__((ext_vector_type(4)));

ACCO_DEV u32 load_key(u32 bits) {
  bits &= 0xffffu;
  const u32 mag = bits & 0x7fffu;
  if (mag > 0x7f80u) return 0u;                      // NaN: below everything
  if (mag == 0u) return kKeyZero;                    // -0 -> +0
  if (mag == 0x7f80u) bits = (bits & 0x8000u) | 0x7f7fu;   // +-inf clamped
  return (bits & 0x8000u) ? (~bits & 0xffffu) : (bits | 0x8000u);
}

ACCO_DEV u16 key_bits(u32 key) {
  return (u16)((key & 0x8000u) ? (key ^ 0x8000u) : (~key & 0xffffu));
}

ACCO_DEV float key_value(u32 key) { return bf16_to_f32(key_bits(key)); }

// f(bits, index) for every element of the row, each exactly once. Nothing is
// asked of the row's address: a scalar head up to the first 16-byte boundary,
// aligned 16-byte vectors and a scalar tail of < 8 elements.
template <class F>
ACCO_DEV void for_each_elem(const u16* __restrict__ row, int V, F&& f) {
  const int tid = threadIdx.x;
  int peel = (int)(((16u - (u32)((uintptr_t)row & 15u)) & 15u) >> 1);
  if (peel > V) peel = V;
  const int nvec = (V - peel) / 8;
  const int tail = peel + nvec * 8;
  if (tid < peel) f((u32)row[tid], tid);
  const w4_* body = reinterpret_cast<const w4_*>(row + peel);
  // one vector per thread and iteration: four loads in flight measured the
  // same (the passes are bound by the CU's VALU, not by load latency)
  for (int c = tid; c < nvec; c += BLOCK) {
    const w4_ q = body[c];
    const int base = peel + c * 8;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      f(q[k] & 0xffffu, base + 2 * k);
      f(q[k] >> 16, base + 2 * k + 1);
    }
  }
  if (tail + tid < V) f((u32)row[tail + tid], tail + tid);
}

// exp((x - max) / T), the same pure function of the element in every pass.
// c2 = log2(e) / T, the argument is <= 0, so the result is <= 1.
ACCO_DEV float mass(u32 key, float vmax, float c2) {
  return __builtin_amdgcn_exp2f((key_value(key) - vmax) * c2);
}

// The mass as 64-bit fixed point, truncated: integer sums of these are exact
// in any order.
ACCO_DEV u64 fixed_mass(u32 key, float vmax, float c2, float mscale) {
  return (u64)(mass(key, vmax, c2) * mscale);
}

// word 0 of Philox4x32-10 at counter (c0, c1, c2, c3) under key (k0, k1)
ACCO_DEV u32 philox_word0(u32 c0, u32 c1, u32 c2, u32 c3, u32 k0, u32 k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    if (r) { k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
    const u64 p0 = (u64)0xD2511F53u * c0;
    const u64 p1 = (u64)0xCD9E8D57u * c2;
    const u32 n0 = (u32)(p1 >> 32) ^ c1 ^ k0;
    const u32 n2 = (u32)(p0 >> 32) ^ c3 ^ k1;
    c1 = (u32)p1;
    c3 = (u32)p0;
    c0 = n0;
    c2 = n2;
  }
  return c0;
}

// u = (r + 0.5) · 2^-23, r the top 23 bits of the word.
// (2r + 1) · 2^-24 = (r + 0.5) · 2^-23, exact: 2r + 1 < 2^24
ACCO_DEV float uniform01(u32 word) {
  return (float)(2u * (word >> 9) + 1u) * 5.9604644775390625e-08f;
}

ACCO_DEV float gumbel(u32 word) { return -logf(-logf(uniform01(word))); }

// the running argmax: highest score, lowest index on ties
struct Best {
  float score;
  int idx;
};

ACCO_DEV void better(Best& a, float score, int idx) {
  if (score > a.score || (score == a.score && idx < a.idx)) {
    a.score = score;
    a.idx = idx;
  }
}

// What both entry points derive from (temperature, V) on the host.
struct SamplingParams {
  bool greedy;
  float T, c2, mscale;
};

inline SamplingParams sampling_params(float temperature, int V) {
  SamplingParams s;
  s.greedy = temperature == 0.0f;
  s.T = s.greedy ? 1.0f : temperature;
  // log2(e) / T rounded once: the exponent of a mass is one product away
  s.c2 = (float)(1.4426950408889634 / (double)s.T);
  // V masses of at most 2^shift each sum below 2^62
  int bits = 0;
  while ((1ll << bits) < (long long)V) ++bits;
  const int shift = 62 - bits < 40 ? 62 - bits : 40;
  s.mscale = ldexpf(1.0f, shift);
  return s;
}

}  // namespace sampling
