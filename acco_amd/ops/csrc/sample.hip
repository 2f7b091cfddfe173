// On-device token sampling for gfx950: temperature, top-k, top-p and one
// Gumbel-max draw per row of bf16 logits, so a generation loop never copies
// logits to the host. torch_ref.sample_logits is the executable definition.
//
// Values and keys. On load -0 becomes +0, +-inf the largest finite bf16 of
// that sign, and NaN the lowest key (0), which no threshold admits. Every
// other value maps to an order-preserving 16-bit key (sign bit flipped for
// x >= 0, all bits flipped for x < 0), so finite values have keys in
// [0x0080, 0xff7f]. top-k and top-p thresholds are keys: selection compares
// integers and is exact.
//
// One 1024-thread workgroup per row; the row (256 KB at V = 128k) is re-read
// from L2 by each pass:
//   1  max key                                           (always)
//   2  count histogram of the key's high byte, 3 of the low byte inside the
//      threshold bin -> thr_k                            (top-k only)
//   4  mass histogram of the high byte over the top-k survivors, 5 of the low
//      byte inside the threshold bin -> thr_p            (top-p only)
//   6  over x >= thr = max(thr_k, thr_p): n_kept, the kept mass, and the
//      argmax of x / T + g_i (greedy: of x), lowest index on ties
// Histograms live in LDS and are filled with integer atomics: counts as
// uint32, masses as 64-bit fixed point (exp((x - max) / T) · 2^shift,
// truncated), so every sum is order-independent and the outputs are bitwise
// reproducible. No float atomics, no global workspace, nothing crosses
// workgroups. The high byte of a bf16 key is sign + exponent: a wave's 64
// lanes hit a handful of bins, so each histogram has one copy per lane group
// (32 for counts, 16 for masses, row stride 257 so that copies of one bin lie
// on distinct banks) and the copies are summed before the suffix scan.
// The pass structure and the one-workgroup-per-row shape are first guesses;
// RESULTS.md ("On-device sampling") has what they cost.
//
// g_i = -log(-log(u_i)), u_i = (r_i + 0.5) · 2^-23, r_i the top 23 bits of
// word 0 of Philox4x32-10 at counter (i, row, step_lo, step_hi) under key
// (seed_lo, seed_hi). Only kept elements draw. The draw is a pure function of
// (logits, T, top_k, top_p, seed, step, row).
//
// Alignment: nothing is asked of the base or the row stride. Each row is
// split by its own address into a scalar head up to the first 16-byte
// boundary, aligned 16-byte vectors and a scalar tail of < 8 elements.

#include <cstdint>

#include "common.h"
#include "kernels.h"

namespace {

using u16 = unsigned short;
using u32 = unsigned int;
using u64 = unsigned long long;

constexpr int BLOCK = 1024;
constexpr int NWAVE = BLOCK / 64;
constexpr int BINS = 256;
constexpr int HSTRIDE = BINS + 1;
constexpr int CNT_COPIES = 32;    // uint32 view of the histogram buffer
constexpr int MASS_COPIES = 16;   // uint64 view of the same bytes
constexpr int HIST_U64 = MASS_COPIES * HSTRIDE;
static_assert(CNT_COPIES * HSTRIDE <= 2 * HIST_U64, "count view fits");
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

// f(bits, index) for every element of the row, each exactly once
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

// exp((x - max) / T) as fixed point; the same pure function of the element
// in every pass. c2 = log2(e) / T, arg <= 0, so the result is <= mscale.
ACCO_DEV u64 fixed_mass(u32 key, float vmax, float c2, float mscale) {
  const float e = __builtin_amdgcn_exp2f((key_value(key) - vmax) * c2);
  return (u64)(e * mscale);
}

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

ACCO_DEV float gumbel(u32 word) {
  // (2r + 1) · 2^-24 = (r + 0.5) · 2^-23, exact: 2r + 1 < 2^24
  const float u = (float)(2u * (word >> 9) + 1u) * 5.9604644775390625e-08f;
  return -logf(-logf(u));
}

// One histogram level. Elements with key >= min_key (and, at level 1, with
// high byte hi_bin) add their weight (1, or their fixed-point mass) to the
// bin of their high (level 0) or low (level 1) byte; suf[t] becomes the sum
// of bins >= t (suf[256] = 0). Ends on a barrier.
template <bool MASS>
ACCO_DEV void fill_level(const u16* __restrict__ row, int V, int level,
                         u32 hi_bin, u32 min_key, float vmax, float c2,
                         float mscale, u64* hist, u64* suf) {
  const int tid = threadIdx.x;
  for (int i = tid; i < HIST_U64; i += BLOCK) hist[i] = 0ull;
  __syncthreads();
  u32* cnt = reinterpret_cast<u32*>(hist);
  const int lane = tid & 63;
  for_each_elem(row, V, [&](u32 bits, int) {
    const u32 key = load_key(bits);
    if (key < min_key) return;
    if (level == 1 && (key >> 8) != hi_bin) return;
    const u32 bin = level == 0 ? (key >> 8) : (key & 0xffu);
    if (MASS)
      atomicAdd(&hist[(lane & (MASS_COPIES - 1)) * HSTRIDE + bin],
                fixed_mass(key, vmax, c2, mscale));
    else
      atomicAdd(&cnt[(lane & (CNT_COPIES - 1)) * HSTRIDE + bin], 1u);
  });
  __syncthreads();
  u64 s = 0ull;
  if (tid < BINS) {
    if (MASS)
      for (int c = 0; c < MASS_COPIES; ++c) s += hist[c * HSTRIDE + tid];
    else
      for (int c = 0; c < CNT_COPIES; ++c) s += cnt[c * HSTRIDE + tid];
    suf[tid] = s;
  }
  if (tid == BINS) suf[BINS] = 0ull;
  __syncthreads();
  // suffix sums, integer: any order gives the same bits
  for (int off = 1; off < BINS; off <<= 1) {
    u64 o = 0ull;
    if (tid < BINS && tid + off < BINS) o = suf[tid + off];
    __syncthreads();
    if (tid < BINS) { s += o; suf[tid] = s; }
    __syncthreads();
  }
}

// The largest bin t with above + suf[t] >= target, the same in every thread;
// `above` grows by suf[t + 1], the weight of the bins beyond t. Needs
// above + suf[0] >= target >= 1 (then exactly one t qualifies). Ends on a
// barrier: suf and found may be rewritten at once.
ACCO_DEV u32 search_level(const u64* suf, u32* found, u64 target,
                          u64& above) {
  const int tid = threadIdx.x;
  if (tid < BINS && above + suf[tid] >= target &&
      (tid == BINS - 1 || above + suf[tid + 1] < target))
    *found = (u32)tid;
  __syncthreads();
  const u32 bin = *found;
  above += suf[bin + 1];
  __syncthreads();
  return bin;
}

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

__global__ __launch_bounds__(BLOCK) void sample_kernel(
    const u16* __restrict__ logits, long long row_stride, int V, float T,
    float c2, float mscale, bool greedy, int top_k, double top_p, u64 seed,
    u64 step, unsigned char* __restrict__ done, long long eos_id,
    long long* __restrict__ token, float* __restrict__ logprob,
    u16* __restrict__ thr_out, int* __restrict__ n_kept) {
  __shared__ u64 hist[HIST_U64];
  __shared__ u64 suf[BINS + 1];
  __shared__ u32 found;
  __shared__ u32 w_key[NWAVE];
  __shared__ u32 w_cnt[NWAVE];
  __shared__ u64 w_mass[NWAVE];
  __shared__ float w_score[NWAVE];
  __shared__ int w_idx[NWAVE];

  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  if (done != nullptr && done[b] != 0) {       // block-uniform
    if (tid == 0) {
      token[b] = eos_id;
      logprob[b] = 0.0f;
      thr_out[b] = 0;
      n_kept[b] = 0;
    }
    return;
  }
  const u16* row = logits + (long long)b * row_stride;

  // ---- pass 1: the largest key
  u32 kmax = 0u;
  for_each_elem(row, V, [&](u32 bits, int) {
    const u32 key = load_key(bits);
    kmax = key > kmax ? key : kmax;
  });
  for (int off = 32; off > 0; off >>= 1) {
    const u32 o = __shfl_xor(kmax, off, 64);
    kmax = o > kmax ? o : kmax;
  }
  if ((tid & 63) == 0) w_key[tid >> 6] = kmax;
  if (tid == 0) found = 0u;
  __syncthreads();
  for (int w = 0; w < NWAVE; ++w) kmax = w_key[w] > kmax ? w_key[w] : kmax;
  if (kmax == 0u) {                            // no finite logit in the row
    if (tid == 0) {
      token[b] = 0;
      logprob[b] = 0.0f;
      thr_out[b] = key_bits(kKeyMin);
      n_kept[b] = 0;
      if (done != nullptr) done[b] = (unsigned char)(eos_id == 0);
    }
    return;
  }
  const float vmax = key_value(kmax);

  // ---- thresholds
  u32 thr = kKeyMin;
  if (!greedy && top_k >= 1 && top_k < V) {
    // NaN counts as the lowest value: key 0, bin 0, so the V elements of the
    // histogram always reach top_k < V
    const u64 target = (u64)top_k;
    u64 above = 0ull;
    fill_level<false>(row, V, 0, 0u, 0u, vmax, c2, mscale, hist, suf);
    const u32 hi = search_level(suf, &found, target, above);
    fill_level<false>(row, V, 1, hi, 0u, vmax, c2, mscale, hist, suf);
    const u32 lo = search_level(suf, &found, target, above);
    const u32 t = (hi << 8) | lo;
    thr = t > thr ? t : thr;                   // never admits NaN
  }
  if (!greedy && top_p < 1.0) {
    // masses of the top-k survivors only: thr_p >= thr_k by construction
    u64 above = 0ull;
    fill_level<true>(row, V, 0, 0u, thr, vmax, c2, mscale, hist, suf);
    const u64 total = suf[0];                  // >= mscale: the max is in it
    u64 target = (u64)ceil((double)total * top_p);
    target = target < 1ull ? 1ull : target;    // at least one token
    target = target > total ? total : target;
    const u32 hi = search_level(suf, &found, target, above);
    fill_level<true>(row, V, 1, hi, thr, vmax, c2, mscale, hist, suf);
    const u32 lo = search_level(suf, &found, target, above);
    const u32 t = (hi << 8) | lo;
    thr = t > thr ? t : thr;
  }

  // ---- last pass: count, mass and the winner among x >= thr
  u32 cnt = 0u;
  u64 mass = 0ull;
  Best best = {-INFINITY, 0x7fffffff};
  const u32 k0 = (u32)seed, k1 = (u32)(seed >> 32);
  const u32 s0 = (u32)step, s1 = (u32)(step >> 32);
  for_each_elem(row, V, [&](u32 bits, int i) {
    const u32 key = load_key(bits);
    if (key < thr) return;
    cnt += 1u;
    mass += fixed_mass(key, vmax, c2, mscale);
    const float x = key_value(key);
    const float score =
        greedy ? x
               : x / T + gumbel(philox_word0((u32)i, (u32)b, s0, s1, k0, k1));
    better(best, score, i);
  });
  for (int off = 32; off > 0; off >>= 1) {
    cnt += __shfl_down(cnt, off, 64);
    mass += __shfl_down(mass, off, 64);
    const float so = __shfl_down(best.score, off, 64);
    const int io = __shfl_down(best.idx, off, 64);
    better(best, so, io);
  }
  if ((tid & 63) == 0) {
    w_cnt[tid >> 6] = cnt;
    w_mass[tid >> 6] = mass;
    w_score[tid >> 6] = best.score;
    w_idx[tid >> 6] = best.idx;
  }
  __syncthreads();
  if (tid != 0) return;
  for (int w = 1; w < NWAVE; ++w) {
    cnt += w_cnt[w];
    mass += w_mass[w];
    better(best, w_score[w], w_idx[w]);
  }
  // thr >= kKeyMin <= kmax and the max is always kept: cnt >= 1, idx < V
  const int idx = (best.idx >= 0 && best.idx < V) ? best.idx : 0;
  const float x_tok = key_value(load_key((u32)row[idx]));
  // the max's own mass is mscale exactly, so mass / mscale >= 1
  const float lz = logf((float)mass / mscale);
  token[b] = idx;
  logprob[b] = (x_tok - vmax) / T - lz;
  thr_out[b] = key_bits(thr);
  n_kept[b] = (int)cnt;
  if (done != nullptr) done[b] = (unsigned char)((long long)idx == eos_id);
}

}  // namespace

extern "C" void acco_sample_logits(const void* logits, long long row_stride,
                                   int B, int V, float temperature,
                                   int top_k, double top_p,
                                   unsigned long long seed,
                                   unsigned long long step,
                                   unsigned char* done, long long eos_id,
                                   long long* token, float* logprob,
                                   void* thr, int* n_kept, hipStream_t s) {
  const bool greedy = temperature == 0.0f;
  const float T = greedy ? 1.0f : temperature;
  // log2(e) / T rounded once: the exponent of a mass is one product away
  const float c2 = (float)(1.4426950408889634 / (double)T);
  // V masses of at most 2^shift each sum below 2^62
  int bits = 0;
  while ((1ll << bits) < (long long)V) ++bits;
  const int shift = 62 - bits < 40 ? 62 - bits : 40;
  const float mscale = ldexpf(1.0f, shift);
  hipLaunchKernelGGL(sample_kernel, dim3(B), dim3(BLOCK), 0, s,
                     (const u16*)logits, row_stride, V, T, c2, mscale, greedy,
                     top_k, top_p, seed, step, done, eos_id, token, logprob,
                     (u16*)thr, n_kept);
}
