// Draft verification for speculative decoding on gfx950: the accept / reject /
// resample step over target logits p [B, k+1, V] and draft logits q [B, k, V]
// (bf16), with no softmax tensor, no host read and no dependency between
// workgroups. torch_ref.spec_verify is the executable definition.
//
// Two kernels.
//   spec_rows_kernel    one 1024-thread workgroup per row (b, t), B (k + 1) of
//     them. The row of the first rejection is known only after every accept
//     test, so each row computes what it would contribute if the rejection
//     fell there: its accept decision and probability (t < k), and its
//     candidate token: the Gumbel-max draw from the residual max(p_t - q_t, 0)
//     for t < k, from p_k for t = k. Both go by ordinary stores into a
//     workspace int32 [B, k+1, 2] that needs no clearing.
//   spec_select_kernel  one thread per sequence walks its k + 1 workspace rows
//     in order: n_accept = accepted rows before the first rejection,
//     next_token = that row's candidate. It also owns the done flags.
// No atomics, global or LDS; nothing crosses workgroups inside a kernel.
//
// Passes of a row at temperature > 0 (a pair of rows is 512 KB at V = 128k and
// is re-read from L2 by each pass):
//   1  the largest key of p_t and of q_t
//   2  both partition sums, as 64-bit fixed point (trunc(exp2(.) · 2^shift),
//      sample.hip's masses): integer sums are exact in any order, so the
//      outputs are bitwise reproducible whatever the rows' alignment
//   3  t < k: argmax over p_i > q_i of log(p_i - q_i) + g_i, lowest index on
//      ties; only elements with a positive residual draw from Philox
//   4  the Gumbel-max draw from p_t, score x_i / T + g_i as the sampler writes
//      it: always for t = k (in place of pass 3), and for t < k only when the
//      residual is empty
// p_i = exp2((x_i - max) · c2) / Z with 1 / Z rounded once per row; the accept
// test is u · q(x) < p(x), without a division. temperature == 0 is one pass:
// the lowest-index argmax of p_t, accepted iff the drafted token equals it; q
// is not read.
//
// Generator. Philox4x32-10 under key (seed_lo, seed_hi); the sampler owns the
// counters (i, row, step_lo, step_hi) with i < 2^31 and row < 2^31. Here
// word 1 is 2^31 | (b (k + 1) + t), which no sampler row has: g_i of row
// (b, t) sits at word 0 = i < V, the accept test's u_t at word 0 = 2^32 - 1.
//
// Alignment: each row is split by its own address into a scalar head, aligned
// 16-byte vectors and a scalar tail (for_each_elem). p_t and q_t
// have different alignments when V is odd, so pass 3 walks p_t that way and
// reads q_t[i] by a 2-byte load per element.
//
// First guesses that nobody has measured against an alternative: 1024 threads
// per workgroup; one workgroup per row, which leaves most CUs idle at small
// B (k + 1); four passes instead of a fused max / sum pass; the 2-byte loads
// of q in pass 3 (instead of a second vector path for equal alignments).
// RESULTS.md ("Speculative decoding") has what the kernel costs.

// The attribute opens before the includes so that the HIP headers' helpers
// still inline; the host pass does not know the feature, hence the guard.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(                                      \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

#include "kernels.h"
#include "sampling_common.h"

namespace {

using namespace sampling;

constexpr u32 kRowTag = 0x80000000u;      // word 1: no sampler row has bit 31
constexpr u32 kAcceptWord = 0xffffffffu;  // word 0 of u_t: no index reaches it
constexpr int kNoIdx = 0x7fffffff;

// Block reductions. Every thread returns with the result; each ends on a
// barrier, so its LDS may be rewritten at once.
ACCO_DEV void block_max2(u32& a, u32& b, u32 (*sh)[NWAVE]) {
  for (int off = 32; off > 0; off >>= 1) {
    const u32 oa = __shfl_xor(a, off, 64), ob = __shfl_xor(b, off, 64);
    a = oa > a ? oa : a;
    b = ob > b ? ob : b;
  }
  const int tid = threadIdx.x;
  if ((tid & 63) == 0) { sh[0][tid >> 6] = a; sh[1][tid >> 6] = b; }
  __syncthreads();
  for (int w = 0; w < NWAVE; ++w) {
    a = sh[0][w] > a ? sh[0][w] : a;
    b = sh[1][w] > b ? sh[1][w] : b;
  }
  __syncthreads();
}

ACCO_DEV void block_sum2(u64& a, u64& b, u64 (*sh)[NWAVE]) {
  for (int off = 32; off > 0; off >>= 1) {
    a += __shfl_xor(a, off, 64);
    b += __shfl_xor(b, off, 64);
  }
  const int tid = threadIdx.x;
  if ((tid & 63) == 0) { sh[0][tid >> 6] = a; sh[1][tid >> 6] = b; }
  __syncthreads();
  a = 0ull;
  b = 0ull;
  for (int w = 0; w < NWAVE; ++w) { a += sh[0][w]; b += sh[1][w]; }
  __syncthreads();
}

ACCO_DEV void block_best(Best& best, float* sh_score, int* sh_idx) {
  for (int off = 32; off > 0; off >>= 1) {
    const float so = __shfl_xor(best.score, off, 64);
    const int io = __shfl_xor(best.idx, off, 64);
    better(best, so, io);
  }
  const int tid = threadIdx.x;
  if ((tid & 63) == 0) {
    sh_score[tid >> 6] = best.score;
    sh_idx[tid >> 6] = best.idx;
  }
  __syncthreads();
  for (int w = 0; w < NWAVE; ++w) better(best, sh_score[w], sh_idx[w]);
  __syncthreads();
}

__global__ __launch_bounds__(BLOCK) void spec_rows_kernel(
    const u16* __restrict__ p, long long p_bs, long long p_ts,
    const u16* __restrict__ q, long long q_bs, long long q_ts,
    const long long* __restrict__ draft, int k, int V, float T, float c2,
    float mscale, bool greedy, u64 seed, u64 step,
    const unsigned char* __restrict__ done, float* __restrict__ accept_prob,
    int* __restrict__ ws) {
  __shared__ u32 sh_key[2][NWAVE];
  __shared__ u64 sh_sum[2][NWAVE];
  __shared__ float sh_score[NWAVE];
  __shared__ int sh_idx[NWAVE];

  const int row = blockIdx.x;
  const int b = row / (k + 1), t = row - b * (k + 1);
  const int tid = threadIdx.x;
  const bool has_q = t < k;
  if (done != nullptr && done[b] != 0) {       // block-uniform
    if (tid == 0 && has_q) accept_prob[(long long)b * k + t] = 0.0f;
    return;                                    // the select never reads ws
  }
  const u16* prow = p + (long long)b * p_bs + (long long)t * p_ts;
  const u16* qrow = has_q ? q + (long long)b * q_bs + (long long)t * q_ts
                          : prow;              // never read when !has_q
  const long long x = has_q ? draft[(long long)b * k + t] : -1;
  const bool x_ok = x >= 0 && x < (long long)V;
  int* out = ws + 2 * (long long)row;

  Best best = {-INFINITY, kNoIdx};
  if (greedy) {
    // keys are integers below 2^16: exact as floats
    for_each_elem(prow, V, [&](u32 bits, int i) {
      better(best, (float)load_key(bits), i);
    });
    block_best(best, sh_score, sh_idx);
    if (tid == 0) {
      const bool acc = x_ok && x == (long long)best.idx;
      out[0] = acc;
      out[1] = best.idx;
      if (has_q) accept_prob[(long long)b * k + t] = acc ? 1.0f : 0.0f;
    }
    return;
  }

  // ---- pass 1: both maxima
  u32 kp = 0u, kq = 0u;
  for_each_elem(prow, V, [&](u32 bits, int) {
    const u32 key = load_key(bits);
    kp = key > kp ? key : kp;
  });
  if (has_q)
    for_each_elem(qrow, V, [&](u32 bits, int) {
      const u32 key = load_key(bits);
      kq = key > kq ? key : kq;
    });
  block_max2(kp, kq, sh_key);
  if (kp == 0u) {                              // p_t has no finite logit: p = 0
    if (tid == 0) {
      out[0] = 0;
      out[1] = 0;
      if (has_q) accept_prob[(long long)b * k + t] = 0.0f;
    }
    return;
  }
  const float vp = key_value(kp);
  const float vq = kq != 0u ? key_value(kq) : 0.0f;

  // ---- pass 2: both partition sums, fixed point
  u64 zp = 0ull, zq = 0ull;
  for_each_elem(prow, V, [&](u32 bits, int) {
    const u32 key = load_key(bits);
    if (key != 0u) zp += fixed_mass(key, vp, c2, mscale);
  });
  if (kq != 0u)
    for_each_elem(qrow, V, [&](u32 bits, int) {
      const u32 key = load_key(bits);
      if (key != 0u) zq += fixed_mass(key, vq, c2, mscale);
    });
  block_sum2(zp, zq, sh_sum);
  // the maximum's own mass is mscale exactly: both sums are >= mscale
  const float rzp = 1.0f / ((float)zp / mscale);
  const float rzq = kq != 0u ? 1.0f / ((float)zq / mscale) : 0.0f;
  auto prob_p = [&](u32 key) {
    return key != 0u ? mass(key, vp, c2) * rzp : 0.0f;
  };
  auto prob_q = [&](u32 key) {
    return (key != 0u && kq != 0u) ? mass(key, vq, c2) * rzq : 0.0f;
  };

  const u32 k0 = (u32)seed, k1 = (u32)(seed >> 32);
  const u32 s0 = (u32)step, s1 = (u32)(step >> 32);
  const u32 c1 = kRowTag | (u32)row;

  // ---- the accept test of the drafted token
  if (tid == 0 && has_q) {
    float px = 0.0f, qx = 0.0f;
    if (x_ok) {
      px = prob_p(load_key((u32)prow[x]));
      qx = prob_q(load_key((u32)qrow[x]));
    }
    const float u = uniform01(philox_word0(kAcceptWord, c1, s0, s1, k0, k1));
    out[0] = u * qx < px;
    accept_prob[(long long)b * k + t] =
        px >= qx ? (px > 0.0f ? 1.0f : 0.0f) : px / qx;
  }

  // ---- pass 3: the draw from the residual
  if (has_q) {
    for_each_elem(prow, V, [&](u32 bits, int i) {
      const u32 key = load_key(bits);
      if (key == 0u) return;
      const float r = prob_p(key) - prob_q(load_key((u32)qrow[i]));
      if (r > 0.0f)
        better(best, logf(r) + gumbel(philox_word0((u32)i, c1, s0, s1, k0, k1)),
               i);
    });
    block_best(best, sh_score, sh_idx);
  }
  // ---- pass 4: the draw from p_t (t = k, or an empty residual)
  if (best.idx == kNoIdx) {                    // block-uniform
    for_each_elem(prow, V, [&](u32 bits, int i) {
      const u32 key = load_key(bits);
      if (key == 0u) return;
      better(best, key_value(key) / T +
                       gumbel(philox_word0((u32)i, c1, s0, s1, k0, k1)), i);
    });
    block_best(best, sh_score, sh_idx);
  }
  if (tid == 0) {
    if (!has_q) out[0] = 0;
    // kp != 0: at least one element was a candidate, so idx < V
    out[1] = (best.idx >= 0 && best.idx < V) ? best.idx : 0;
  }
}

__global__ void spec_select_kernel(const int* __restrict__ ws, int B, int k,
                                   unsigned char* __restrict__ done,
                                   long long eos_id,
                                   int* __restrict__ n_accept,
                                   long long* __restrict__ next_token) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  if (done != nullptr && done[b] != 0) {
    n_accept[b] = 0;
    next_token[b] = eos_id;
    return;
  }
  const int* rows = ws + 2 * (long long)b * (k + 1);
  int t = 0;
  while (t < k && rows[2 * t] != 0) ++t;
  const long long tok = rows[2 * t + 1];
  n_accept[b] = t;
  next_token[b] = tok;
  if (done != nullptr) done[b] = (unsigned char)(tok == eos_id);
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

}  // namespace

extern "C" void acco_spec_verify(const void* p_logits, long long p_bs,
                                 long long p_ts, const void* q_logits,
                                 long long q_bs, long long q_ts,
                                 const long long* draft_tokens, int B, int k,
                                 int V, float temperature,
                                 unsigned long long seed,
                                 unsigned long long step, unsigned char* done,
                                 long long eos_id, int* n_accept,
                                 long long* next_token, float* accept_prob,
                                 int* workspace, hipStream_t s) {
  const SamplingParams sp = sampling_params(temperature, V);
  hipLaunchKernelGGL(spec_rows_kernel, dim3(B * (k + 1)), dim3(BLOCK), 0, s,
                     (const u16*)p_logits, p_bs, p_ts, (const u16*)q_logits,
                     q_bs, q_ts, draft_tokens, k, V, sp.T, sp.c2, sp.mscale,
                     sp.greedy, seed, step, (const unsigned char*)done,
                     accept_prob, workspace);
  hipLaunchKernelGGL(spec_select_kernel, dim3((B + 255) / 256), dim3(256), 0,
                     s, (const int*)workspace, B, k, done, eos_id, n_accept,
                     next_token);
}
