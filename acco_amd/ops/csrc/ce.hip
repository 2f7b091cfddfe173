// Fused causal-LM cross-entropy for gfx950 (SURVEY.md §2.5 K1 loss + K9).
// The eager path materializes fp32 log-softmax over [B,S,V] (vocab 50k:
// ~1.6 GB of HBM traffic per cast); these kernels do one online logsumexp
// pass over bf16 logits (fwd) and one fused softmax-minus-onehot pass (bwd),
// both at HBM-roofline. One 256-thread block per row of V logits.
//
// One row skeleton, two policies:
//   Shifted  whole [B, S, V] logits. The kernel shifts the labels itself
//            (row t takes labels[t + 1], a sequence's last position none),
//            writes dlogits to a second buffer scaled by dloss / n_valid, and
//            atomicAdds {loss_sum, n_valid} into a sharded fp32 accumulator.
//   Rows     [T, V] rows of the chunked lm_head + loss with targets the
//            caller has already shifted. Per-row lse and loss get ordinary
//            stores (summed afterwards in a fixed order) and the rows turn
//            into dlogits in place, scaled by a device scalar. No atomics and
//            no zeroed workspace: bitwise reproducible for the same input.
//
// A row is valid iff 0 <= target < V, under both policies; any other target
// (-100, >= V) marks an ignored row (lse 0, no loss, not counted, zero
// dlogits) and is never used as an index.
//
// epsilon != 0 adds HF-LabelSmoother semantics (SURVEY.md §2.5 K9;
// reference utils/trainer_utils.py:862-902): per valid row,
// loss = (1-eps)·(lse - x[label]) + eps·(lse - Σ_v x_v / V).
//
// Alignment: the logits base is 16-byte aligned (checked by the bindings) but
// row t starts at element t·V, which for odd V is only 2-byte aligned. Each
// row is split into a scalar head of (-(t·V)) mod 8 elements, naturally
// aligned 16-byte vectors, and a scalar tail of < 8 elements; a second
// buffer of the same layout and alignment shares the split.

#include "common.h"
#include "kernels.h"

namespace {

using u16 = unsigned short;
constexpr int BLOCK = 256;
constexpr int kGridCap = 8192;
// SHARDED accumulator: 16k per-row atomicAdds on one L2 cell serialize at
// ~88/us and were the kernel's real bound (PMC: 87% WAIT_ANY, loads already
// dwordx4); 128 shards cut the contention 128x and the wrapper reduces
// [128,2] with one tiny sum
constexpr int kAccShards = 128;

typedef unsigned int w4_ __attribute__((ext_vector_type(4)));

struct RowSplit {
  int peel;   // scalar head elements [0, peel)
  int nvec;   // 16-byte vectors covering [peel, tail)
  int tail;   // first scalar tail element
};

ACCO_DEV RowSplit split_row(long long t, int V) {
  RowSplit r;
  r.peel = (int)((8 - ((t * (long long)V) & 7)) & 7);
  if (r.peel > V) r.peel = V;
  r.nvec = (V - r.peel) / 8;
  r.tail = r.peel + r.nvec * 8;
  return r;
}

ACCO_DEV bool valid_target(long long target, int V) {
  return (unsigned long long)target < (unsigned long long)V;
}

ACCO_DEV float bits_to_f32(unsigned int i) {
  union { unsigned int i; float f; } c;
  c.i = i;
  return c.f;
}

// the 8 bf16 of one 16-byte vector, in memory order
ACCO_DEV void unpack8(w4_ q, float* f) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    f[2 * k] = bits_to_f32(q[k] << 16);
    f[2 * k + 1] = bits_to_f32(q[k] & 0xffff0000u);
  }
}

ACCO_DEV w4_ pack8(const u16* o) {
  w4_ q;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    q[k] = (unsigned int)o[2 * k] | ((unsigned int)o[2 * k + 1] << 16);
  return q;
}

// one element into a thread's running (max, sum)
ACCO_DEV void online_scalar(float x, float& m, float& sum) {
  if (x > m) { sum *= __expf(m - x); m = x; }
  sum += __expf(x - m);
}

// ---- policies: what a launch carries beyond the rows themselves
struct Shifted {
  int S;
  // backward only
  float dloss;                 // upstream grad, unless the launch has a
  const float* acc;            //   device scalar; n_valid at acc[1]
  u16* dlogits;
  // out of place: nothing reaches the logits but this pointer, which is
  // what lets their loads move across the dlogits stores
  using Src = const u16* __restrict__;
  ACCO_DEV u16* dst(Src) const { return dlogits; }
  ACCO_DEV long long target(const long long* labels, long long t) const {
    return ((int)(t % S) < S - 1) ? labels[t + 1] : -100;
  }
  ACCO_DEV void sink(float* accs, long long, float loss, bool valid) const {
    if (!valid) return;
    float* a = accs + 2 * (blockIdx.x & (kAccShards - 1));
    atomicAdd(a, loss);
    atomicAdd(a + 1, 1.0f);
  }
  ACCO_DEV float scale(const float* dloss_dev) const {
    // the device scalar avoids a D2H sync in backward
    const float dl = (dloss_dev != nullptr) ? *dloss_dev : dloss;
    return dl / fmaxf(acc[1], 1.0f);
  }
};

struct Rows {
  // in place: one pointer, every element read and written by the same thread
  using Src = u16* __restrict__;
  ACCO_DEV u16* dst(Src logits) const { return logits; }
  ACCO_DEV long long target(const long long* targets, long long t) const {
    return targets[t];
  }
  ACCO_DEV void sink(float* tok_loss, long long t, float loss, bool) const {
    tok_loss[t] = loss;
  }
  ACCO_DEV float scale(const float* scale_dev) const { return *scale_dev; }
};

// ---- forward
// Online logsumexp of one row over the whole block: head, vectors, tail per
// thread, wave shuffle reduce, LDS combine. Thread 0 alone gets l and the
// row's Σ x (epsilon != 0 only); the caller syncs before the next row.
ACCO_DEV void row_logsumexp(const u16* row, const RowSplit rs, int V,
                            float epsilon, float& l, float& Xsum) {
  __shared__ float lds_m[BLOCK / 64];
  __shared__ float lds_s[BLOCK / 64];
  __shared__ float lds_x[BLOCK / 64];
  const int tid = threadIdx.x;
  float m = -3.4e38f, sum = 0.0f, xsum = 0.0f;
  if (tid < rs.peel) {
    const float x = bf16_to_f32(row[tid]);
    online_scalar(x, m, sum);
    if (epsilon != 0.0f) xsum += x;
  }
  const w4_* body = reinterpret_cast<const w4_*>(row + rs.peel);
  for (int c = tid; c < rs.nvec; c += BLOCK) {
    float f[8];
    unpack8(body[c], f);
    if (epsilon != 0.0f)
      xsum += ((f[0] + f[1]) + (f[2] + f[3])) +
              ((f[4] + f[5]) + (f[6] + f[7]));
    // chunk max first, one rescale of the running sum per 8 elements —
    // replaces the per-element branchy online update (8 dependent
    // branch+rescale chains) with independent exps. The 8 exps combine as
    // a TREE: without fast-math the naive `sum += e[k]` loop is a strictly
    // ordered 9-deep dependent fp chain per chunk; the tree cuts the
    // cross-chunk dependency to rescale-mul + one add.
    const float cm = fmaxf(fmaxf(fmaxf(f[0], f[1]), fmaxf(f[2], f[3])),
                           fmaxf(fmaxf(f[4], f[5]), fmaxf(f[6], f[7])));
    const float mn = fmaxf(m, cm);
    float e[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) e[k] = __expf(f[k] - mn);
    const float es = ((e[0] + e[1]) + (e[2] + e[3])) +
                     ((e[4] + e[5]) + (e[6] + e[7]));
    sum = sum * __expf(m - mn) + es;
    m = mn;
  }
  if (rs.tail + tid < V) {              // < 8 tail elements
    const float x = bf16_to_f32(row[rs.tail + tid]);
    online_scalar(x, m, sum);
    if (epsilon != 0.0f) xsum += x;
  }
  // wave-reduce the (m, sum) pairs (+ xsum for the smoothing term)
  for (int off = 32; off > 0; off >>= 1) {
    const float mo = __shfl_down(m, off, 64);
    const float so = __shfl_down(sum, off, 64);
    const float mn = fmaxf(m, mo);
    sum = sum * __expf(m - mn) + so * __expf(mo - mn);
    m = mn;
    if (epsilon != 0.0f) xsum += __shfl_down(xsum, off, 64);
  }
  const int wave = tid / 64;
  if ((tid & 63) == 0) {
    lds_m[wave] = m; lds_s[wave] = sum; lds_x[wave] = xsum;
  }
  __syncthreads();
  if (tid != 0) return;
  float M = lds_m[0], Ssum = lds_s[0];
  Xsum = lds_x[0];
  for (int w2 = 1; w2 < BLOCK / 64; ++w2) {
    const float mo = lds_m[w2], so = lds_s[w2];
    const float mn = fmaxf(M, mo);
    Ssum = Ssum * __expf(M - mn) + so * __expf(mo - mn);
    M = mn;
    Xsum += lds_x[w2];
  }
  l = M + __logf(Ssum);
}

// lse[t] of every row (0 on ignored rows); the row's loss goes to the
// policy's sink: `out` is the [128, 2] accumulator (Shifted) or tok_loss
// (Rows)
template <class P>
__global__ void ce_fwd_kernel(const u16* __restrict__ logits,        // [T, V]
                              const long long* __restrict__ targets,
                              float* __restrict__ lse,               // [T]
                              float* __restrict__ out,
                              long long T, int V, float epsilon, const P p) {
  for (long long t = blockIdx.x; t < T; t += gridDim.x) {
    const long long target = p.target(targets, t);
    if (!valid_target(target, V)) {       // block-uniform
      if (threadIdx.x == 0) { lse[t] = 0.0f; p.sink(out, t, 0.0f, false); }
      continue;
    }
    const u16* row = logits + t * (long long)V;
    float l = 0.0f, Xsum = 0.0f;
    row_logsumexp(row, split_row(t, V), V, epsilon, l, Xsum);
    if (threadIdx.x == 0) {
      float gold = bf16_to_f32(row[target]);
      if (epsilon != 0.0f)
        gold = (1.0f - epsilon) * gold + epsilon * (Xsum / (float)V);
      lse[t] = l;
      p.sink(out, t, l - gold, true);
    }
    __syncthreads();
  }
}

// ---- backward
// scale * (exp(x - lse[t]) - (1-eps)·1[v == target] - eps/V); eps = 0 is
// plain CE
ACCO_DEV u16 dlogit(float x, float l, float c_uni, float c_lab, bool at_label,
                    float scale) {
  float p = __expf(x - l) - c_uni;
  if (at_label) p -= c_lab;
  return f32_to_bf16(p * scale);
}

ACCO_DEV void zero_row(u16* drow, const RowSplit rs, int V) {
  const int tid = threadIdx.x;
  w4_* dbody = reinterpret_cast<w4_*>(drow + rs.peel);
  if (tid < rs.peel) drow[tid] = 0;
  const w4_ z = {0u, 0u, 0u, 0u};
  for (int c = tid; c < rs.nvec; c += BLOCK) dbody[c] = z;
  if (rs.tail + tid < V) drow[rs.tail + tid] = 0;
}

// dlogits rows of valid targets as above, zero rows otherwise; scale and
// destination are the policy's: `scale_dev` is the scale itself (Rows) or
// the upstream grad, null for the host's `dloss` (Shifted)
template <class P>
__global__ void ce_bwd_kernel(typename P::Src logits,               // [T, V]
                              const long long* __restrict__ targets,
                              const float* __restrict__ lse,
                              const float* __restrict__ scale_dev,
                              long long T, int V, float epsilon, const P p) {
  const float scale = p.scale(scale_dev);
  const float c_lab = 1.0f - epsilon;       // onehot weight
  const float c_uni = epsilon / (float)V;   // uniform smoothing weight
  const int tid = threadIdx.x;
  for (long long t = blockIdx.x; t < T; t += gridDim.x) {
    const long long target = p.target(targets, t);
    const auto* row = logits + t * (long long)V;
    u16* drow = p.dst(logits) + t * (long long)V;
    const RowSplit rs = split_row(t, V);
    if (!valid_target(target, V)) {
      zero_row(drow, rs, V);
      continue;
    }
    const int label = (int)target;
    const float l = lse[t];
    if (tid < rs.peel)
      drow[tid] = dlogit(bf16_to_f32(row[tid]), l, c_uni, c_lab, tid == label,
                         scale);
    const w4_* body = reinterpret_cast<const w4_*>(row + rs.peel);
    w4_* dbody = reinterpret_cast<w4_*>(drow + rs.peel);
    for (int c = tid; c < rs.nvec; c += BLOCK) {
      float f[8];
      unpack8(body[c], f);
      const int base = rs.peel + c * 8;
      u16 o[8];
#pragma unroll
      for (int k = 0; k < 8; ++k)
        o[k] = dlogit(f[k], l, c_uni, c_lab, base + k == label, scale);
      dbody[c] = pack8(o);
    }
    if (rs.tail + tid < V) {
      const int v = rs.tail + tid;
      drow[v] = dlogit(bf16_to_f32(row[v]), l, c_uni, c_lab, v == label,
                       scale);
    }
  }
}

dim3 ce_grid(long long T) { return dim3((int)((T < kGridCap) ? T : kGridCap)); }

}  // namespace

extern "C" {

void acco_ce_fwd(const void* logits, const long long* labels, float* lse,
                 float* acc, long long T, int S, int V, float epsilon,
                 hipStream_t s) {
  hipLaunchKernelGGL(ce_fwd_kernel<Shifted>, ce_grid(T), dim3(BLOCK), 0, s,
                     (const u16*)logits, labels, lse, acc, T, V, epsilon,
                     Shifted{S});
}

void acco_ce_bwd(const void* logits, const long long* labels,
                 const float* lse, void* dlogits, const float* acc,
                 float dloss, const float* dloss_dev, long long T, int S,
                 int V, float epsilon, hipStream_t s) {
  hipLaunchKernelGGL(ce_bwd_kernel<Shifted>, ce_grid(T), dim3(BLOCK), 0, s,
                     (const u16*)logits, labels, lse, dloss_dev, T, V,
                     epsilon, Shifted{S, dloss, acc, (u16*)dlogits});
}

void acco_ce_rows_fwd(const void* logits, const long long* targets,
                      float* lse, float* tok_loss, long long T, int V,
                      float epsilon, hipStream_t s) {
  hipLaunchKernelGGL(ce_fwd_kernel<Rows>, ce_grid(T), dim3(BLOCK), 0, s,
                     (const u16*)logits, targets, lse, tok_loss, T, V,
                     epsilon, Rows{});
}

void acco_ce_rows_bwd(void* logits_inout, const long long* targets,
                      const float* lse, const float* scale_dev, long long T,
                      int V, float epsilon, hipStream_t s) {
  hipLaunchKernelGGL(ce_bwd_kernel<Rows>, ce_grid(T), dim3(BLOCK), 0, s,
                     (u16*)logits_inout, targets, lse, scale_dev, T, V,
                     epsilon, Rows{});
}

}  // extern "C"
