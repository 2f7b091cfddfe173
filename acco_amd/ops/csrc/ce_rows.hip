// Row-wise cross-entropy for the chunked lm_head + loss path (gfx950).
//
// ce.hip works on whole [B, S, V] logits: it shifts the labels itself
// (t % S), writes dlogits to a second buffer and sums the loss with atomics.
// The chunked head computes the logits of a few thousand tokens at a time
// into one reused [C, V] buffer, so these kernels take rows with targets the
// caller has already shifted, emit per-row lse and loss (summed afterwards in
// a fixed order), and turn the buffer into dlogits in place.
//
// A row is valid iff 0 <= target < V; any other target (-100, >= V) marks an
// ignored row and is never used as an index.
//
// Alignment: the buffer base is 16-byte aligned (checked by the bindings) but
// row t starts at element t·V, which for odd V is only 2-byte aligned. Each
// row is split into a scalar head of (-(t·V)) mod 8 elements, naturally
// aligned 16-byte vectors, and a scalar tail of < 8 elements.
//
// No atomics and no zeroed workspace: every output slot gets an ordinary
// store on every call and every sum runs in a fixed order, so results are
// bitwise reproducible for the same input.

#include "common.h"
#include "kernels.h"

namespace {

using u16 = unsigned short;
constexpr int BLOCK = 256;
constexpr int kGridCap = 8192;   // as ce.hip

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

// one element into a thread's running (max, sum)
ACCO_DEV void online_scalar(float x, float& m, float& sum) {
  if (x > m) { sum *= __expf(m - x); m = x; }
  sum += __expf(x - m);
}

__global__ void ce_rows_fwd_kernel(const u16* __restrict__ logits,  // [T, V]
                                   const long long* __restrict__ targets,
                                   float* __restrict__ lse,          // [T]
                                   float* __restrict__ tok_loss,     // [T]
                                   long long T, int V, float epsilon) {
  __shared__ float lds_m[BLOCK / 64];
  __shared__ float lds_s[BLOCK / 64];
  __shared__ float lds_x[BLOCK / 64];
  const int tid = threadIdx.x;
  for (long long t = blockIdx.x; t < T; t += gridDim.x) {
    const long long target = targets[t];
    if (!valid_target(target, V)) {       // block-uniform
      if (tid == 0) { lse[t] = 0.0f; tok_loss[t] = 0.0f; }
      continue;
    }
    const u16* row = logits + t * (long long)V;
    const RowSplit rs = split_row(t, V);
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
      // chunk max first, one rescale of the running sum per 8 elements and
      // the 8 exps combined as a tree (ce_fwd_kernel has the reasoning)
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
    if (tid == 0) {
      float M = lds_m[0], Ssum = lds_s[0], Xsum = lds_x[0];
      for (int w2 = 1; w2 < BLOCK / 64; ++w2) {
        const float mo = lds_m[w2], so = lds_s[w2];
        const float mn = fmaxf(M, mo);
        Ssum = Ssum * __expf(M - mn) + so * __expf(mo - mn);
        M = mn;
        Xsum += lds_x[w2];
      }
      const float l = M + __logf(Ssum);
      float gold = bf16_to_f32(row[target]);
      if (epsilon != 0.0f)
        gold = (1.0f - epsilon) * gold + epsilon * (Xsum / (float)V);
      lse[t] = l;
      tok_loss[t] = l - gold;
    }
    __syncthreads();
  }
}

// row[v] = scale * (exp(x - lse[t]) - (1-eps)·1[v == target] - eps/V)
//          (valid rows; eps = 0 is plain CE)
//        = 0                                           (otherwise)
// in place: every element is read and written by the same thread
__global__ void ce_rows_bwd_kernel(u16* __restrict__ logits,   // [T, V]
                                   const long long* __restrict__ targets,
                                   const float* __restrict__ lse,
                                   const float* __restrict__ scale_dev,
                                   long long T, int V, float epsilon) {
  const float scale = *scale_dev;
  const float c_lab = 1.0f - epsilon;       // onehot weight
  const float c_uni = epsilon / (float)V;   // uniform smoothing weight
  const int tid = threadIdx.x;
  for (long long t = blockIdx.x; t < T; t += gridDim.x) {
    const long long target = targets[t];
    u16* row = logits + t * (long long)V;
    const RowSplit rs = split_row(t, V);
    w4_* body = reinterpret_cast<w4_*>(row + rs.peel);
    if (!valid_target(target, V)) {
      if (tid < rs.peel) row[tid] = 0;
      const w4_ z = {0u, 0u, 0u, 0u};
      for (int c = tid; c < rs.nvec; c += BLOCK) body[c] = z;
      if (rs.tail + tid < V) row[rs.tail + tid] = 0;
      continue;
    }
    const int label = (int)target;
    const float l = lse[t];
    if (tid < rs.peel) {
      float p = __expf(bf16_to_f32(row[tid]) - l) - c_uni;
      if (tid == label) p -= c_lab;
      row[tid] = f32_to_bf16(p * scale);
    }
    for (int c = tid; c < rs.nvec; c += BLOCK) {
      float f[8];
      unpack8(body[c], f);
      const int base = rs.peel + c * 8;
      u16 o[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        float p = __expf(f[k] - l) - c_uni;
        if (base + k == label) p -= c_lab;
        o[k] = f32_to_bf16(p * scale);
      }
      w4_ q;
#pragma unroll
      for (int k = 0; k < 4; ++k)
        q[k] = (unsigned int)o[2 * k] | ((unsigned int)o[2 * k + 1] << 16);
      body[c] = q;
    }
    if (rs.tail + tid < V) {
      const int v = rs.tail + tid;
      float p = __expf(bf16_to_f32(row[v]) - l) - c_uni;
      if (v == label) p -= c_lab;
      row[v] = f32_to_bf16(p * scale);
    }
  }
}

int rows_grid(long long T) { return (int)((T < kGridCap) ? T : kGridCap); }

}  // namespace

extern "C" {

void acco_ce_rows_fwd(const void* logits, const long long* targets,
                      float* lse, float* tok_loss, long long T, int V,
                      float epsilon, hipStream_t s) {
  hipLaunchKernelGGL(ce_rows_fwd_kernel, dim3(rows_grid(T)), dim3(BLOCK), 0,
                     s, (const u16*)logits, targets, lse, tok_loss, T, V,
                     epsilon);
}

void acco_ce_rows_bwd(void* logits_inout, const long long* targets,
                      const float* lse, const float* scale_dev, long long T,
                      int V, float epsilon, hipStream_t s) {
  hipLaunchKernelGGL(ce_rows_bwd_kernel, dim3(rows_grid(T)), dim3(BLOCK), 0,
                     s, (u16*)logits_inout, targets, lse, scale_dev, T, V,
                     epsilon);
}

}  // extern "C"
