// Sum of squares of a gradient segment for gfx950: the reduction behind
// global gradient-norm clipping on the ZeRO-1 sharded com round.
//
//   acco_grad_sumsq      one pass over a bf16 / fp32 segment, one fp32
//                        partial per block (partials[blockIdx.x]);
//   acco_sumsq_finalize  one block sums the partials of every bucket in
//                        double, in a fixed order, into one fp32.
//
// The scalar all-reduce across ranks and the clip coefficient sit between
// the finalize and the fused AdamW, which multiplies the gradient by a
// device-resident scale already (adamw.hip scale_dev), so the AdamW kernel
// is untouched.
//
// No atomics and no zeroed workspace: every block of the launch stores its
// slot (zero included) with an ordinary store, and every sum runs in a
// fixed order, so the result is bitwise reproducible for the same input.
//
// Memory-bound: 2 B/element (bf16). The segment is read once here and once
// more by the AdamW that follows; nontemporal loads keep it out of the L2
// the compute stream is using (adamw.hip has the same note).

#include "common.h"
#include "kernels.h"

namespace {

constexpr int kBlock = 256;

typedef float f4_ __attribute__((ext_vector_type(4)));
typedef unsigned int w4_ __attribute__((ext_vector_type(4)));

// elements per 16-byte chunk
template <typename T>
constexpr int vec_of() { return 16 / (int)sizeof(T); }

// acc[k] += x_k^2 over one 16-byte chunk; one accumulator per vector slot.
// The fma is spelled out: x·x + acc rounds once, in every instantiation.
template <typename T>
ACCO_DEV void square_accumulate(const T* __restrict__ g, long long chunk,
                                float* acc);

template <>
ACCO_DEV void square_accumulate<unsigned short>(
    const unsigned short* __restrict__ g, long long chunk, float* acc) {
  const w4_ w = __builtin_nontemporal_load(
      reinterpret_cast<const w4_*>(g) + chunk);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    // two bf16 per dword, the low half first in memory
    const float lo = __uint_as_float(w[k] << 16);
    const float hi = __uint_as_float(w[k] & 0xffff0000u);
    acc[2 * k] = __builtin_fmaf(lo, lo, acc[2 * k]);
    acc[2 * k + 1] = __builtin_fmaf(hi, hi, acc[2 * k + 1]);
  }
}

template <>
ACCO_DEV void square_accumulate<float>(const float* __restrict__ g,
                                       long long chunk, float* acc) {
  const f4_ x = __builtin_nontemporal_load(
      reinterpret_cast<const f4_*>(g) + chunk);
#pragma unroll
  for (int k = 0; k < 4; ++k) acc[k] = __builtin_fmaf(x[k], x[k], acc[k]);
}

ACCO_DEV float load_one(const unsigned short* g, long long i) {
  return bf16_to_f32(g[i]);
}
ACCO_DEV float load_one(const float* g, long long i) { return g[i]; }

template <typename T>
__global__ __launch_bounds__(kBlock)
void grad_sumsq_kernel(const T* __restrict__ g, float* __restrict__ partials,
                       long long n) {
  constexpr int VEC = vec_of<T>();
  const long long i0 = (long long)blockIdx.x * kBlock + threadIdx.x;
  const long long stride = (long long)gridDim.x * kBlock;
  const long long nv = n / VEC;

  // two grid-stride chunks per iteration, each with its own accumulators:
  // both 16-byte loads are in flight before any fma retires, and the 2·VEC
  // fma chains per lane are independent
  float a[VEC], b[VEC];
#pragma unroll
  for (int k = 0; k < VEC; ++k) { a[k] = 0.0f; b[k] = 0.0f; }

  long long i = i0;
  for (; i + stride < nv; i += 2 * stride) {
    square_accumulate<T>(g, i, a);
    square_accumulate<T>(g, i + stride, b);
  }
  for (; i < nv; i += stride) square_accumulate<T>(g, i, a);

  // scalar tail: n not a multiple of the vector width
  for (long long t = nv * VEC + i0; t < n; t += stride) {
    const float x = load_one(g, t);
    a[0] = __builtin_fmaf(x, x, a[0]);
  }

  // lane: pairwise over the accumulators, in a fixed order
#pragma unroll
  for (int k = 0; k < VEC; ++k) a[k] += b[k];
#pragma unroll
  for (int w = VEC / 2; w > 0; w >>= 1)
#pragma unroll
    for (int k = 0; k < w; ++k) a[k] += a[k + w];
  float s = a[0];

  // wave: shuffles; block: one slot per wave in LDS, summed by thread 0
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) s += __shfl_down(s, off, kWave);
  __shared__ float wave_sum[kBlock / kWave];
  if ((threadIdx.x & (kWave - 1)) == 0) wave_sum[threadIdx.x / kWave] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    float r = wave_sum[0];
#pragma unroll
    for (int w = 1; w < kBlock / kWave; ++w) r += wave_sum[w];
    partials[blockIdx.x] = r;
  }
}

// One block. Thread t sums partials[t], partials[t + 256], ... in double,
// then a fixed binary tree over the 256 lane sums in LDS.
__global__ __launch_bounds__(kBlock)
void sumsq_finalize_kernel(const float* __restrict__ partials,
                           long long count, float* __restrict__ out) {
  __shared__ double lane_sum[kBlock];
  double s = 0.0;
  for (long long i = threadIdx.x; i < count; i += kBlock)
    s += (double)partials[i];
  lane_sum[threadIdx.x] = s;
  __syncthreads();
  for (int w = kBlock / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w)
      lane_sum[threadIdx.x] += lane_sum[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = (float)lane_sum[0];
}

}  // namespace

extern "C" int acco_grad_sumsq_grid(long long n, bool is_bf16) {
  const int vec = is_bf16 ? 8 : 4;
  return elementwise_grid((n + vec - 1) / vec, kBlock);
}

extern "C" void acco_grad_sumsq(const void* g, float* partials, long long n,
                                bool is_bf16, hipStream_t stream) {
  const int grid = acco_grad_sumsq_grid(n, is_bf16);
  if (is_bf16)
    hipLaunchKernelGGL(grad_sumsq_kernel<unsigned short>, dim3(grid),
                       dim3(kBlock), 0, stream, (const unsigned short*)g,
                       partials, n);
  else
    hipLaunchKernelGGL(grad_sumsq_kernel<float>, dim3(grid), dim3(kBlock), 0,
                       stream, (const float*)g, partials, n);
}

extern "C" void acco_sumsq_finalize(const float* partials, long long count,
                                    float* out, hipStream_t stream) {
  hipLaunchKernelGGL(sumsq_finalize_kernel, dim3(1), dim3(kBlock), 0, stream,
                     partials, count, out);
}
