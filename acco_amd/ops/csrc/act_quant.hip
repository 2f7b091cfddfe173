// Activation quantiser of the W4A8 path on gfx950: bf16 rows to OCP MXFP8,
//   x [M, K] bf16 (rows x_rs apart) -> codes [M, K] e4m3, scales [M, K / 32]
// e8m0 bytes, bit for bit torch_ref.act_quantize_mxfp8. A streaming kernel:
// every byte of x read once, 1 + 1/32 bytes written per element, nothing
// reused, so no LDS.
//   - A thread owns 8 consecutive k: one 16-byte load, one 8-byte store. A
//     block of 32 is four adjacent lanes, aligned to 4 in the flat numbering
//     (K / 8 is a multiple of 4, so a group never straddles a row and is in
//     range or out of it as a whole), and amax crosses them by two xor
//     shuffles.
//   - The scale is integer arithmetic on amax's exponent field E:
//     floor(log2 amax) = E - 127 for a normal amax, so e = E - 135, clamped
//     into [-120, 120]; a subnormal amax (E = 0) lands on the clamp, as its
//     true logarithm does; a zero block takes e = 0. Finite bf16 has
//     E <= 254, so e <= 119 and 448 * 2^e is a finite fp32.
//   - x is clamped to +-448 * 2^e in fp32 (exact: a compare) and then
//     v_cvt_scalef32_pk_fp8_f32 divides by the scale's power of two and
//     rounds to nearest even, subnormals kept: two values per instruction,
//     four per thread. With the clamp in front the result does not depend on
//     what the convert does on overflow.
//   - The scale bytes: with K % 128 == 0 the four groups of 16 lanes own one
//     aligned dword of a row's scales, gathered by two more shuffles and
//     stored by the first lane; any other K % 32 == 0 stores a byte per
//     group. All stores are ordinary vector stores.
// Non-finite x is outside the contract, as in the reference.

#include "common.h"
#include "kernels.h"

namespace {

constexpr int kThreads = 256;

__global__ __launch_bounds__(kThreads)
void act_quant_kernel(const unsigned short* __restrict__ x,
                      unsigned char* __restrict__ codes,
                      unsigned char* __restrict__ scales, long long total,
                      int K, long long x_rs, bool pack) {
  const int per_row = K / 8;
  const long long stride = (long long)gridDim.x * kThreads;
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < total;
       i += stride) {
    const long long m = i / per_row;
    const int c = (int)(i % per_row);
    const uint4 raw = *reinterpret_cast<const uint4*>(x + m * x_rs + 8 * c);
    const unsigned* w = reinterpret_cast<const unsigned*>(&raw);
    float v[8];
    unsigned amax = 0;                  // as fp32 bits: order is the integers'
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const unsigned lo = w[q] << 16, hi = w[q] & 0xffff0000u;
      v[2 * q] = __uint_as_float(lo);
      v[2 * q + 1] = __uint_as_float(hi);
      amax = max(amax, max(lo & 0x7fffffffu, hi & 0x7fffffffu));
    }
    amax = max(amax, (unsigned)__shfl_xor((int)amax, 1));
    amax = max(amax, (unsigned)__shfl_xor((int)amax, 2));
    int e = min(max((int)(amax >> 23) - 135, -120), 120);
    if (amax == 0) e = 0;
    const float scale = __uint_as_float((unsigned)(e + 127) << 23);
    const float lim = __uint_as_float(((unsigned)(e + 135) << 23) | 0x600000u);
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = fminf(fmaxf(v[q], -lim), lim);
    using short2v = __attribute__((ext_vector_type(2))) short;
    union { short2v s; unsigned u; } lo, hi;
    lo.u = hi.u = 0;
    lo.s = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(lo.s, v[0], v[1], scale,
                                                    false);
    lo.s = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(lo.s, v[2], v[3], scale,
                                                    true);
    hi.s = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(hi.s, v[4], v[5], scale,
                                                    false);
    hi.s = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(hi.s, v[6], v[7], scale,
                                                    true);
    *reinterpret_cast<uint2*>(codes + m * K + 8 * c) = make_uint2(lo.u, hi.u);

    const long long sb = m * (K / 32) + c / 4;
    if (pack) {       // uniform; the 16 lanes of a dword are live together
      unsigned b = (unsigned)(e + 127) << (8 * (threadIdx.x / 4 % 4));
      b |= (unsigned)__shfl_xor((int)b, 4);
      b |= (unsigned)__shfl_xor((int)b, 8);
      if (threadIdx.x % 16 == 0) *reinterpret_cast<unsigned*>(scales + sb) = b;
    } else if (threadIdx.x % 4 == 0) {
      scales[sb] = (unsigned char)(e + 127);
    }
  }
}

}  // namespace

extern "C" void acco_act_quant_mxfp8(const void* x, void* codes, void* scales,
                                     long long M, int K, long long x_rs,
                                     hipStream_t stream) {
  const long long total = M * (K / 8);
  if (total < 1) return;            // the binding admits neither
  // whole passes of the grid keep the lane groups of a dword together
  hipLaunchKernelGGL(act_quant_kernel,
                     dim3(elementwise_grid(total, kThreads, 4096)),
                     dim3(kThreads), 0, stream, (const unsigned short*)x,
                     (unsigned char*)codes, (unsigned char*)scales, total, K,
                     x_rs, K % 128 == 0);
}
