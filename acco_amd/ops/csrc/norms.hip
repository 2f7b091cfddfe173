// RMSNorm (Llama) and LayerNorm (GPT-Neo) forward + backward for gfx950.
// One 256-thread block per G rows (G = 4/2/1 picked from D so every wave
// has work even at small D — D=768 fills 96 of 256 lanes in the one-row
// layout, measured 1.4 TB/s; the grouped layout packs 2 rows per block),
// grid-striding rows; bf16 loads vectorized ×8 (guide G13); row statistics
// by wave shuffle + LDS cross-wave reduce; weight/bias staged in LDS once
// per block.
//
// Three kernel templates serve both families: the grouped forward, the
// block-per-row backward (D/8 > 128) and the wave-per-row backward
// (D/8 <= 128). The family (Rms / Ln tag) is a compile-time parameter and
// only picks the per-row arithmetic.
//
// The per-thread value arrays are templated on the compile-time chunk
// count (guide §5.4 rule 20: runtime-indexed ext-vector arrays go to
// scratch — a first version with a runtime chunk loop ran 8-14× off
// roofline; see profiles/r01_bench_llama1b_acco_1gpu_kernels.txt).
// dW/dB land as one [partial_rows, D] fp32 scratch row per block,
// reduced to [D] in the weight's dtype by norm_dw_finalize_kernel (one
// launch; atomicAdd from the bwd kernels serialized ~3× worse).
// Replaces the HF RMSNorm / nn.LayerNorm ATen chains.

#include <type_traits>

#include "common.h"
#include "kernels.h"

namespace {

using u16 = unsigned short;

constexpr int BLOCK = 256;
constexpr int VEC = 8;                  // bf16 per thread per chunk

// The norm family as a tag type, so a kernel trace reads
// norm_fwd_kernel<Rms, 1, 4>. kLayer: a bias, a row mean and dB on top of
// what RMSNorm has. kPrefetch: the wave-per-row bwd loads the next row under
// the current row's reductions; it costs the Rms instantiations an occupancy
// step each (76 -> 94 and 112 -> 140 VGPRs, RESULTS.md) and no shipped
// config runs RMSNorm at D <= 1024, so only LayerNorm, where it was
// measured, has it.
struct Rms { static constexpr bool kLayer = false, kPrefetch = false; };
struct Ln { static constexpr bool kLayer = true, kPrefetch = true; };

// Reduce a float over one row-group (TPG = BLOCK/G threads). All groups
// hit the same __syncthreads unconditionally — barriers stay block-uniform
// even when a group's row index runs past R.
template <int G>
ACCO_DEV float group_reduce_sum(float x, float* lds, int g, int lane) {
  constexpr int WPG = (BLOCK / G) / 64;   // waves per group
  for (int off = 32; off > 0; off >>= 1)
    x += __shfl_down(x, off, 64);
  if ((lane & 63) == 0) lds[g * WPG + lane / 64] = x;
  __syncthreads();
  float r = 0.0f;
#pragma unroll
  for (int wv = 0; wv < WPG; ++wv) r += lds[g * WPG + wv];
  __syncthreads();
  return r;
}

ACCO_DEV float wave_reduce_sum(float x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
  return x;
}

ACCO_DEV void load8(const u16* p, float* f) {
  ushort4 a = reinterpret_cast<const ushort4*>(p)[0];
  ushort4 b = reinterpret_cast<const ushort4*>(p)[1];
  f[0] = bf16_to_f32(a.x); f[1] = bf16_to_f32(a.y);
  f[2] = bf16_to_f32(a.z); f[3] = bf16_to_f32(a.w);
  f[4] = bf16_to_f32(b.x); f[5] = bf16_to_f32(b.y);
  f[6] = bf16_to_f32(b.z); f[7] = bf16_to_f32(b.w);
}

ACCO_DEV void store8(u16* p, const float* f) {
  reinterpret_cast<ushort4*>(p)[0] =
      make_ushort4(f32_to_bf16(f[0]), f32_to_bf16(f[1]),
                   f32_to_bf16(f[2]), f32_to_bf16(f[3]));
  reinterpret_cast<ushort4*>(p)[1] =
      make_ushort4(f32_to_bf16(f[4]), f32_to_bf16(f[5]),
                   f32_to_bf16(f[6]), f32_to_bf16(f[7]));
}

// ------------------------------------------- pieces every kernel shares
// A thread of a row group owns CH chunks of VEC columns; chunk j is vector
// cid[j] = lane + j·tpg of the row, live (act[j]) while that is inside D.
// CH is a template parameter everywhere so the arrays stay in registers.

// the bf16 [D] weight (BIAS: and the bias behind it) → LDS, 16 bytes per
// thread with both loads in flight together; the caller syncs
template <bool BIAS>
ACCO_DEV void stage_params(u16* lds, const u16* w, const u16* b, int D) {
  for (int c = threadIdx.x; c < D / VEC; c += BLOCK) {
    reinterpret_cast<uint4*>(lds)[c] = reinterpret_cast<const uint4*>(w)[c];
    if constexpr (BIAS)
      reinterpret_cast<uint4*>(lds + D)[c] =
          reinterpret_cast<const uint4*>(b)[c];
  }
}

template <int CH>
ACCO_DEV void chunk_map(int lane, int tpg, int nv, int (&cid)[CH],
                        bool (&act)[CH]) {
#pragma unroll
  for (int j = 0; j < CH; ++j) {
    cid[j] = lane + j * tpg;
    act[j] = cid[j] < nv;
  }
}

// this thread's chunks of a staged parameter, as fp32
template <int CH>
ACCO_DEV void load_param(const u16* lds, const int (&cid)[CH],
                         const bool (&act)[CH], float (&f)[CH][VEC]) {
#pragma unroll
  for (int j = 0; j < CH; ++j)
    if (act[j]) load8(lds + cid[j] * VEC, f[j]);
}

// res fuses the residual add: s = bf16(x + res) is written to sum_out and
// the statistics/normalization run on s — one kernel replaces the eager
// add + norm pair (saves a full read+write pass of the hidden state per
// fusion site; the bf16 rounding of s matches the eager add).
ACCO_DEV void add_residual_round(float* xs, const u16* res) {
  float rr[VEC];
  load8(res, rr);
#pragma unroll
  for (int kk = 0; kk < VEC; ++kk)
    xs[kk] = bf16_to_f32(f32_to_bf16(xs[kk] + rr[kk]));
}

// o += the residual branch's grad chunk at p (folded into the dx write)
ACCO_DEV void fold_dadd(const u16* p, float* o) {
  float da[VEC];
  load8(p, da);
#pragma unroll
  for (int kk = 0; kk < VEC; ++kk) o[kk] += da[kk];
}

// one coalesced fp32 partial row; chunks that never saw a live row still
// write their zeros (the scratch is allocated w/ empty)
template <int CH>
ACCO_DEV void write_partial_row(float* out_row, const int (&cid)[CH],
                                const bool (&act)[CH],
                                const float (&acc)[CH][VEC]) {
#pragma unroll
  for (int j = 0; j < CH; ++j)
    if (act[j])
#pragma unroll
      for (int kk = 0; kk < VEC; ++kk) out_row[cid[j] * VEC + kk] = acc[j][kk];
}

// the 4 row groups' partials of one block → ONE partial row, through a
// 4·D fp32 LDS region nobody reads any more
template <int CH>
ACCO_DEV void combine_groups_through_lds(float* part, float* out_row, int g,
                                         int D, const int (&cid)[CH],
                                         const bool (&act)[CH],
                                         const float (&acc)[CH][VEC]) {
  __syncthreads();
  write_partial_row<CH>(part + g * D, cid, act, acc);
  __syncthreads();
  for (int c = threadIdx.x; c < D; c += BLOCK)
    out_row[c] = part[c] + part[D + c] + part[2 * D + c] + part[3 * D + c];
}

// The backward's per-element arithmetic, shared by both bwd kernels:
//   Rms: dx = r*(dy*w) - x * r^3/D * sum(dy*w*x);  dw_col = sum_rows dy*x*r
//   Ln:  xhat=(x-mean)*r; dyw=dy*w
//        dx = r*(dyw - mean(dyw) - xhat*mean(dyw*xhat)); dw=Σ dy*xhat; db=Σ dy
// First pass: the row sums; returns what the second pass needs of x (Ln: xhat)
template <class F>
ACCO_DEV float bwd_sums(float x, float ds, float wf, float mean, float r,
                        float& s1, float& s2) {
  if constexpr (F::kLayer) {
    const float xh = (x - mean) * r;
    const float dyw = ds * wf;
    s1 += dyw;
    s2 += dyw * xh;
    return xh;
  } else {
    s1 += ds * wf * x;
    return x;
  }
}

// Between the passes `reduce` sums s1 (and s2) over the row and turns them
// into the two row coefficients bwd_out takes: Ln (mean(dyw),
// mean(dyw*xhat)); Rms (coef = r^3/D * sum(dy*w*x), unused)
template <class F, class Reduce>
ACCO_DEV void bwd_reduce(float r, int D, float& s1, float& s2,
                         Reduce reduce) {
  if constexpr (F::kLayer) {
    s1 = reduce(s1) / (float)D;
    s2 = reduce(s2) / (float)D;
  } else {
    const float dot = reduce(s1);
    s1 = r * r * r * dot / (float)D;      // coef
  }
}

// Second pass: returns the dx element, accumulates dW (and dB)
template <class F>
ACCO_DEV float bwd_out(float xn, float ds, float wf, float r, float s1,
                       float s2, float& dw, float& db) {
  if constexpr (F::kLayer) {
    dw += ds * xn;
    db += ds;
    return r * (ds * wf - s1 - xn * s2);
  } else {
    dw += ds * xn * r;
    return r * ds * wf - xn * s1;
  }
}

// ------------------------------------------------------- grouped forward
// Rms: y = x·rstd·w.  Ln: y = (x-mean)·rstd·w + b, two-pass mean/variance.
// b and mean_out are unused (null) for Rms.
template <class F, int CH, int G>
__global__ __launch_bounds__(BLOCK)
void norm_fwd_kernel(const u16* __restrict__ x, const u16* __restrict__ w,
                     const u16* __restrict__ b, u16* __restrict__ y,
                     float* __restrict__ mean_out,
                     float* __restrict__ rstd_out,
                     const u16* __restrict__ res, u16* __restrict__ sum_out,
                     long long R, int D, float eps) {
  constexpr int TPG = BLOCK / G;
  __shared__ float lds[4];
  extern __shared__ __attribute__((aligned(16))) u16 wb_lds[];
  const int nv = D / VEC;
  stage_params<F::kLayer>(wb_lds, w, b, D);
  __syncthreads();

  const int g = threadIdx.x / TPG;
  const int lane = threadIdx.x % TPG;
  int cid[CH];
  bool act[CH];
  float wf[CH][VEC], bf[F::kLayer ? CH : 1][VEC];
  chunk_map<CH>(lane, TPG, nv, cid, act);
  // (w, b) chunk pairs read together: one load_param sweep per parameter
  // costs <Ln, 2, 1> two VGPRs and with them an occupancy step
#pragma unroll
  for (int j = 0; j < CH; ++j)
    if (act[j]) {
      load8(wb_lds + cid[j] * VEC, wf[j]);
      if constexpr (F::kLayer) load8(wb_lds + D + cid[j] * VEC, bf[j]);
    }

  for (long long base = (long long)blockIdx.x * G; base < R;
       base += (long long)gridDim.x * G) {
    const long long row = base + g;
    const bool live = row < R;
    const u16* xr = x + row * D;
    u16* yr = y + row * D;
    float xs[CH][VEC];
    float sum = 0.0f;                    // Rms: Σ x²;  Ln: Σ x
#pragma unroll
    for (int j = 0; j < CH; ++j)
      if (live && act[j]) {
        load8(xr + cid[j] * VEC, xs[j]);
        if (res != nullptr) {
          add_residual_round(xs[j], res + row * D + cid[j] * VEC);
          store8(sum_out + row * D + cid[j] * VEC, xs[j]);
        }
#pragma unroll
        for (int kk = 0; kk < VEC; ++kk) {
          if constexpr (F::kLayer) sum += xs[j][kk];
          else sum += xs[j][kk] * xs[j][kk];
        }
      }
    sum = group_reduce_sum<G>(sum, lds, g, lane);
    float mean = 0.0f, r;
    if constexpr (F::kLayer) {
      mean = sum / (float)D;
      float var = 0.0f;
#pragma unroll
      for (int j = 0; j < CH; ++j)
        if (live && act[j])
#pragma unroll
          for (int kk = 0; kk < VEC; ++kk) {
            float d = xs[j][kk] - mean;
            var += d * d;
          }
      var = group_reduce_sum<G>(var, lds, g, lane) / (float)D;
      r = rsqrtf(var + eps);
    } else {
      r = rsqrtf(sum / (float)D + eps);
    }
    if (live && lane == 0) {
      if (F::kLayer && mean_out) mean_out[row] = mean;
      if (rstd_out) rstd_out[row] = r;
    }
#pragma unroll
    for (int j = 0; j < CH; ++j)
      if (live && act[j]) {
        float o[VEC];
#pragma unroll
        for (int kk = 0; kk < VEC; ++kk) {
          if constexpr (F::kLayer)
            o[kk] = (xs[j][kk] - mean) * r * wf[j][kk] + bf[j][kk];
          else
            o[kk] = xs[j][kk] * r * wf[j][kk];
        }
        store8(yr + cid[j] * VEC, o);
      }
  }
}

// --------------------------------------- block-per-row bwd (nv > 128)
// One row per block per step, one partial row per block. mean_in and
// db_part are unused (null) for Rms. mean_in / rstd_in are deliberately not
// __restrict__: the row index is block-uniform, and with the no-alias
// promise the compiler turns the two reads into scalar loads that it sinks
// below the x/dy waits, exposing one load miss per row (24.6 against
// 24.1 us at R=8192, D=2048, RESULTS.md); without it they stay vector loads
// in flight together with x and dy.
template <class F, int CH>
__global__ __launch_bounds__(BLOCK)
void norm_bwd_kernel(const u16* __restrict__ dy, const u16* __restrict__ x,
                     const u16* __restrict__ w,
                     const float* mean_in,
                     const float* rstd_in, u16* __restrict__ dx,
                     float* __restrict__ dw_part,  // [grid, D] fp32
                     float* __restrict__ db_part,  // [grid, D] fp32
                     const u16* __restrict__ dadd,  // fused += residual grad
                     long long R, int D) {
  __shared__ float lds[4];
  extern __shared__ __attribute__((aligned(16))) u16 w_lds[];
  const int nv = D / VEC;
  stage_params<false>(w_lds, w, nullptr, D);
  __syncthreads();

  const int lane = threadIdx.x;
  int cid[CH];
  bool act[CH];
  float wf[CH][VEC], dwacc[CH][VEC] = {}, dbacc[F::kLayer ? CH : 1][VEC] = {};
  chunk_map<CH>(lane, BLOCK, nv, cid, act);
  load_param<CH>(w_lds, cid, act, wf);

  for (long long row = blockIdx.x; row < R; row += gridDim.x) {
    float mean = 0.0f;
    if constexpr (F::kLayer) mean = mean_in[row];
    const float r = rstd_in[row];
    float xn[CH][VEC], ds[CH][VEC];
    float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
    for (int j = 0; j < CH; ++j)
      if (act[j]) {
        // x straight into xn: through a temporary the compiler put a
        // vmcnt(0) between the x and the dy load (24.1 against 23.3 us)
        load8(x + row * D + cid[j] * VEC, xn[j]);
        load8(dy + row * D + cid[j] * VEC, ds[j]);
#pragma unroll
        for (int kk = 0; kk < VEC; ++kk)
          xn[j][kk] = bwd_sums<F>(xn[j][kk], ds[j][kk], wf[j][kk], mean, r,
                                  s1, s2);
      }
    bwd_reduce<F>(r, D, s1, s2, [&](float v) {
      return group_reduce_sum<1>(v, lds, 0, lane);
    });
#pragma unroll
    for (int j = 0; j < CH; ++j)
      if (act[j]) {
        float o[VEC];
#pragma unroll
        for (int kk = 0; kk < VEC; ++kk)
          o[kk] = bwd_out<F>(xn[j][kk], ds[j][kk], wf[j][kk], r, s1, s2,
                             dwacc[j][kk], dbacc[F::kLayer ? j : 0][kk]);
        if (dadd != nullptr) fold_dadd(dadd + row * D + cid[j] * VEC, o);
        store8(dx + row * D + cid[j] * VEC, o);
      }
  }
  write_partial_row<CH>(dw_part + (long long)blockIdx.x * D, cid, act, dwacc);
  if constexpr (F::kLayer)
    write_partial_row<CH>(db_part + (long long)blockIdx.x * D, cid, act,
                          dbacc);
}

// ------------------------------------------- wave-per-row bwd (nv ≤ 128)
// The block-per-row layout would split one row over 2-4 waves, paying 2
// barriers per cross-wave reduction and idling lanes at D=768 (96 of 128):
// measured 1.58 TB/s on the GPT-Neo LayerNorm bwd. This kernel gives each
// WAVE a whole row (zero barriers in the row loop, reductions are 6
// shfl_xor), runs 1024 blocks (4 waves/SIMD), and combines the block's 4
// per-group dW/dB partials through LDS at the end so the scratch stays at
// ≤1024 partial rows.
template <class F, int CH>
__global__ __launch_bounds__(BLOCK)
void norm_bwd_wr_kernel(const u16* __restrict__ dy, const u16* __restrict__ x,
                        const u16* __restrict__ w,
                        const float* __restrict__ mean_in,
                        const float* __restrict__ rstd_in,
                        u16* __restrict__ dx,
                        float* __restrict__ dw_part,  // [grid, D]
                        float* __restrict__ db_part,  // [grid, D]
                        const u16* __restrict__ dadd,
                        long long R, int D) {
  extern __shared__ __attribute__((aligned(16))) u16 w_lds[];  // 16·D bytes
  const int nv = D / VEC;
  stage_params<false>(w_lds, w, nullptr, D);
  __syncthreads();

  const int g = threadIdx.x >> 6;        // wave = row group
  const int lane = threadIdx.x & 63;
  int cid[CH];
  bool act[CH];
  float wf[CH][VEC], dwacc[CH][VEC] = {}, dbacc[F::kLayer ? CH : 1][VEC] = {};
  chunk_map<CH>(lane, 64, nv, cid, act);
  load_param<CH>(w_lds, cid, act, wf);

  // 1-deep software pipeline over rows: the next row's x/dy uint4 loads
  // (and its mean/rstd) issue before the current row's reductions, hiding
  // the ~900-cycle HBM latency under the shfl-reduce + epilogue (PMC
  // showed the plain loop 55% parked at waits)
  const long long stride = (long long)gridDim.x * 4;
  long long row = (long long)blockIdx.x * 4 + g;
  uint4 xv[CH], dv[CH];
  float mean = 0.f, r = 0.f;
  auto issue = [&](long long rw) {
#pragma unroll
    for (int j = 0; j < CH; ++j)
      if (act[j]) {
        xv[j] = *reinterpret_cast<const uint4*>(x + rw * D + cid[j] * VEC);
        dv[j] = *reinterpret_cast<const uint4*>(dy + rw * D + cid[j] * VEC);
      }
    if constexpr (F::kLayer) mean = mean_in[rw];
    r = rstd_in[rw];
  };
  auto unpack8 = [](const uint4& v, float* f) {
    const u16* u = reinterpret_cast<const u16*>(&v);
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) f[kk] = bf16_to_f32(u[kk]);
  };
  if (F::kPrefetch && row < R) issue(row);
  for (; row < R; row += stride) {
    float xn[CH][VEC], ds[CH][VEC];
    if constexpr (!F::kPrefetch) r = rstd_in[row];
    const float mean_c = mean, r_c = r;
    float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
    for (int j = 0; j < CH; ++j)
      if (act[j]) {
        float xs[VEC];
        if constexpr (F::kPrefetch) {
          unpack8(xv[j], xs);
          unpack8(dv[j], ds[j]);
        } else {
          load8(x + row * D + cid[j] * VEC, xs);
          load8(dy + row * D + cid[j] * VEC, ds[j]);
        }
#pragma unroll
        for (int kk = 0; kk < VEC; ++kk)
          xn[j][kk] = bwd_sums<F>(xs[kk], ds[j][kk], wf[j][kk], mean_c, r_c,
                                  s1, s2);
      }
    if (F::kPrefetch && row + stride < R)
      issue(row + stride);                       // in flight under reduce
    bwd_reduce<F>(r_c, D, s1, s2,
                  [](float v) { return wave_reduce_sum(v); });
#pragma unroll
    for (int j = 0; j < CH; ++j)
      if (act[j]) {
        float o[VEC];
#pragma unroll
        for (int kk = 0; kk < VEC; ++kk)
          o[kk] = bwd_out<F>(xn[j][kk], ds[j][kk], wf[j][kk], r_c, s1, s2,
                             dwacc[j][kk], dbacc[F::kLayer ? j : 0][kk]);
        if (dadd != nullptr) fold_dadd(dadd + row * D + cid[j] * VEC, o);
        store8(dx + row * D + cid[j] * VEC, o);
      }
  }

  // combine dW, then dB, through the LDS the weights no longer need
  float* part = reinterpret_cast<float*>(w_lds);
  combine_groups_through_lds<CH>(part, dw_part + (long long)blockIdx.x * D, g,
                                 D, cid, act, dwacc);
  if constexpr (F::kLayer)
    combine_groups_through_lds<CH>(part, db_part + (long long)blockIdx.x * D,
                                   g, D, cid, act, dbacc);
}

// ------------------------------------------------- column sum (dim-0 sum)
// out[d] = Σ_p in[p·D + d] for a [P, D] row-major matrix — the bias-wgrad
// reduce (the norm dW/dB partial rows go through norm_dw_finalize_kernel
// below instead). ATen's dim-0 reduce_kernel runs this at ~150 GB/s
// (20.8 µs on [1024,768] fp32); coalesced row sweeps with a P-split + fp32
// atomics reach the roofline.
// VECW consecutive columns per thread, 16-byte row loads (guide G13: a
// scalar-load version of this ran at 0.5 TB/s and regressed the GPT-Neo
// bias-wgrad path 4x vs ATen before being caught in the step profile)
template <typename Tin>
__global__ __launch_bounds__(BLOCK)
void colsum_kernel(const Tin* __restrict__ in, float* __restrict__ out,
                   long long P, int D) {
  constexpr int VECW = (sizeof(Tin) == 2) ? 8 : 4;   // 16 B per lane
  const int d0 = (blockIdx.x * BLOCK + threadIdx.x) * VECW;
  if (d0 >= D) return;
  const long long p0 = (long long)blockIdx.y * P / gridDim.y;
  const long long p1 = (long long)(blockIdx.y + 1) * P / gridDim.y;
  float acc[VECW];
#pragma unroll
  for (int k = 0; k < VECW; ++k) acc[k] = 0.0f;
  if (d0 + VECW <= D) {
    for (long long p = p0; p < p1; ++p) {
      if constexpr (sizeof(Tin) == 2) {
        const u16* row = (const u16*)in + p * D + d0;
        ushort4 a = reinterpret_cast<const ushort4*>(row)[0];
        ushort4 b = reinterpret_cast<const ushort4*>(row)[1];
        acc[0] += bf16_to_f32(a.x); acc[1] += bf16_to_f32(a.y);
        acc[2] += bf16_to_f32(a.z); acc[3] += bf16_to_f32(a.w);
        acc[4] += bf16_to_f32(b.x); acc[5] += bf16_to_f32(b.y);
        acc[6] += bf16_to_f32(b.z); acc[7] += bf16_to_f32(b.w);
      } else {
        const float4 v =
            *reinterpret_cast<const float4*>((const float*)in + p * D + d0);
        acc[0] += v.x; acc[1] += v.y; acc[2] += v.z; acc[3] += v.w;
      }
    }
  } else {
    for (long long p = p0; p < p1; ++p)      // ragged tail columns
#pragma unroll
      for (int k = 0; k < VECW; ++k)
        if (d0 + k < D) {
          if constexpr (sizeof(Tin) == 2)
            acc[k] += bf16_to_f32(((const u16*)in)[p * D + d0 + k]);
          else
            acc[k] += ((const float*)in)[p * D + d0 + k];
        }
  }
#pragma unroll
  for (int k = 0; k < VECW; ++k)
    if (d0 + k < D) atomicAdd(out + d0 + k, acc[k]);
}

// ------------------------------------- norm dW/dB partial-row finalize
// out[d] = Tw(Σ_p part[p·D + d]) for the [P, D] fp32 scratch the bwd
// kernels emit, written straight in the weight's dtype. A block owns 32
// columns (one 128-byte line per partial row) and walks ALL P rows with 32
// row slots × float4 lanes, then folds the slots through LDS — no atomics,
// so no zero-fill of the output and no separate cast launch (the colsum
// tail was at::zeros + colsum_kernel<float> + a bf16 cast per norm).
// blockIdx.y picks the (in, out) pair so LayerNorm's dW and dB share one
// launch.
constexpr int FIN_COLS = 32;              // columns per block
constexpr int FIN_SLOTS = BLOCK / (FIN_COLS / 4);   // 32 row slots

__global__ __launch_bounds__(BLOCK)
void norm_dw_finalize_kernel(const float* __restrict__ in0,
                             const float* __restrict__ in1,
                             void* __restrict__ out0, void* __restrict__ out1,
                             int P, int D, int out_bf16) {
  __shared__ float red[FIN_SLOTS][FIN_COLS + 4];
  const float* in = blockIdx.y == 0 ? in0 : in1;
  void* out = blockIdx.y == 0 ? out0 : out1;
  const int cx = threadIdx.x % (FIN_COLS / 4);
  const int slot = threadIdx.x / (FIN_COLS / 4);
  const int d0 = blockIdx.x * FIN_COLS + cx * 4;     // D % 8 == 0
  float4 a0 = make_float4(0.f, 0.f, 0.f, 0.f), a1 = a0, a2 = a0, a3 = a0;
  if (d0 < D) {
    const float* col = in + d0;
    int p = slot;
    for (; p + 3 * FIN_SLOTS < P; p += 4 * FIN_SLOTS) {
      const float4 v0 = *reinterpret_cast<const float4*>(col + (long long)p * D);
      const float4 v1 = *reinterpret_cast<const float4*>(
          col + (long long)(p + FIN_SLOTS) * D);
      const float4 v2 = *reinterpret_cast<const float4*>(
          col + (long long)(p + 2 * FIN_SLOTS) * D);
      const float4 v3 = *reinterpret_cast<const float4*>(
          col + (long long)(p + 3 * FIN_SLOTS) * D);
      a0.x += v0.x; a0.y += v0.y; a0.z += v0.z; a0.w += v0.w;
      a1.x += v1.x; a1.y += v1.y; a1.z += v1.z; a1.w += v1.w;
      a2.x += v2.x; a2.y += v2.y; a2.z += v2.z; a2.w += v2.w;
      a3.x += v3.x; a3.y += v3.y; a3.z += v3.z; a3.w += v3.w;
    }
    for (; p < P; p += FIN_SLOTS) {
      const float4 v0 = *reinterpret_cast<const float4*>(col + (long long)p * D);
      a0.x += v0.x; a0.y += v0.y; a0.z += v0.z; a0.w += v0.w;
    }
  }
  red[slot][cx * 4 + 0] = (a0.x + a1.x) + (a2.x + a3.x);
  red[slot][cx * 4 + 1] = (a0.y + a1.y) + (a2.y + a3.y);
  red[slot][cx * 4 + 2] = (a0.z + a1.z) + (a2.z + a3.z);
  red[slot][cx * 4 + 3] = (a0.w + a1.w) + (a2.w + a3.w);
  __syncthreads();
  if (threadIdx.x < FIN_COLS) {
    const int d = blockIdx.x * FIN_COLS + threadIdx.x;
    float sum = 0.0f;
#pragma unroll
    for (int sl = 0; sl < FIN_SLOTS; ++sl) sum += red[sl][threadIdx.x];
    if (d < D) {
      if (out_bf16) reinterpret_cast<u16*>(out)[d] = f32_to_bf16(sum);
      else reinterpret_cast<float*>(out)[d] = sum;
    }
  }
}

// ------------------------------------------------------------ launch side
int groups_for(int D) {
  const int nv = D / VEC;
  if (nv <= 64) return 4;      // one wave per row
  if (nv <= 128) return 2;     // two waves per row (e.g. gptneo D=768)
  return 1;
}

int chunks_for(int D) {
  const int nv = D / VEC;
  if (nv <= BLOCK) return 1;
  if (nv <= 2 * BLOCK) return 2;
  if (nv <= 4 * BLOCK) return 4;
  return 8;
}

int fwd_blocks(long long R, int G) {
  long long b = (R + G - 1) / G;
  const long long cap = 8192 / G;
  return (int)((b < cap) ? (b < 1 ? 1 : b) : cap);
}

// block-per-row bwd: one row and one partial row per block
int bwd_blocks(long long R) {
  // cap partial rows at 1024: the [partials, D] fp32 scratch write + its
  // finalize read is ~25% of bwd traffic at 2048 partials and halves here,
  // while 1024 blocks x 4 waves still fill all 1024 SIMDs
  return (int)((R < 1024) ? (R < 1 ? 1 : R) : 1024);
}

// wave-per-row bwd (nv ≤ 128): 4 rows per block, 1 partial row per block
bool use_wr(int D) { return D / VEC <= 128; }

int wr_blocks(long long R) {
  long long b = (R + 3) / 4;
  return (int)((b < 1024) ? (b < 1 ? 1 : b) : 1024);
}

// Compile-time CH and G reach the launch lambdas as integral_constant values
template <int N> using Int = std::integral_constant<int, N>;

// chunks_for(D) → launch(Int<CH>): the one-row-per-block layouts
template <class Launch>
void dispatch_chunks(int D, Launch&& launch) {
  switch (chunks_for(D)) {
    case 1: launch(Int<1>{}); break;
    case 2: launch(Int<2>{}); break;
    case 4: launch(Int<4>{}); break;
    default: launch(Int<8>{}); break;
  }
}

template <class F>
void launch_norm_fwd(const void* x, const void* w, const void* b, void* y,
                     void* mean, void* rstd, const void* res, void* sum_out,
                     long long R, int D, float eps, hipStream_t s) {
  const int lds = (F::kLayer ? 2 : 1) * D * sizeof(u16);
  auto launch = [&](auto ch, auto g) {
    constexpr int CH = decltype(ch)::value, G = decltype(g)::value;
    hipLaunchKernelGGL((norm_fwd_kernel<F, CH, G>), dim3(fwd_blocks(R, G)),
                       dim3(BLOCK), lds, s, (const u16*)x, (const u16*)w,
                       (const u16*)b, (u16*)y, (float*)mean, (float*)rstd,
                       (const u16*)res, (u16*)sum_out, R, D, eps);
  };
  switch (groups_for(D)) {
    case 4: launch(Int<1>{}, Int<4>{}); break;
    case 2: launch(Int<1>{}, Int<2>{}); break;
    default:
      dispatch_chunks(D, [&](auto ch) { launch(ch, Int<1>{}); });
  }
}

template <class F>
void launch_norm_bwd(const void* dy, const void* x, const void* w,
                     const void* mean, const void* rstd, void* dx,
                     void* dw_fp32, void* db_fp32, const void* dadd,
                     long long R, int D, hipStream_t s) {
  auto block_per_row = [&](auto ch) {
    hipLaunchKernelGGL((norm_bwd_kernel<F, decltype(ch)::value>),
                       dim3(bwd_blocks(R)), dim3(BLOCK), D * sizeof(u16), s,
                       (const u16*)dy, (const u16*)x, (const u16*)w,
                       (const float*)mean, (const float*)rstd, (u16*)dx,
                       (float*)dw_fp32, (float*)db_fp32, (const u16*)dadd,
                       R, D);
  };
  // 64 lanes per row; LDS: 4 fp32 partial rows (≥ the staged weights)
  auto wave_per_row = [&](auto ch) {
    hipLaunchKernelGGL((norm_bwd_wr_kernel<F, decltype(ch)::value>),
                       dim3(wr_blocks(R)), dim3(BLOCK), 16 * D, s,
                       (const u16*)dy, (const u16*)x, (const u16*)w,
                       (const float*)mean, (const float*)rstd, (u16*)dx,
                       (float*)dw_fp32, (float*)db_fp32, (const u16*)dadd,
                       R, D);
  };
  if (!use_wr(D)) dispatch_chunks(D, block_per_row);
  else if (D / VEC <= 64) wave_per_row(Int<1>{});
  else wave_per_row(Int<2>{});
}

}  // namespace

extern "C" {

// dW (and optionally dB) partial rows [P, D] fp32 → [D] in the weight dtype
void acco_norm_dw_finalize(const float* dw_part, const float* db_part,
                           void* dw, void* db, int P, int D, bool out_bf16,
                           hipStream_t s) {
  dim3 grid((D + FIN_COLS - 1) / FIN_COLS, db_part != nullptr ? 2 : 1);
  hipLaunchKernelGGL(norm_dw_finalize_kernel, grid, dim3(BLOCK), 0, s,
                     dw_part, db_part, dw, db, P, D, out_bf16 ? 1 : 0);
}

void acco_colsum(const void* in, float* out, long long P, int D,
                 bool in_is_bf16, hipStream_t s) {
  const int vecw = in_is_bf16 ? 8 : 4;
  const int xblocks = (D + BLOCK * vecw - 1) / (BLOCK * vecw);
  // split P so the grid covers the chip even at small D (out is zeroed by
  // the caller; partial sums combine via fp32 atomics)
  int ysplit = (int)(512 / (xblocks < 1 ? 1 : xblocks));
  if (ysplit < 1) ysplit = 1;
  if ((long long)ysplit > P) ysplit = (int)(P < 1 ? 1 : P);
  dim3 grid(xblocks, ysplit);
  if (in_is_bf16)
    hipLaunchKernelGGL((colsum_kernel<u16>), grid, dim3(BLOCK), 0, s,
                       (const u16*)in, out, P, D);
  else
    hipLaunchKernelGGL((colsum_kernel<float>), grid, dim3(BLOCK), 0, s,
                       (const float*)in, out, P, D);
}

// number of fp32 partial rows the bwd kernels emit (scratch allocation)
int acco_norm_bwd_grid(long long R, int D) {
  return use_wr(D) ? wr_blocks(R) : bwd_blocks(R);
}

void acco_rmsnorm_fwd(const void* x, const void* w, void* y, void* rstd,
                      const void* res, void* sum_out,
                      long long R, int D, float eps, hipStream_t s) {
  launch_norm_fwd<Rms>(x, w, nullptr, y, nullptr, rstd, res, sum_out, R, D,
                       eps, s);
}

void acco_rmsnorm_bwd(const void* dy, const void* x, const void* w,
                      const void* rstd, void* dx, void* dw_fp32,
                      const void* dadd, long long R, int D, hipStream_t s) {
  launch_norm_bwd<Rms>(dy, x, w, nullptr, rstd, dx, dw_fp32, nullptr, dadd, R,
                       D, s);
}

void acco_layernorm_fwd(const void* x, const void* w, const void* b, void* y,
                        void* mean, void* rstd, const void* res,
                        void* sum_out, long long R, int D, float eps,
                        hipStream_t s) {
  launch_norm_fwd<Ln>(x, w, b, y, mean, rstd, res, sum_out, R, D, eps, s);
}

void acco_layernorm_bwd(const void* dy, const void* x, const void* w,
                        const void* mean, const void* rstd, void* dx,
                        void* dw_fp32, void* db_fp32, const void* dadd,
                        long long R, int D, hipStream_t s) {
  launch_norm_bwd<Ln>(dy, x, w, mean, rstd, dx, dw_fp32, db_fp32, dadd, R, D,
                      s);
}

}  // extern "C"
