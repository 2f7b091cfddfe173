// Python bindings for the acco_amd gfx950 HIP kernels.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <c10/hip/HIPException.h>

#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"

namespace {

using u16 = unsigned short;

// base pointer on a multiple of the vector width the kernel loads with
static bool aligned_to(const at::Tensor& t, size_t bytes) {
  return reinterpret_cast<uintptr_t>(t.data_ptr()) % bytes == 0;
}

// one fp32 element on ref's device
static void check_dev_scalar(const at::Tensor& t, const at::Tensor& ref,
                             const char* name) {
  TORCH_CHECK(t.is_cuda() && t.device() == ref.device() &&
              t.scalar_type() == at::kFloat && t.numel() == 1, name,
              " must be one fp32 on ", ref.device(), ", got ",
              t.scalar_type(), " ", t.sizes(), " on ", t.device());
}

// contiguous CUDA fp32 with n elements on ref's device
static void check_f32_vec(const at::Tensor& t, int64_t n,
                          const at::Tensor& ref, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.device() == ref.device() &&
              t.scalar_type() == at::kFloat && t.is_contiguous() &&
              t.numel() == n, name, " must be contiguous CUDA fp32 with ", n,
              " elements on ", ref.device(), ", got ", t.scalar_type(), " ",
              t.sizes(), " on ", t.device());
}

// The argument contract of the fused AdamW: p, m, v contiguous CUDA fp32 of
// one numel on one device, 16-byte aligned (float4 accesses); g (and out,
// when given) contiguous bf16 or fp32 of that numel on that device, aligned
// to 4 elements; scale_dev, when given, one fp32 on that device.
void fused_adamw(at::Tensor p, at::Tensor g, at::Tensor m, at::Tensor v,
                 int64_t step, double lr, double beta1, double beta2,
                 double eps, double weight_decay, double scale,
                 at::Tensor scale_dev, at::Tensor out, bool commit) {
  TORCH_CHECK(p.is_cuda() && p.scalar_type() == at::kFloat && p.is_contiguous(),
              "p must be contiguous CUDA fp32");
  auto check_state = [&](const at::Tensor& t, const char* name) {
    TORCH_CHECK(t.is_cuda() && t.device() == p.device() &&
                t.scalar_type() == at::kFloat && t.is_contiguous() &&
                t.numel() == p.numel(), name, " must be contiguous CUDA fp32 "
                "with p's numel (", p.numel(), ") on ", p.device(), ", got ",
                t.scalar_type(), " ", t.sizes(), " on ", t.device());
  };
  check_state(m, "m");
  check_state(v, "v");
  TORCH_CHECK(step >= 0, "step must be >= 0, got ", step);
  const bool bf16 = g.scalar_type() == at::kBFloat16;
  TORCH_CHECK(bf16 || g.scalar_type() == at::kFloat,
              "grad must be bf16 or fp32");
  TORCH_CHECK(g.device() == p.device() && g.numel() == p.numel() &&
              g.is_contiguous(), "g must be contiguous with p's numel (",
              p.numel(), ") on ", p.device(), ", got ", g.sizes(), " on ",
              g.device());
  const size_t buf_align = bf16 ? 8 : 16;
  TORCH_CHECK(aligned_to(p, 16) && aligned_to(m, 16) && aligned_to(v, 16),
              "p, m, v must be 16-byte aligned");
  TORCH_CHECK(aligned_to(g, buf_align), "g must be ", buf_align,
              "-byte aligned");
  void* out_ptr = nullptr;
  if (out.numel() > 0) {
    TORCH_CHECK(out.device() == p.device() && out.numel() == p.numel() &&
                out.is_contiguous(), "out must be contiguous with p's numel (",
                p.numel(), ") on ", p.device(), ", got ", out.sizes(), " on ",
                out.device());
    TORCH_CHECK(out.scalar_type() == g.scalar_type(),
                "out dtype must match grad (com-buffer) dtype");
    TORCH_CHECK(aligned_to(out, buf_align), "out must be ", buf_align,
                "-byte aligned");
    out_ptr = out.data_ptr();
  }
  const float* sd = nullptr;
  if (scale_dev.numel() > 0) {
    check_dev_scalar(scale_dev, p, "scale_dev");
    sd = scale_dev.data_ptr<float>();
  }
  if (p.numel() == 0) return;
  auto stream = at::hip::getCurrentHIPStream();
  acco_fused_adamw_launch(p.data_ptr(), g.data_ptr(), m.data_ptr(),
                          v.data_ptr(), out_ptr, sd, (long long)p.numel(),
                          bf16, commit, (float)scale, (float)lr, (float)beta1,
                          (float)beta2, (float)eps, (float)weight_decay,
                          step + 1, stream.stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

// ---- gradient sum of squares (global grad-norm clipping)
// The argument contract: g contiguous CUDA bf16 or fp32, 16-byte aligned
// (16-byte vector loads); partials contiguous CUDA fp32 on g's device with
// at least grad_sumsq_grid(n) elements. Returns the number of partials
// written, partials[0 .. grid); the rest of the workspace is not touched.
int64_t grad_sumsq_grid(int64_t n, bool is_bf16) {
  TORCH_CHECK(n >= 0, "n must be >= 0, got ", n);
  return acco_grad_sumsq_grid((long long)n, is_bf16);
}

int64_t grad_sumsq(at::Tensor g, at::Tensor partials) {
  const bool bf16 = g.scalar_type() == at::kBFloat16;
  TORCH_CHECK(g.is_cuda() && (bf16 || g.scalar_type() == at::kFloat) &&
              g.is_contiguous(), "g must be contiguous CUDA bf16 or fp32, "
              "got ", g.scalar_type(), " on ", g.device());
  TORCH_CHECK(aligned_to(g, 16), "g must be 16-byte aligned");
  const int grid = acco_grad_sumsq_grid((long long)g.numel(), bf16);
  TORCH_CHECK(partials.is_cuda() && partials.device() == g.device() &&
              partials.scalar_type() == at::kFloat &&
              partials.is_contiguous() && partials.numel() >= grid,
              "partials must be contiguous CUDA fp32 with at least ", grid,
              " elements on ", g.device(), ", got ", partials.scalar_type(),
              " ", partials.sizes(), " on ", partials.device());
  acco_grad_sumsq(g.data_ptr(), partials.data_ptr<float>(),
                  (long long)g.numel(), bf16,
                  at::hip::getCurrentHIPStream().stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return grid;
}

// out[0] = sum of every element of partials (double accumulation, fixed
// order); partials contiguous CUDA fp32, out one fp32 on its device
void sumsq_finalize(at::Tensor partials, at::Tensor out) {
  TORCH_CHECK(partials.is_cuda() && partials.scalar_type() == at::kFloat &&
              partials.is_contiguous(), "partials must be contiguous CUDA "
              "fp32, got ", partials.scalar_type(), " on ", partials.device());
  check_dev_scalar(out, partials, "out");
  acco_sumsq_finalize(partials.data_ptr<float>(), (long long)partials.numel(),
                      out.data_ptr<float>(),
                      at::hip::getCurrentHIPStream().stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

at::Tensor colsum(at::Tensor in) {
  TORCH_CHECK(in.dim() == 2 && in.is_contiguous() && in.is_cuda());
  TORCH_CHECK(in.scalar_type() == at::kBFloat16 ||
              in.scalar_type() == at::kFloat);
  const long long P = in.size(0);
  const int D = (int)in.size(1);
  auto out = at::zeros({D}, in.options().dtype(at::kFloat));
  acco_colsum(in.data_ptr(), out.data_ptr<float>(), P, D,
              in.scalar_type() == at::kBFloat16,
              at::hip::getCurrentHIPStream().stream());
  return out;
}

#define CHECK_BF16_CONTIG(t) \
  TORCH_CHECK((t).is_cuda() && (t).scalar_type() == at::kBFloat16 && \
              (t).is_contiguous(), #t " must be contiguous CUDA bf16")

static hipStream_t cur_stream() {
  return at::hip::getCurrentHIPStream().stream();
}

// fp32 [>=S, D] contiguous cos/sin tables on the same device as `like`
static void check_rope_table(const at::Tensor& cos_t, const at::Tensor& sin_t,
                             int64_t S, int64_t D, const at::Tensor& like) {
  TORCH_CHECK(cos_t.is_cuda() && sin_t.is_cuda() &&
              cos_t.device() == like.device() &&
              sin_t.device() == like.device());
  TORCH_CHECK(cos_t.scalar_type() == at::kFloat && cos_t.is_contiguous() &&
              sin_t.scalar_type() == at::kFloat && sin_t.is_contiguous());
  TORCH_CHECK(cos_t.dim() == 2 && cos_t.size(0) >= S && cos_t.size(1) == D &&
              sin_t.sizes() == cos_t.sizes(),
              "cos/sin must be fp32 [>=S, D]");
}

// ---- SwiGLU / gelu_new
// The input of an elementwise kernel: contiguous CUDA bf16, at least 1-D,
// whole 8-element vectors per row (`last_mult` = 16 for the packed [.., 2I]
// layout, whose two halves are each read as vectors).
static void check_ew_input(const at::Tensor& x, const char* name,
                           int64_t last_mult) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16 &&
              x.is_contiguous(), name, " must be contiguous CUDA bf16");
  TORCH_CHECK(x.dim() >= 1 && x.size(-1) % last_mult == 0 &&
              x.numel() % 8 == 0, name, " must be at least 1-D with a last "
              "dimension that is a multiple of ", last_mult, ", got ",
              x.sizes());
}

// `t` (u against g, dout against the output): contiguous CUDA bf16 of
// exactly `sizes` on ref's device
static void check_ew_like(const at::Tensor& ref, at::IntArrayRef sizes,
                          const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kBFloat16 &&
              t.is_contiguous(), name, " must be contiguous CUDA bf16");
  TORCH_CHECK(t.device() == ref.device() && t.sizes() == sizes, name,
              ": expected ", sizes, " on ", ref.device(), ", got ", t.sizes(),
              " on ", t.device());
}

at::Tensor swiglu_fwd(at::Tensor g, at::Tensor u) {
  check_ew_input(g, "g", 8);
  check_ew_like(g, g.sizes(), u, "u");
  const int I = (int)g.size(-1);
  auto out = at::empty_like(g);
  if (g.numel() == 0) return out;
  acco_swiglu_fwd(g.data_ptr(), u.data_ptr(), out.data_ptr(), g.numel(),
                  I, I / 8, cur_stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return out;
}

std::vector<at::Tensor> swiglu_bwd(at::Tensor dout, at::Tensor g, at::Tensor u) {
  check_ew_input(g, "g", 8);
  check_ew_like(g, g.sizes(), u, "u");
  check_ew_like(g, g.sizes(), dout, "dout");
  const int I = (int)g.size(-1);
  auto dg = at::empty_like(g);
  auto du = at::empty_like(u);
  if (g.numel() == 0) return {dg, du};
  acco_swiglu_bwd(dout.data_ptr(), g.data_ptr(), u.data_ptr(), dg.data_ptr(),
                  du.data_ptr(), g.numel(), I, I / 8, cur_stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {dg, du};
}

// sizes of the packed SwiGLU's output: gu's with the last dimension halved
static std::vector<int64_t> packed_out_sizes(const at::Tensor& gu) {
  auto sizes = gu.sizes().vec();
  sizes.back() /= 2;
  return sizes;
}

// SwiGLU over the packed [rows, 2I] fused gate_up projection output:
// out = silu(gu[:, :I]) * gu[:, I:]; backward emits dgu in one pass
// (no torch.split → no contiguous copies forward, no cat backward).
at::Tensor swiglu_packed_fwd(at::Tensor gu) {
  check_ew_input(gu, "gu", 16);
  const int twoI = (int)gu.size(-1);
  const int I = twoI / 2;
  auto out = at::empty(packed_out_sizes(gu), gu.options());
  if (gu.numel() == 0) return out;
  const u16* base = (const u16*)gu.data_ptr();
  acco_swiglu_fwd(base, base + I, out.data_ptr(), gu.numel() / 2, I,
                  twoI / 8, cur_stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return out;
}

at::Tensor swiglu_packed_bwd(at::Tensor dout, at::Tensor gu) {
  check_ew_input(gu, "gu", 16);
  check_ew_like(gu, packed_out_sizes(gu), dout, "dout");
  const int twoI = (int)gu.size(-1);
  const int I = twoI / 2;
  auto dgu = at::empty_like(gu);
  if (gu.numel() == 0) return dgu;
  const u16* base = (const u16*)gu.data_ptr();
  u16* dbase = (u16*)dgu.data_ptr();
  acco_swiglu_bwd(dout.data_ptr(), base, base + I, dbase, dbase + I,
                  gu.numel() / 2, I, twoI / 8, cur_stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return dgu;
}

at::Tensor gelu_fwd(at::Tensor x) {
  check_ew_input(x, "x", 8);
  auto out = at::empty_like(x);
  if (x.numel() == 0) return out;
  acco_gelu_fwd(x.data_ptr(), out.data_ptr(), x.numel(), cur_stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return out;
}

at::Tensor gelu_bwd(at::Tensor dout, at::Tensor x) {
  check_ew_input(x, "x", 8);
  check_ew_like(x, x.sizes(), dout, "dout");
  auto dx = at::empty_like(x);
  if (x.numel() == 0) return dx;
  acco_gelu_bwd(dout.data_ptr(), x.data_ptr(), dx.data_ptr(), x.numel(),
                cur_stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return dx;
}

// ---- RMSNorm / LayerNorm
struct NormShape { long long R; int D; };

// The argument contract of every norm entry point, forward and backward:
// D % 8 == 0 (16-byte vector loads), D <= 16384 (8 chunks of 256 lanes),
// x's last dimension is D = w.numel(); each `like_x` that is given (dy, res, dadd) is bf16 of x's
// numel on x's device; every saved row statistic is a contiguous fp32 [R]
// on x's device.
static NormShape check_norm_args(
    const at::Tensor& x, const at::Tensor& w,
    std::initializer_list<c10::optional<at::Tensor>> like_x,
    std::initializer_list<at::Tensor> stats = {}) {
  CHECK_BF16_CONTIG(x); CHECK_BF16_CONTIG(w);
  const long long D = w.numel();
  TORCH_CHECK(D > 0 && D % 8 == 0 && D <= 16384 && x.numel() % D == 0 &&
              w.device() == x.device(),
              "norm width must be a multiple of 8, at most 16384, and divide "
              "x.numel(); got D=", D, " x.numel()=", x.numel());
  // a w of half the width divides x.numel() too and would norm half rows
  TORCH_CHECK(x.dim() >= 1 && x.size(-1) == D, "w must hold one element per "
              "column of x; got w.numel()=", D, " x ", x.sizes());
  const long long R = x.numel() / D;
  for (const auto& t : like_x)
    if (t.has_value()) {
      CHECK_BF16_CONTIG(*t);
      TORCH_CHECK(t->numel() == x.numel() && t->device() == x.device(),
                  "dy/res/dadd must have x's numel and device");
    }
  for (const at::Tensor& st : stats)
    TORCH_CHECK(st.is_cuda() && st.device() == x.device() &&
                st.scalar_type() == at::kFloat && st.is_contiguous() &&
                st.numel() == R,
                "mean/rstd must be contiguous CUDA fp32 with one element per "
                "row (", R, "), got ", st.numel());
  return {R, (int)D};
}

static const void* ptr_or_null(const c10::optional<at::Tensor>& t) {
  return t.has_value() ? t->data_ptr() : nullptr;
}

// res given: fused residual add, s = bf16(x + res), y = rmsnorm(s)·w
static std::vector<at::Tensor> rmsnorm_fwd_impl(
    const at::Tensor& x, const c10::optional<at::Tensor>& res,
    const at::Tensor& w, double eps) {
  const auto [R, D] = check_norm_args(x, w, {res});
  auto y = at::empty_like(x);
  auto rstd = at::empty({R}, x.options().dtype(at::kFloat));
  at::Tensor sum_out = res.has_value() ? at::empty_like(x) : at::Tensor();
  acco_rmsnorm_fwd(x.data_ptr(), w.data_ptr(), y.data_ptr(), rstd.data_ptr(),
                   ptr_or_null(res),
                   res.has_value() ? sum_out.data_ptr() : nullptr, R, D,
                   (float)eps, cur_stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  if (res.has_value()) return {y, sum_out, rstd};
  return {y, rstd};
}

std::vector<at::Tensor> rmsnorm_fwd(at::Tensor x, at::Tensor w, double eps) {
  return rmsnorm_fwd_impl(x, c10::nullopt, w, eps);
}

std::vector<at::Tensor> add_rmsnorm_fwd(at::Tensor x, at::Tensor res,
                                        at::Tensor w, double eps) {
  return rmsnorm_fwd_impl(x, res, w, eps);
}

std::vector<at::Tensor> rmsnorm_bwd(at::Tensor dy, at::Tensor x, at::Tensor w,
                                    at::Tensor rstd,
                                    c10::optional<at::Tensor> dadd) {
  const auto [R, D] = check_norm_args(x, w, {dy, dadd}, {rstd});
  auto dx = at::empty_like(x);
  const int grid = acco_norm_bwd_grid(R, D);
  auto dw_part = at::empty({grid, D}, x.options().dtype(at::kFloat));
  acco_rmsnorm_bwd(dy.data_ptr(), x.data_ptr(), w.data_ptr(),
                   rstd.data_ptr(), dx.data_ptr(), dw_part.data_ptr(),
                   ptr_or_null(dadd), R, D, cur_stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  // one launch: partial rows → dW in the weight's dtype (no zero-fill, no
  // atomics, no cast)
  auto dw = at::empty({D}, w.options());
  acco_norm_dw_finalize(dw_part.data_ptr<float>(), nullptr, dw.data_ptr(),
                        nullptr, grid, D, true, cur_stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {dx, dw};
}

// res given: fused residual add, s = bf16(x + res), y = ln(s)·w + b
static std::vector<at::Tensor> layernorm_fwd_impl(
    const at::Tensor& x, const c10::optional<at::Tensor>& res,
    const at::Tensor& w, const at::Tensor& b, double eps) {
  const auto [R, D] = check_norm_args(x, w, {res});
  CHECK_BF16_CONTIG(b);
  TORCH_CHECK(b.numel() == D && b.device() == x.device());
  auto y = at::empty_like(x);
  auto mean = at::empty({R}, x.options().dtype(at::kFloat));
  auto rstd = at::empty({R}, x.options().dtype(at::kFloat));
  at::Tensor sum_out = res.has_value() ? at::empty_like(x) : at::Tensor();
  acco_layernorm_fwd(x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(),
                     mean.data_ptr(), rstd.data_ptr(), ptr_or_null(res),
                     res.has_value() ? sum_out.data_ptr() : nullptr, R, D,
                     (float)eps, cur_stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  if (res.has_value()) return {y, sum_out, mean, rstd};
  return {y, mean, rstd};
}

std::vector<at::Tensor> layernorm_fwd(at::Tensor x, at::Tensor w, at::Tensor b,
                                      double eps) {
  return layernorm_fwd_impl(x, c10::nullopt, w, b, eps);
}

std::vector<at::Tensor> add_layernorm_fwd(at::Tensor x, at::Tensor res,
                                          at::Tensor w, at::Tensor b,
                                          double eps) {
  return layernorm_fwd_impl(x, res, w, b, eps);
}

std::vector<at::Tensor> layernorm_bwd(at::Tensor dy, at::Tensor x,
                                      at::Tensor w, at::Tensor mean,
                                      at::Tensor rstd,
                                      c10::optional<at::Tensor> dadd) {
  const auto [R, D] = check_norm_args(x, w, {dy, dadd}, {mean, rstd});
  auto dx = at::empty_like(x);
  const int grid = acco_norm_bwd_grid(R, D);
  auto dw_part = at::empty({grid, D}, x.options().dtype(at::kFloat));
  auto db_part = at::empty({grid, D}, x.options().dtype(at::kFloat));
  acco_layernorm_bwd(dy.data_ptr(), x.data_ptr(), w.data_ptr(),
                     mean.data_ptr(), rstd.data_ptr(), dx.data_ptr(),
                     dw_part.data_ptr(), db_part.data_ptr(), ptr_or_null(dadd),
                     R, D, cur_stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  auto dw = at::empty({D}, w.options());
  auto db = at::empty({D}, w.options());
  acco_norm_dw_finalize(dw_part.data_ptr<float>(), db_part.data_ptr<float>(),
                        dw.data_ptr(), db.data_ptr(), grid, D, true,
                        cur_stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {dx, dw, db};
}

// ---- RoPE ([B, S, H, D] contiguous)
at::Tensor rope_fwd(at::Tensor x, at::Tensor cos_t, at::Tensor sin_t,
                    bool bwd) {
  CHECK_BF16_CONTIG(x);
  TORCH_CHECK(x.dim() == 4 && x.size(3) % 8 == 0 && x.size(1) < (1LL << 31),
              "x must be [B,S,H,D] with D % 8 == 0, got ", x.sizes());
  const long long B = x.size(0);
  const int S = (int)x.size(1), H = (int)x.size(2), D = (int)x.size(3);
  check_rope_table(cos_t, sin_t, S, D, x);
  auto y = at::empty_like(x);
  if (x.numel() == 0) return y;
  acco_rope(x.data_ptr(), y.data_ptr(), cos_t.data_ptr<float>(),
            sin_t.data_ptr<float>(), B, S, H, D, bwd,
            (long long)H * D, cur_stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return y;
}

// ---- fused causal-LM CE (ce.hip): whole [B, S, V] logits, labels shifted
// by the kernels
struct CeShape { long long T; int S, V; };

// The argument contract of the shifted CE entry points: logits contiguous
// CUDA bf16 [B, S, V] on a 16-byte aligned base; labels contiguous int64
// [B, S] on the logits' device (a label outside [0, V) is an ignored token);
// in the backward, lse contiguous fp32 with one element per token and acc
// fp32 {loss_sum, n_valid, ...}, both on that device.
static CeShape check_ce_args(const at::Tensor& logits,
                             const at::Tensor& labels,
                             const at::Tensor* lse = nullptr,
                             const at::Tensor* acc = nullptr) {
  CHECK_BF16_CONTIG(logits);
  TORCH_CHECK(logits.dim() == 3 && logits.size(1) < (1LL << 31) &&
              logits.size(2) > 0 && logits.size(2) < (1LL << 31),
              "logits must be [B,S,V] with V > 0, got ", logits.sizes());
  TORCH_CHECK(aligned_to(logits, 16), "logits must be 16-byte aligned");
  const int64_t B = logits.size(0), S = logits.size(1);
  TORCH_CHECK(labels.is_cuda() && labels.device() == logits.device() &&
              labels.scalar_type() == at::kLong && labels.is_contiguous() &&
              labels.dim() == 2 && labels.size(0) == B && labels.size(1) == S,
              "labels must be contiguous int64 [B, S] = [", B, ", ", S,
              "] on ", logits.device(), ", got ", labels.scalar_type(), " ",
              labels.sizes(), " on ", labels.device());
  if (lse != nullptr) check_f32_vec(*lse, B * S, logits, "lse");
  if (acc != nullptr)
    TORCH_CHECK(acc->is_cuda() && acc->device() == logits.device() &&
                acc->scalar_type() == at::kFloat && acc->is_contiguous() &&
                acc->numel() >= 2, "acc must be contiguous CUDA fp32 "
                "{loss_sum, n_valid} on ", logits.device(), ", got ",
                acc->scalar_type(), " ", acc->sizes(), " on ", acc->device());
  return {(long long)(B * S), (int)S, (int)logits.size(2)};
}

std::vector<at::Tensor> ce_fwd(at::Tensor logits, at::Tensor labels,
                               double epsilon) {
  const auto [T, S, V] = check_ce_args(logits, labels);
  auto lse = at::empty({T}, logits.options().dtype(at::kFloat));
  // 128 accumulator shards (atomic-contention fix in ce.hip) reduced here
  auto accs = at::zeros({128, 2}, logits.options().dtype(at::kFloat));
  if (T == 0) return {accs.sum(0), lse};
  acco_ce_fwd(logits.data_ptr(),
              reinterpret_cast<const long long*>(labels.data_ptr<int64_t>()),
              lse.data_ptr<float>(), accs.data_ptr<float>(), T, S, V,
              (float)epsilon, cur_stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {accs.sum(0), lse};
}

// dloss from the host, or from dloss_dev (one fp32 on the device) when given
static at::Tensor ce_bwd_impl(const at::Tensor& logits,
                              const at::Tensor& labels, const at::Tensor& lse,
                              const at::Tensor& acc, double dloss,
                              const at::Tensor* dloss_dev, double epsilon) {
  const auto [T, S, V] = check_ce_args(logits, labels, &lse, &acc);
  if (dloss_dev != nullptr) check_dev_scalar(*dloss_dev, logits, "dloss_dev");
  auto dlogits = at::empty_like(logits);
  if (T == 0) return dlogits;
  acco_ce_bwd(logits.data_ptr(),
              reinterpret_cast<const long long*>(labels.data_ptr<int64_t>()),
              lse.data_ptr<float>(), dlogits.data_ptr(),
              acc.data_ptr<float>(), (float)dloss,
              dloss_dev != nullptr ? dloss_dev->data_ptr<float>() : nullptr,
              T, S, V, (float)epsilon, cur_stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return dlogits;
}

at::Tensor ce_bwd(at::Tensor logits, at::Tensor labels, at::Tensor lse,
                  at::Tensor acc, double dloss, double epsilon) {
  return ce_bwd_impl(logits, labels, lse, acc, dloss, nullptr, epsilon);
}

// dloss read from a 1-elem fp32 device tensor: no D2H sync in backward
at::Tensor ce_bwd_dev(at::Tensor logits, at::Tensor labels, at::Tensor lse,
                      at::Tensor acc, at::Tensor dloss_dev, double epsilon) {
  return ce_bwd_impl(logits, labels, lse, acc, 0.0, &dloss_dev, epsilon);
}

// ---- the same kernels on rows (ce.hip): the chunked lm_head + loss path
struct CeRowsShape { long long T; int V; };

// The argument contract of the row-wise CE entry points: logits contiguous
// CUDA bf16 [T, V] on a 16-byte aligned base, 0 < V < 2^31; targets
// contiguous int64 with T elements on the logits' device (already shifted:
// targets[t] is the label of row t); lse and tok_loss contiguous fp32 with T
// elements on that device; in the backward, scale_dev one fp32 there.
static CeRowsShape check_ce_rows_args(const at::Tensor& logits,
                                      const at::Tensor& targets,
                                      const at::Tensor& lse,
                                      const at::Tensor* tok_loss,
                                      const at::Tensor* scale_dev) {
  CHECK_BF16_CONTIG(logits);
  TORCH_CHECK(logits.dim() == 2 && logits.size(1) > 0 &&
              logits.size(1) < (1LL << 31),
              "logits must be [T, V] with 0 < V < 2^31, got ", logits.sizes());
  TORCH_CHECK(aligned_to(logits, 16), "logits must be 16-byte aligned");
  const int64_t T = logits.size(0);
  TORCH_CHECK(targets.is_cuda() && targets.device() == logits.device() &&
              targets.scalar_type() == at::kLong && targets.is_contiguous() &&
              targets.numel() == T, "targets must be contiguous int64 with T"
              " = ", T, " elements on ", logits.device(), ", got ",
              targets.scalar_type(), " ", targets.sizes(), " on ",
              targets.device());
  check_f32_vec(lse, T, logits, "lse");
  if (tok_loss != nullptr) check_f32_vec(*tok_loss, T, logits, "tok_loss");
  if (scale_dev != nullptr) check_dev_scalar(*scale_dev, logits, "scale_dev");
  return {(long long)T, (int)logits.size(1)};
}

// lse[t], tok_loss[t] of every row (0 on ignored rows), stored into the
// caller's buffers
void ce_rows_fwd(at::Tensor logits, at::Tensor targets, at::Tensor lse,
                 at::Tensor tok_loss, double epsilon) {
  const auto [T, V] = check_ce_rows_args(logits, targets, lse, &tok_loss,
                                         nullptr);
  if (T == 0) return;
  acco_ce_rows_fwd(logits.data_ptr(),
                   reinterpret_cast<const long long*>(
                       targets.data_ptr<int64_t>()),
                   lse.data_ptr<float>(), tok_loss.data_ptr<float>(), T, V,
                   (float)epsilon, cur_stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

// logits become scale_dev[0] · dloss/dlogits in place
void ce_rows_bwd_(at::Tensor logits, at::Tensor targets, at::Tensor lse,
                  at::Tensor scale_dev, double epsilon) {
  const auto [T, V] = check_ce_rows_args(logits, targets, lse, nullptr,
                                         &scale_dev);
  if (T == 0) return;
  acco_ce_rows_bwd(logits.data_ptr(),
                   reinterpret_cast<const long long*>(
                       targets.data_ptr<int64_t>()),
                   lse.data_ptr<float>(), scale_dev.data_ptr<float>(), T, V,
                   (float)epsilon, cur_stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

// ---- flash attention ([B, S, H, D] layout)
// window: what the kernels get, the caller's clamped to S (below)
struct AttnShape { int B, S, H, Hkv, D, window; };

// What every attention kernel needs of its sizes: D in {64, 128}, GQA groups
// of whole heads, whole tiles (s_mult = 64, or 256 where only the 32x32
// kernels are launched), window >= 0 and a 1-D grid that fits. A window >= S
// bounds nothing, so it reaches the kernels as S: their int arithmetic on
// row + window then stays below 2^31 (S < 2^30), and a 64-bit window is
// never truncated to a small one by the cast.
static AttnShape check_attn_dims(int64_t B, int64_t S, int64_t H, int64_t Hkv,
                                 int64_t D, int64_t window, int64_t s_mult) {
  TORCH_CHECK((D == 64 || D == 128) && H > 0 && Hkv > 0 && H % Hkv == 0,
              "need D in {64, 128} and H % Hkv == 0, got D=", D, " H=", H,
              " Hkv=", Hkv);
  TORCH_CHECK(S > 0 && S % s_mult == 0 && S < (1LL << 30) && window >= 0,
              "need S % ", s_mult, " == 0 and window >= 0, got S=", S,
              " window=", window);
  TORCH_CHECK(B > 0 && B * H <= 65535 && (S / 64) * B * H < (1LL << 31),
              "need 1 <= B*H <= 65535 and S/64 * B*H < 2^31 (the 1-D grid), "
              "got B=", B, " H=", H, " S=", S);
  return {(int)B, (int)S, (int)H, (int)Hkv, (int)D,
          (int)(window < S ? window : S)};
}

// every tensor of `same` is contiguous bf16 on ref's device with ref's sizes
static void check_attn_like(const at::Tensor& ref, const char* what,
                            std::initializer_list<at::Tensor> same) {
  for (const at::Tensor& t : same) {
    CHECK_BF16_CONTIG(t);
    TORCH_CHECK(t.device() == ref.device() && t.sizes() == ref.sizes(), what,
                ": expected ", ref.sizes(), " on ", ref.device(), ", got ",
                t.sizes(), " on ", t.device());
  }
}

// lse / delta: contiguous fp32 with one element per (b, h, s)
static void check_attn_stats(const at::Tensor& ref, const AttnShape& a,
                             std::initializer_list<at::Tensor> stats) {
  const int64_t n = (int64_t)a.B * a.H * a.S;
  for (const at::Tensor& st : stats)
    TORCH_CHECK(st.is_cuda() && st.device() == ref.device() &&
                st.scalar_type() == at::kFloat && st.is_contiguous() &&
                st.numel() == n, "lse/delta must be contiguous CUDA fp32 with "
                "B*H*S = ", n, " elements, got ", st.numel(), " of ",
                st.scalar_type());
}

// doc_start / doc_end (document bounds of packed rows): contiguous int32
// [B, S] on ref's device. The kernels that take them are the 32x32
// generation only, so S % 256 == 0 is required with them, and a positive
// scale (the forward kernel masks raw scores with -inf before scaling).
static const int* check_attn_doc(const at::Tensor& ref, const AttnShape& a,
                                 const c10::optional<at::Tensor>& doc,
                                 const char* name, double scale) {
  if (!doc.has_value()) return nullptr;
  const at::Tensor& t = *doc;
  TORCH_CHECK(t.is_cuda() && t.device() == ref.device() &&
              t.scalar_type() == at::kInt && t.is_contiguous() &&
              t.dim() == 2 && t.size(0) == a.B && t.size(1) == a.S, name,
              " must be contiguous int32 [B, S] = [", a.B, ", ", a.S,
              "] on ", ref.device(), ", got ", t.scalar_type(), " ",
              t.sizes(), " on ", t.device());
  TORCH_CHECK(a.S % 256 == 0, name, " needs S % 256 == 0 (the 32x32 "
              "kernels), got S=", a.S);
  TORCH_CHECK(scale > 0 && scale < 1e30, name, " needs a positive finite "
              "scale, got ", scale);
  return t.data_ptr<int>();
}

// The argument contract of the unpacked entry points: q [B,S,H,D] and
// k, v [B,S,Hkv,D] contiguous bf16 on q's device; each of `like_q` (dO) of
// q's shape; `stats` (lse, delta) as above.
static AttnShape check_attn_args(
    const at::Tensor& q, const at::Tensor& k, const at::Tensor& v,
    int64_t window, std::initializer_list<at::Tensor> like_q = {},
    std::initializer_list<at::Tensor> stats = {}) {
  CHECK_BF16_CONTIG(q); CHECK_BF16_CONTIG(k);
  TORCH_CHECK(q.dim() == 4 && k.dim() == 4 && k.device() == q.device() &&
              k.size(0) == q.size(0) && k.size(1) == q.size(1) &&
              k.size(3) == q.size(3),
              "need q [B,S,H,D] and k [B,S,Hkv,D] on one device, got ",
              q.sizes(), " on ", q.device(), " and ", k.sizes(), " on ",
              k.device());
  const AttnShape a = check_attn_dims(q.size(0), q.size(1), q.size(2),
                                      k.size(2), q.size(3), window, 64);
  check_attn_like(k, "v against k", {v});
  check_attn_like(q, "dO against q", like_q);
  check_attn_stats(q, a, stats);
  return a;
}

std::vector<at::Tensor> attn_fwd(at::Tensor q, at::Tensor k, at::Tensor v,
                                 double scale, int64_t window,
                                 c10::optional<at::Tensor> doc_start) {
  const AttnShape a = check_attn_args(q, k, v, window);
  const auto [B, S, H, Hkv, D, win] = a;
  const int* ds = check_attn_doc(q, a, doc_start, "doc_start", scale);
  auto o = at::empty_like(q);
  auto lse = at::empty({B, H, S}, q.options().dtype(at::kFloat));
  if (ds != nullptr) {
    acco_attn_fwd32(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(),
                    lse.data_ptr<float>(), B, S, H, Hkv, D, (float)scale,
                    win, (long long)H * D, (long long)Hkv * D,
                    (long long)H * D, ds, cur_stream());
  } else {
    acco_attn_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(),
                  lse.data_ptr<float>(), B, S, H, Hkv, D, (float)scale,
                  win, cur_stream());
  }
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {o, lse};
}

at::Tensor attn_delta(at::Tensor dO, at::Tensor o) {
  CHECK_BF16_CONTIG(dO);
  TORCH_CHECK(dO.dim() == 4 && dO.size(3) % 8 == 0 && dO.size(1) < (1LL << 31),
              "dO must be [B,S,H,D] with D % 8 == 0, got ", dO.sizes());
  check_attn_like(dO, "o against dO", {o});
  const long long B = dO.size(0);
  const int S = (int)dO.size(1), H = (int)dO.size(2), D = (int)dO.size(3);
  auto delta = at::empty({B, H, S}, dO.options().dtype(at::kFloat));
  acco_attn_delta(dO.data_ptr(), o.data_ptr(), delta.data_ptr<float>(), B, S,
                  H, D, cur_stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return delta;
}

std::vector<at::Tensor> attn_bwd(at::Tensor q, at::Tensor k, at::Tensor v,
                                 at::Tensor dO, at::Tensor lse,
                                 at::Tensor delta, double scale,
                                 int64_t window,
                                 c10::optional<at::Tensor> doc_start,
                                 c10::optional<at::Tensor> doc_end) {
  const AttnShape a = check_attn_args(q, k, v, window, {dO}, {lse, delta});
  const auto [B, S, H, Hkv, D, win] = a;
  TORCH_CHECK(doc_start.has_value() == doc_end.has_value(),
              "doc_start and doc_end must both be given or both be None");
  const int* ds = check_attn_doc(q, a, doc_start, "doc_start", scale);
  const int* de = check_attn_doc(q, a, doc_end, "doc_end", scale);
  auto dq = at::empty_like(q);
  // dk/dv are emitted per QUERY head; the Python wrapper group-reduces
  auto dk = at::empty_like(q);
  auto dv = at::empty_like(q);
  if (ds != nullptr) {
    const long long qr = (long long)H * D, kr = (long long)Hkv * D;
    acco_attn_bwd32_dq(q.data_ptr(), k.data_ptr(), v.data_ptr(),
                       dO.data_ptr(), lse.data_ptr<float>(),
                       delta.data_ptr<float>(), dq.data_ptr(), B, S, H, Hkv,
                       D, (float)scale, win, qr, kr, qr, qr, nullptr,
                       nullptr, ds, cur_stream());
    C10_HIP_KERNEL_LAUNCH_CHECK();
    acco_attn_bwd32_dkv(q.data_ptr(), k.data_ptr(), v.data_ptr(),
                        dO.data_ptr(), lse.data_ptr<float>(),
                        delta.data_ptr<float>(), dk.data_ptr(), dv.data_ptr(),
                        B, S, H, Hkv, D, (float)scale, win, qr, kr,
                        qr, de, cur_stream());
    C10_HIP_KERNEL_LAUNCH_CHECK();
    return {dq, dk, dv};
  }
  acco_attn_bwd_dq(q.data_ptr(), k.data_ptr(), v.data_ptr(), dO.data_ptr(),
                   lse.data_ptr<float>(), delta.data_ptr<float>(),
                   dq.data_ptr(), B, S, H, Hkv, D, (float)scale, win,
                   cur_stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  acco_attn_bwd_dkv(q.data_ptr(), k.data_ptr(), v.data_ptr(), dO.data_ptr(),
                    lse.data_ptr<float>(), delta.data_ptr<float>(),
                    dk.data_ptr(), dv.data_ptr(), B, S, H, Hkv, D,
                    (float)scale, win, cur_stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {dq, dk, dv};
}

// The kernels' block order on the host: row i of the int32 [n_blk*B*H, 2]
// result is the (row block, b*H + h) that linear block id i works on;
// heavy_last = true is the forward / dq order, false the dkv order.
at::Tensor attn_block_order(int64_t n_blk, int64_t B, int64_t H,
                            bool heavy_last) {
  TORCH_CHECK(B > 0 && H > 0 && B * H <= 65535 && n_blk > 0 &&
              n_blk < (1LL << 31) && n_blk * B * H < (1LL << 31),
              "need 1 <= B*H <= 65535 and 1 <= n_blk*B*H < 2^31, got n_blk=",
              n_blk, " B=", B, " H=", H);
  auto out = at::empty({n_blk * B * H, 2}, at::TensorOptions().dtype(at::kInt));
  acco_attn_block_order(out.data_ptr<int>(), (int)n_blk, (int)B, (int)H,
                        heavy_last);
  return out;
}

// ---- packed-QKV layout: qkv [B, S, W] contiguous bf16, each section
// (q: H*D wide, k and v: Hkv*D wide) at a caller-given column offset, so
// both packing orders work (Llama q|k|v, GPT-Neo k|v|q).
struct PackedSection { const char* name; int64_t off, width; };

// qkv is 3-D contiguous bf16; W and every offset are multiples of 8 (the
// kernels read 16-byte vectors from base + off); every section lies inside
// W and no two overlap.
static void check_packed_layout(const at::Tensor& qkv,
                                std::initializer_list<PackedSection> secs) {
  CHECK_BF16_CONTIG(qkv);
  TORCH_CHECK(qkv.dim() == 3 && qkv.size(2) % 8 == 0,
              "packed qkv must be [B,S,W] with W % 8 == 0, got ", qkv.sizes());
  const int64_t W = qkv.size(2);
  for (const PackedSection& s : secs) {
    TORCH_CHECK(s.off >= 0 && s.off % 8 == 0 && s.width > 0 &&
                s.off + s.width <= W, s.name, " section [", s.off, ", ",
                s.off + s.width, ") must start at a multiple of 8 inside W=",
                W);
    for (const PackedSection& t : secs)
      TORCH_CHECK(&s == &t || s.off + s.width <= t.off ||
                  t.off + t.width <= s.off, s.name, " section [", s.off, ", ",
                  s.off + s.width, ") overlaps ", t.name, " section [", t.off,
                  ", ", t.off + t.width, ")");
  }
}

// GQA group-reduce of per-query-head dK/dV [B, S, Hkv*rep, D] straight into
// the k|v sections of the packed grad; cos/sin given: the inverse RoPE of
// the k grad is folded in (rep >= 1)
static void gqa_reduce_impl(const at::Tensor& dkq, const at::Tensor& dvq,
                            const at::Tensor& dqkv, const at::Tensor* cos_t,
                            const at::Tensor* sin_t, int64_t Hkv, int64_t rep,
                            int64_t D, int64_t k_off, int64_t v_off) {
  CHECK_BF16_CONTIG(dkq);
  TORCH_CHECK(Hkv > 0 && rep > 0 && D > 0 && D % (cos_t ? 16 : 8) == 0 &&
              dkq.dim() == 4 && dkq.size(2) == Hkv * rep && dkq.size(3) == D,
              "dkq/dvq must be [B, S, Hkv*rep, D] with D % ", cos_t ? 16 : 8,
              " == 0, got ", dkq.sizes(), " for Hkv=", Hkv, " rep=", rep,
              " D=", D);
  check_attn_like(dkq, "dvq against dkq", {dvq});
  check_packed_layout(dqkv, {{"k", k_off, Hkv * D}, {"v", v_off, Hkv * D}});
  TORCH_CHECK(dqkv.device() == dkq.device() && dqkv.size(0) == dkq.size(0) &&
              dqkv.size(1) == dkq.size(1), "dqkv must be [B,S,W] on dkq's "
              "device; dkq is ", dkq.sizes(), ", dqkv is ", dqkv.sizes());
  const long long T = dkq.size(0) * dkq.size(1);
  const int S = (int)dkq.size(1);
  const long long W = dqkv.size(2);
  if (cos_t) {
    check_rope_table(*cos_t, *sin_t, S, D, dqkv);
    TORCH_CHECK(T * Hkv * (D / 16) < (1LL << 31));
    acco_attn_gqa_reduce_rope(dkq.data_ptr(), dvq.data_ptr(), dqkv.data_ptr(),
                              cos_t->data_ptr<float>(),
                              sin_t->data_ptr<float>(), T, S, (int)Hkv,
                              (int)rep, (int)D, W, k_off, v_off, cur_stream());
  } else {
    acco_attn_gqa_reduce(dkq.data_ptr(), dvq.data_ptr(), dqkv.data_ptr(), T,
                         (int)Hkv, (int)rep, (int)D, W, k_off, v_off,
                         cur_stream());
  }
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

void attn_gqa_reduce(at::Tensor dkq, at::Tensor dvq, at::Tensor dqkv,
                     int64_t Hkv, int64_t rep, int64_t D, int64_t k_off,
                     int64_t v_off) {
  gqa_reduce_impl(dkq, dvq, dqkv, nullptr, nullptr, Hkv, rep, D, k_off, v_off);
}

void attn_gqa_reduce_rope(at::Tensor dkq, at::Tensor dvq, at::Tensor dqkv,
                          at::Tensor cos_t, at::Tensor sin_t, int64_t Hkv,
                          int64_t rep, int64_t D, int64_t k_off,
                          int64_t v_off) {
  gqa_reduce_impl(dkq, dvq, dqkv, &cos_t, &sin_t, Hkv, rep, D, k_off, v_off);
}

// ---- experimental NT GEMM (C = A · B^T, bf16; bench/refcheck only)
at::Tensor gemm_nt(at::Tensor A, at::Tensor B) {
  CHECK_BF16_CONTIG(A); CHECK_BF16_CONTIG(B);
  TORCH_CHECK(A.dim() == 2 && B.dim() == 2 && B.device() == A.device(),
              "need A [M,K] and B [N,K] on one device, got ", A.sizes(),
              " on ", A.device(), " and ", B.sizes(), " on ", B.device());
  const int M = (int)A.size(0), K = (int)A.size(1), N = (int)B.size(0);
  TORCH_CHECK(B.size(1) == K && M % 128 == 0 && N % 128 == 0 && K % 64 == 0,
              "need M % 128 == 0, N % 128 == 0, K % 64 == 0 and one K, got ",
              A.sizes(), " and ", B.sizes());
  if (M == 0 || N == 0 || K == 0) return at::zeros({M, N}, A.options());
  auto C = at::empty({M, N}, A.options());
  acco_gemm_nt(A.data_ptr(), B.data_ptr(), C.data_ptr(), M, N, K,
               cur_stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return C;
}

// ---- packed-QKV attention path (fused projection output consumed and
// grad produced with ZERO split/cat copies). qkv: [B, S, W] contiguous with
// W >= (H + 2*Hkv)*D, sections at the given offsets (check_packed_layout);
// D in {64, 128}, S%256==0 (v4 kernels only).

// RoPE of one section (Hsec heads of width D at column `off`) of src [B,S,W]
// into the same section of dst; off a multiple of 4 (8-byte vectors).
std::vector<at::Tensor> rope_packed(at::Tensor src, at::Tensor dst,
                                    at::Tensor cos_t, at::Tensor sin_t,
                                    int64_t off, int64_t Hsec, int64_t D,
                                    bool bwd) {
  CHECK_BF16_CONTIG(src); CHECK_BF16_CONTIG(dst);
  TORCH_CHECK(src.dim() == 3 && src.size(1) < (1LL << 31),
              "src must be [B,S,W], got ", src.sizes());
  TORCH_CHECK(dst.device() == src.device() && dst.sizes() == src.sizes(),
              "dst: expected ", src.sizes(), " on ", src.device(), ", got ",
              dst.sizes(), " on ", dst.device());
  const long long B = src.size(0);
  const int S = (int)src.size(1);
  const long long W = src.size(2);
  TORCH_CHECK(D > 0 && D % 8 == 0 && Hsec > 0 && Hsec < (1LL << 31) / D,
              "need D % 8 == 0 and Hsec > 0, got D=", D, " Hsec=", Hsec);
  TORCH_CHECK(off >= 0 && off % 4 == 0 && off + Hsec * D <= W, "section [",
              off, ", ", off + Hsec * D, ") must start at a multiple of 4 "
              "inside W=", W);
  check_rope_table(cos_t, sin_t, S, D, src);
  if (src.numel() == 0) return {dst};
  acco_rope((const u16*)src.data_ptr() + off,
            (u16*)dst.data_ptr() + off, cos_t.data_ptr<float>(),
            sin_t.data_ptr<float>(), B, S, (int)Hsec, (int)D, bwd, W,
            cur_stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {dst};
}

// forward rotation of the q and k sections of the packed projection output
// IN PLACE, one launch; the V section is left untouched
void rope_qk_inplace(at::Tensor qkv, at::Tensor cos_t, at::Tensor sin_t,
                     int64_t H, int64_t Hkv, int64_t D, int64_t q_off,
                     int64_t k_off) {
  check_packed_layout(qkv, {{"q", q_off, H * D}, {"k", k_off, Hkv * D}});
  TORCH_CHECK(D % 16 == 0, "in-place RoPE needs D % 16 == 0, got ", D);
  const long long T = qkv.size(0) * qkv.size(1);
  const int S = (int)qkv.size(1);
  const long long W = qkv.size(2);
  check_rope_table(cos_t, sin_t, S, D, qkv);
  TORCH_CHECK(T * (H + Hkv) * (D / 16) < (1LL << 31));
  acco_rope_qk_inplace(qkv.data_ptr(), cos_t.data_ptr<float>(),
                       sin_t.data_ptr<float>(), T, S, (int)H, (int)Hkv,
                       (int)D, W, q_off, k_off, cur_stream());
}

// The argument contract of the packed entry points: the layout above with
// all three sections, the sizes the 32x32 kernels take (S % 256 == 0), and
// each of `like_qkv` (dqkv) of qkv's shape on qkv's device.
static AttnShape check_attn_packed_args(
    const at::Tensor& qkv, int64_t H, int64_t Hkv, int64_t D, int64_t window,
    int64_t q_off, int64_t k_off, int64_t v_off,
    std::initializer_list<at::Tensor> like_qkv = {}) {
  check_packed_layout(qkv, {{"q", q_off, H * D}, {"k", k_off, Hkv * D},
                            {"v", v_off, Hkv * D}});
  const AttnShape a =
      check_attn_dims(qkv.size(0), qkv.size(1), H, Hkv, D, window, 256);
  check_attn_like(qkv, "dqkv against qkv", like_qkv);
  return a;
}

std::vector<at::Tensor> attn_fwd_packed(at::Tensor qkv, int64_t H,
                                        int64_t Hkv, int64_t D, double scale,
                                        int64_t window, int64_t q_off,
                                        int64_t k_off, int64_t v_off,
                                        c10::optional<at::Tensor> doc_start) {
  const AttnShape a =
      check_attn_packed_args(qkv, H, Hkv, D, window, q_off, k_off, v_off);
  const int* ds = check_attn_doc(qkv, a, doc_start, "doc_start", scale);
  const long long W = qkv.size(2);
  const u16* base = (const u16*)qkv.data_ptr();
  auto o = at::empty({a.B, a.S, H * D}, qkv.options());
  auto lse = at::empty({a.B, a.H, a.S}, qkv.options().dtype(at::kFloat));
  acco_attn_fwd32(base + q_off, base + k_off, base + v_off, o.data_ptr(),
                  lse.data_ptr<float>(), a.B, a.S, a.H, a.Hkv, a.D,
                  (float)scale, a.window, W, W, H * D, ds, cur_stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {o, lse};
}

std::vector<at::Tensor> attn_bwd_packed(at::Tensor qkv, at::Tensor dO,
                                        at::Tensor lse, at::Tensor delta,
                                        at::Tensor dqkv, int64_t H,
                                        int64_t Hkv, int64_t D, double scale,
                                        int64_t window, int64_t q_off,
                                        int64_t k_off, int64_t v_off,
                                        c10::optional<at::Tensor> cos_opt,
                                        c10::optional<at::Tensor> sin_opt,
                                        c10::optional<at::Tensor> doc_start,
                                        c10::optional<at::Tensor> doc_end) {
  const AttnShape a = check_attn_packed_args(qkv, H, Hkv, D, window, q_off,
                                             k_off, v_off, {dqkv});
  TORCH_CHECK(doc_start.has_value() == doc_end.has_value(),
              "doc_start and doc_end must both be given or both be None");
  const int* ds = check_attn_doc(qkv, a, doc_start, "doc_start", scale);
  const int* de = check_attn_doc(qkv, a, doc_end, "doc_end", scale);
  const int B = a.B, S = a.S;
  const long long W = qkv.size(2);
  CHECK_BF16_CONTIG(dO);
  TORCH_CHECK(dO.device() == qkv.device() && dO.dim() == 3 &&
              dO.size(0) == B && dO.size(1) == S && dO.size(2) == H * D,
              "dO must be [B,S,H*D] = [", B, ", ", S, ", ", H * D,
              "] on qkv's device, got ", dO.sizes());
  check_attn_stats(qkv, a, {lse, delta});
  // cos/sin given: the dq kernel applies the inverse RoPE in its epilogue
  TORCH_CHECK(cos_opt.has_value() == sin_opt.has_value(),
              "cos and sin must both be given or both be None");
  const float* rc = nullptr;
  const float* rs = nullptr;
  if (cos_opt.has_value()) {
    check_rope_table(*cos_opt, *sin_opt, S, D, qkv);
    rc = cos_opt->data_ptr<float>();
    rs = sin_opt->data_ptr<float>();
  }
  const u16* base = (const u16*)qkv.data_ptr();
  u16* dbase = (u16*)dqkv.data_ptr();
  // dq straight into the packed grad (stride W); dk/dv per-QUERY-head temps
  auto dkq = at::empty({B, S, H, D}, qkv.options());
  auto dvq = at::empty({B, S, H, D}, qkv.options());
  acco_attn_bwd32_dq(base + q_off, base + k_off, base + v_off, dO.data_ptr(),
                     lse.data_ptr<float>(), delta.data_ptr<float>(),
                     dbase + q_off, B, S, (int)H, (int)Hkv, (int)D,
                     (float)scale, a.window, W, W, H * D, W, rc, rs, ds,
                     cur_stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  acco_attn_bwd32_dkv(base + q_off, base + k_off, base + v_off,
                      dO.data_ptr(), lse.data_ptr<float>(),
                      delta.data_ptr<float>(), dkq.data_ptr(),
                      dvq.data_ptr(), B, S, (int)H, (int)Hkv, (int)D,
                      (float)scale, a.window, W, W, H * D, de,
                      cur_stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {dkq, dvq};
}

// ---- KV cache: append and single-token attention
struct CacheShape { int B, Hkv, Smax, D; };

// The argument contract of both cache entry points: k_cache and v_cache
// contiguous CUDA bf16 [B, Hkv, Smax, D] on one device, 16-byte aligned,
// D in {64, 128}; cache_len contiguous int32 [B] on that device (data: the
// kernels clamp it into [0, Smax]).
static CacheShape check_cache_args(const at::Tensor& k_cache,
                                   const at::Tensor& v_cache,
                                   const at::Tensor& cache_len) {
  CHECK_BF16_CONTIG(k_cache); CHECK_BF16_CONTIG(v_cache);
  TORCH_CHECK(k_cache.dim() == 4 && v_cache.sizes() == k_cache.sizes() &&
              v_cache.device() == k_cache.device(),
              "k_cache and v_cache must be [B, Hkv, Smax, D] of one shape on "
              "one device, got ", k_cache.sizes(), " on ", k_cache.device(),
              " and ", v_cache.sizes(), " on ", v_cache.device());
  const int64_t B = k_cache.size(0), Hkv = k_cache.size(1);
  const int64_t Smax = k_cache.size(2), D = k_cache.size(3);
  TORCH_CHECK((D == 64 || D == 128) && D % 16 == 0,
              "k_cache: need D in {64, 128}, got D=", D);
  TORCH_CHECK(B > 0 && Hkv > 0 && Smax > 0 && Smax < (1LL << 30) &&
              B * Hkv <= 65535, "k_cache: need 1 <= B*Hkv <= 65535 and "
              "1 <= Smax < 2^30, got ", k_cache.sizes());
  TORCH_CHECK(aligned_to(k_cache, 16) && aligned_to(v_cache, 16),
              "k_cache and v_cache must be 16-byte aligned");
  TORCH_CHECK(cache_len.is_cuda() && cache_len.device() == k_cache.device() &&
              cache_len.scalar_type() == at::kInt &&
              cache_len.is_contiguous() && cache_len.dim() == 1 &&
              cache_len.size(0) == B, "cache_len must be contiguous int32 [B]"
              " = [", B, "] on ", k_cache.device(), ", got ",
              cache_len.scalar_type(), " ", cache_len.sizes(), " on ",
              cache_len.device());
  return {(int)B, (int)Hkv, (int)Smax, (int)D};
}

// t [B, T, heads, D] bf16 on ref's device whose heads are contiguous inside a
// token row and whose rows lie one row stride apart (a section of the packed
// projection output, or a contiguous tensor); returns the row stride
static long long check_token_rows(const at::Tensor& t, const at::Tensor& ref,
                                  int64_t B, int64_t T, int64_t heads,
                                  int64_t D, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.device() == ref.device() &&
              t.scalar_type() == at::kBFloat16, name, " must be CUDA bf16 on ",
              ref.device(), ", got ", t.scalar_type(), " on ", t.device());
  TORCH_CHECK(t.dim() == 4 && t.size(0) == B && t.size(1) == T &&
              t.size(2) == heads && t.size(3) == D, name, " must be [", B,
              ", ", T, ", ", heads, ", ", D, "], got ", t.sizes());
  const int64_t rs = T > 1 ? t.stride(1) : (B > 1 ? t.stride(0) : heads * D);
  TORCH_CHECK(t.stride(3) == 1 && t.stride(2) == D && rs >= heads * D &&
              rs % 8 == 0 && (B == 1 || t.stride(0) == T * rs) &&
              (T == 1 || t.stride(1) == rs), name, " must have contiguous "
              "heads and evenly strided token rows (row stride a multiple of "
              "8), got strides ", t.strides());
  TORCH_CHECK(aligned_to(t, 16), name, " must be 16-byte aligned");
  return rs;
}

// Writes k / v of T new tokens per sequence into the caches at row
// cache_len[b] + t (rows >= Smax dropped); with cos / sin, K is rotated by
// its absolute position and the rotated q [B, T, H, D] is returned.
c10::optional<at::Tensor> kv_append(c10::optional<at::Tensor> q, at::Tensor k,
                                    at::Tensor v,
                                    c10::optional<at::Tensor> cos_t,
                                    c10::optional<at::Tensor> sin_t,
                                    at::Tensor k_cache, at::Tensor v_cache,
                                    at::Tensor cache_len) {
  const auto [B, Hkv, Smax, D] = check_cache_args(k_cache, v_cache, cache_len);
  TORCH_CHECK(k.dim() == 4, "k must be [B, T, Hkv, D], got ", k.sizes());
  const int64_t T = k.size(1);
  TORCH_CHECK(T >= 0 && T < (1LL << 30), "k: T out of range: ", T);
  const long long k_rs = check_token_rows(k, k_cache, B, T, Hkv, D, "k");
  const long long v_rs = check_token_rows(v, k_cache, B, T, Hkv, D, "v");
  TORCH_CHECK(cos_t.has_value() == sin_t.has_value(),
              "cos and sin must both be given or both be None");
  TORCH_CHECK(cos_t.has_value() == q.has_value(),
              "q is rotated with the tables: give q, cos and sin, or none");
  if (!cos_t.has_value()) {
    TORCH_CHECK((long long)B * T * 2 * Hkv * (D / 16) < (1LL << 31),
                "k: too many elements for one launch");
    if (T == 0) return c10::nullopt;
    acco_kv_append(nullptr, k.data_ptr(), v.data_ptr(), nullptr,
                   k_cache.data_ptr(), v_cache.data_ptr(),
                   cache_len.data_ptr<int>(), nullptr, nullptr, B, (int)T, 0,
                   Hkv, D, Smax, 0, 0, k_rs, v_rs, cur_stream());
    C10_HIP_KERNEL_LAUNCH_CHECK();
    return c10::nullopt;
  }
  TORCH_CHECK(q->dim() == 4 && q->size(2) > 0 && q->size(2) % Hkv == 0,
              "q must be [B, T, H, D] with H % Hkv == 0, got ", q->sizes());
  const int64_t H = q->size(2);
  const long long q_rs = check_token_rows(*q, k_cache, B, T, H, D, "q");
  check_rope_table(*cos_t, *sin_t, Smax, D, k_cache);
  TORCH_CHECK(cos_t->size(0) < (1LL << 31), "cos: too many rows");
  TORCH_CHECK((long long)B * T * (H + 2 * Hkv) * (D / 16) < (1LL << 31),
              "q: too many elements for one launch");
  auto q_out = at::empty({B, T, H, D}, k_cache.options());
  if (T == 0) return q_out;
  acco_kv_append(q->data_ptr(), k.data_ptr(), v.data_ptr(), q_out.data_ptr(),
                 k_cache.data_ptr(), v_cache.data_ptr(),
                 cache_len.data_ptr<int>(), cos_t->data_ptr<float>(),
                 sin_t->data_ptr<float>(), B, (int)T, (int)H, Hkv, D, Smax,
                 (int)cos_t->size(0), q_rs, k_rs, v_rs, cur_stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return q_out;
}

// (n_split, chunk) of attn_decode for B*Hkv (sequence, kv head) pairs and a
// cache of Smax rows: split i owns keys [i*chunk, (i+1)*chunk)
std::vector<int64_t> attn_decode_grid(int64_t BHkv, int64_t Smax) {
  TORCH_CHECK(BHkv > 0 && Smax > 0 && Smax < (1LL << 30),
              "need BHkv > 0 and 0 < Smax < 2^30, got BHkv=", BHkv, " Smax=",
              Smax);
  int n_split, chunk;
  acco_attn_decode_grid((long long)BHkv, (int)Smax, &n_split, &chunk);
  return {n_split, chunk};
}

// o [B, H, D] of one query token per sequence: q [B, H, D] bf16 whose rows
// may be strided (a section of the packed projection output). A window at or
// beyond Smax bounds nothing and reaches the kernel as 0 (none).
at::Tensor attn_decode(at::Tensor q, at::Tensor k_cache, at::Tensor v_cache,
                       at::Tensor cache_len, double scale, int64_t window) {
  const auto [B, Hkv, Smax, D] = check_cache_args(k_cache, v_cache, cache_len);
  TORCH_CHECK(q.dim() == 3, "q must be [B, H, D], got ", q.sizes());
  const int64_t H = q.size(1);
  TORCH_CHECK(H > 0 && H % Hkv == 0 && H / Hkv <= 8,
              "q: need H % Hkv == 0 and 1 <= H/Hkv <= 8, got H=", H, " Hkv=",
              Hkv);
  const long long q_rs =
      check_token_rows(q.unsqueeze(1), k_cache, B, 1, H, D, "q");
  TORCH_CHECK(window >= 0, "window must be >= 0, got ", window);
  const int win = window >= Smax ? 0 : (int)window;
  int n_split, chunk;
  acco_attn_decode_grid((long long)B * Hkv, Smax, &n_split, &chunk);
  auto o = at::empty({B, H, D}, k_cache.options());
  auto ws = at::empty({(int64_t)B * H * n_split * (2 + D)},
                      k_cache.options().dtype(at::kFloat));
  acco_attn_decode(q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(),
                   cache_len.data_ptr<int>(), o.data_ptr(),
                   ws.data_ptr<float>(), B, (int)H, Hkv, D, Smax,
                   (float)scale, win, q_rs, cur_stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return o;
}

// ---- on-device sampling (sample.hip)
// (token int64 [B], logprob fp32 [B], thr bf16 [B], n_kept int32 [B]) of one
// draw per row. The argument contract: logits CUDA bf16 [B, V] whose last dim
// is contiguous and whose rows lie stride(0) >= V elements apart (no
// alignment asked: the kernel splits each row by its own address),
// 1 <= V < 2^31, B < 2^31; temperature finite and >= 0 (0 = greedy);
// top_k >= 0 (0 = off); top_p > 0 (>= 1 = off); done, when given, contiguous
// uint8 [B] on the logits' device, updated in place, and then
// 0 <= eos_id < V (a finished row's token is eos_id, and every token must
// index the embedding).
std::vector<at::Tensor> sample_logits(at::Tensor logits, double temperature,
                                      int64_t top_k, double top_p,
                                      uint64_t seed, uint64_t step,
                                      c10::optional<at::Tensor> done,
                                      int64_t eos_id) {
  TORCH_CHECK(logits.is_cuda() && logits.scalar_type() == at::kBFloat16,
              "logits must be CUDA bf16, got ", logits.scalar_type(), " on ",
              logits.device());
  TORCH_CHECK(logits.dim() == 2 && logits.size(1) >= 1 &&
              logits.size(1) < (1LL << 31) && logits.size(0) < (1LL << 31),
              "logits must be [B, V] with 1 <= V < 2^31 and B < 2^31, got ",
              logits.sizes());
  const int64_t B = logits.size(0), V = logits.size(1);
  TORCH_CHECK(V == 1 || logits.stride(1) == 1,
              "logits: the last dim must be contiguous, got strides ",
              logits.strides());
  const int64_t rs = B > 1 ? logits.stride(0) : V;
  TORCH_CHECK(rs >= V, "logits: rows must not overlap (row stride >= V = ", V,
              "), got strides ", logits.strides());
  TORCH_CHECK(temperature >= 0.0 && temperature < 1e30,
              "temperature must be finite and >= 0, got ", temperature);
  TORCH_CHECK(temperature == 0.0 || (float)temperature > 0.0f,
              "temperature underflows fp32: ", temperature);
  TORCH_CHECK(top_k >= 0, "top_k must be >= 0 (0 = off), got ", top_k);
  TORCH_CHECK(top_p > 0.0, "top_p must be > 0 (>= 1 = off), got ", top_p);
  unsigned char* done_ptr = nullptr;
  if (done.has_value()) {
    TORCH_CHECK(done->is_cuda() && done->device() == logits.device() &&
                done->scalar_type() == at::kByte && done->is_contiguous() &&
                done->dim() == 1 && done->size(0) == B,
                "done must be contiguous uint8 [B] = [", B, "] on ",
                logits.device(), ", got ", done->scalar_type(), " ",
                done->sizes(), " on ", done->device());
    TORCH_CHECK(eos_id >= 0 && eos_id < V, "with done, eos_id must be in "
                "[0, V = ", V, "), got ", eos_id);
    done_ptr = done->data_ptr<unsigned char>();
  }
  auto opts = logits.options();
  auto token = at::empty({B}, opts.dtype(at::kLong));
  auto logprob = at::empty({B}, opts.dtype(at::kFloat));
  auto thr = at::empty({B}, opts);
  auto n_kept = at::empty({B}, opts.dtype(at::kInt));
  if (B == 0) return {token, logprob, thr, n_kept};
  acco_sample_logits(logits.data_ptr(), rs, (int)B, (int)V,
                     (float)temperature, (int)(top_k < V ? top_k : V), top_p,
                     seed, step, done_ptr, eos_id,
                     reinterpret_cast<long long*>(token.data_ptr<int64_t>()),
                     logprob.data_ptr<float>(), thr.data_ptr(),
                     n_kept.data_ptr<int>(), cur_stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {token, logprob, thr, n_kept};
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("sample_logits", &sample_logits, py::arg("logits"),
        py::arg("temperature"), py::arg("top_k"), py::arg("top_p"),
        py::arg("seed"), py::arg("step"), py::arg("done"),
        py::arg("eos_id"));
  m.def("kv_append", &kv_append, py::arg("q"), py::arg("k"), py::arg("v"),
        py::arg("cos"), py::arg("sin"), py::arg("k_cache"),
        py::arg("v_cache"), py::arg("cache_len"));
  m.def("attn_decode_grid", &attn_decode_grid, py::arg("BHkv"),
        py::arg("Smax"));
  m.def("attn_decode", &attn_decode, py::arg("q"), py::arg("k_cache"),
        py::arg("v_cache"), py::arg("cache_len"), py::arg("scale"),
        py::arg("window"));
  m.def("fused_adamw", &fused_adamw,
        "Fused sharded AdamW (gfx950): cast+scale+AdamW+bf16 writeout; "
        "commit=false = ACCO tentative step");
  m.def("grad_sumsq", &grad_sumsq, py::arg("g"), py::arg("partials"));
  m.def("grad_sumsq_grid", &grad_sumsq_grid, py::arg("n"),
        py::arg("is_bf16"));
  m.def("sumsq_finalize", &sumsq_finalize, py::arg("partials"),
        py::arg("out"));
  m.def("swiglu_fwd", &swiglu_fwd);
  m.def("swiglu_bwd", &swiglu_bwd);
  m.def("swiglu_packed_fwd", &swiglu_packed_fwd);
  m.def("swiglu_packed_bwd", &swiglu_packed_bwd);
  m.def("gelu_fwd", &gelu_fwd);
  m.def("gelu_bwd", &gelu_bwd);
  m.def("colsum", &colsum);
  m.def("rmsnorm_fwd", &rmsnorm_fwd);
  m.def("rmsnorm_bwd", &rmsnorm_bwd, py::arg("dy"), py::arg("x"),
        py::arg("w"), py::arg("rstd"), py::arg("dadd") = py::none());
  m.def("add_rmsnorm_fwd", &add_rmsnorm_fwd);
  m.def("layernorm_fwd", &layernorm_fwd);
  m.def("layernorm_bwd", &layernorm_bwd, py::arg("dy"), py::arg("x"),
        py::arg("w"), py::arg("mean"), py::arg("rstd"),
        py::arg("dadd") = py::none());
  m.def("add_layernorm_fwd", &add_layernorm_fwd);
  m.def("rope_fwd", &rope_fwd);
  m.def("ce_fwd", &ce_fwd, py::arg("logits"), py::arg("labels"),
        py::arg("epsilon") = 0.0);
  m.def("ce_bwd", &ce_bwd, py::arg("logits"), py::arg("labels"),
        py::arg("lse"), py::arg("acc"), py::arg("dloss"),
        py::arg("epsilon") = 0.0);
  m.def("ce_bwd_dev", &ce_bwd_dev, py::arg("logits"), py::arg("labels"),
        py::arg("lse"), py::arg("acc"), py::arg("dloss_dev"),
        py::arg("epsilon") = 0.0);
  m.def("ce_rows_fwd", &ce_rows_fwd, py::arg("logits"), py::arg("targets"),
        py::arg("lse"), py::arg("tok_loss"), py::arg("epsilon") = 0.0);
  m.def("ce_rows_bwd_", &ce_rows_bwd_, py::arg("logits"), py::arg("targets"),
        py::arg("lse"), py::arg("scale_dev"), py::arg("epsilon") = 0.0);
  m.def("attn_fwd", &attn_fwd, py::arg("q"), py::arg("k"), py::arg("v"),
        py::arg("scale"), py::arg("window"),
        py::arg("doc_start") = py::none());
  m.def("attn_delta", &attn_delta);
  m.def("attn_bwd", &attn_bwd, py::arg("q"), py::arg("k"), py::arg("v"),
        py::arg("dO"), py::arg("lse"), py::arg("delta"), py::arg("scale"),
        py::arg("window"), py::arg("doc_start") = py::none(),
        py::arg("doc_end") = py::none());
  m.def("attn_block_order", &attn_block_order, py::arg("n_blk"),
        py::arg("B"), py::arg("H"), py::arg("heavy_last"));
  m.def("attn_gqa_reduce", &attn_gqa_reduce);
  m.def("attn_gqa_reduce_rope", &attn_gqa_reduce_rope);
  m.def("rope_qk_inplace", &rope_qk_inplace);
  m.def("gemm_nt", &gemm_nt);
  m.def("rope_packed", &rope_packed);
  m.def("attn_fwd_packed", &attn_fwd_packed, py::arg("qkv"), py::arg("H"),
        py::arg("Hkv"), py::arg("D"), py::arg("scale"), py::arg("window"),
        py::arg("q_off"), py::arg("k_off"), py::arg("v_off"),
        py::arg("doc_start") = py::none());
  m.def("attn_bwd_packed", &attn_bwd_packed, py::arg("qkv"), py::arg("dO"),
        py::arg("lse"), py::arg("delta"), py::arg("dqkv"), py::arg("H"),
        py::arg("Hkv"), py::arg("D"), py::arg("scale"), py::arg("window"),
        py::arg("q_off"), py::arg("k_off"), py::arg("v_off"),
        py::arg("cos") = py::none(), py::arg("sin") = py::none(),
        py::arg("doc_start") = py::none(), py::arg("doc_end") = py::none());
  m.attr("_gfx950") = true;
}
