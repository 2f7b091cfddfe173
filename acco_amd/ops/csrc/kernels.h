// Prototypes of every extern "C" launcher of the gfx950 kernels, the one
// place a launcher's signature is written down. Each .hip file that defines
// a launcher includes this header, so the compiler checks the definition
// against the prototype the bindings call through (extern "C" names are not
// mangled: a drifted declaration would link cleanly and pass garbage).
#pragma once

#include <hip/hip_runtime.h>

extern "C" {

// ---- adamw.hip
void acco_fused_adamw_launch(void* p, const void* g, void* m, void* v,
                             void* out, const float* scale_dev, long long n,
                             bool buf_is_bf16, bool commit, float scale,
                             float lr, float beta1, float beta2, float eps,
                             float weight_decay, long long step_plus_1,
                             hipStream_t stream);

// ---- gradnorm.hip
// sum of squares of g[0..n) as acco_grad_sumsq_grid(n, is_bf16) fp32
// partials (host only: the launch's block count; n = 0 gives one zero
// partial); the finalize sums `count` partials in double into out[0]
int acco_grad_sumsq_grid(long long n, bool is_bf16);
void acco_grad_sumsq(const void* g, float* partials, long long n,
                     bool is_bf16, hipStream_t stream);
void acco_sumsq_finalize(const float* partials, long long count, float* out,
                         hipStream_t stream);

// ---- elementwise.hip
void acco_swiglu_fwd(const void* g, const void* u, void* out, long long n,
                     int cols, long long row_stride8, hipStream_t s);
void acco_swiglu_bwd(const void* dout, const void* g, const void* u, void* dg,
                     void* du, long long n, int cols, long long row_stride8,
                     hipStream_t s);
void acco_gelu_fwd(const void* x, void* out, long long n, hipStream_t s);
void acco_gelu_bwd(const void* dout, const void* x, void* dx, long long n,
                   hipStream_t s);

// ---- norms.hip
void acco_rmsnorm_fwd(const void* x, const void* w, void* y, void* rstd,
                      const void* res, void* sum_out, long long R, int D,
                      float eps, hipStream_t s);
void acco_rmsnorm_bwd(const void* dy, const void* x, const void* w,
                      const void* rstd, void* dx, void* dw_fp32,
                      const void* dadd, long long R, int D, hipStream_t s);
void acco_layernorm_fwd(const void* x, const void* w, const void* b, void* y,
                        void* mean, void* rstd, const void* res,
                        void* sum_out, long long R, int D, float eps,
                        hipStream_t s);
void acco_layernorm_bwd(const void* dy, const void* x, const void* w,
                        const void* mean, const void* rstd, void* dx,
                        void* dw_fp32, void* db_fp32, const void* dadd,
                        long long R, int D, hipStream_t s);
int acco_norm_bwd_grid(long long R, int D);
void acco_norm_dw_finalize(const float* dw_part, const float* db_part,
                           void* dw, void* db, int P, int D, bool out_bf16,
                           hipStream_t s);
void acco_colsum(const void* in, float* out, long long P, int D,
                 bool in_is_bf16, hipStream_t s);

// ---- rope.hip
void acco_rope(const void* x, void* y, const float* cos_t, const float* sin_t,
               long long B, int S, int H, int D, bool bwd,
               long long row_stride, hipStream_t stream);
void acco_rope_qk_inplace(void* qkv, const float* cos_t, const float* sin_t,
                          long long T, int S, int H, int Hkv, int D,
                          long long W, long long q_off, long long k_off,
                          hipStream_t stream);

// KV-cache append of T tokens per sequence: k / v (row strides k_rs / v_rs,
// heads contiguous inside a row) into caches [B, Hkv, Smax, D] at row
// clamp(cache_len[b], 0, Smax) + t, rows >= Smax dropped. cos_t / sin_t
// (fp32 [table_rows >= Smax, D]) non-null: K rotated by its absolute
// position, rotated q (row stride q_rs) stored to q_out [B, T, H, D]; null:
// K copied, q and q_out unused. cache_len (int32 [B], device) is not modified.
void acco_kv_append(const void* q, const void* k, const void* v, void* q_out,
                    void* k_cache, void* v_cache, const int* cache_len,
                    const float* cos_t, const float* sin_t, int B, int T,
                    int H, int Hkv, int D, int Smax, int table_rows,
                    long long q_rs, long long k_rs, long long v_rs,
                    hipStream_t stream);

// ---- attention_decode.hip
// One query token per sequence against the cache: q [B, H, D] (row stride
// q_rs), caches [B, Hkv, Smax, D], keys [max(0, L - window), L) with
// L = clamp(cache_len[b], 0, Smax), window 0 = none; D in {64, 128},
// 1 <= H / Hkv <= 8. The key range is split over n_split workgroups of
// `chunk` keys each (host only, a function of B * Hkv and Smax); workspace:
// B * H * n_split * (2 + D) fp32, written before it is read.
void acco_attn_decode_grid(long long BHkv, int Smax, int* n_split,
                           int* chunk);
void acco_attn_decode(const void* q, const void* k_cache, const void* v_cache,
                      const int* cache_len, void* o, float* workspace, int B,
                      int H, int Hkv, int D, int Smax, float scale,
                      int window, long long q_rs, hipStream_t stream);

// ---- ce.hip
// bf16 logits on a 16-byte aligned base (any V). A token is valid iff
// 0 <= target < V; any other target (-100, >= V) is ignored: lse 0, no loss,
// not counted in n_valid, zero dlogits row, never used as an index.
//
// Whole [B, S, V] logits, T = B·S: row t takes labels[t + 1], a sequence's
// last position none. fwd stores lse[t] and atomicAdds {loss_sum, n_valid}
// into the 128 zeroed shards of acc [128, 2]; bwd writes dlogits scaled by
// (dloss_dev ? *dloss_dev : dloss) / max(acc[1], 1), acc the shards' sum.
void acco_ce_fwd(const void* logits, const long long* labels, float* lse,
                 float* acc, long long T, int S, int V, float epsilon,
                 hipStream_t s);
void acco_ce_bwd(const void* logits, const long long* labels,
                 const float* lse, void* dlogits, const float* acc,
                 float dloss, const float* dloss_dev, long long T, int S,
                 int V, float epsilon, hipStream_t s);
// Rows [T, V], targets[t] the label of row t: fwd stores lse[t] and
// tok_loss[t] for every t (0 on ignored rows), bwd overwrites the rows with
// dlogits scaled by the device scalar *scale_dev
void acco_ce_rows_fwd(const void* logits, const long long* targets,
                      float* lse, float* tok_loss, long long T, int V,
                      float epsilon, hipStream_t s);
void acco_ce_rows_bwd(void* logits_inout, const long long* targets,
                      const float* lse, const float* scale_dev, long long T,
                      int V, float epsilon, hipStream_t s);

// ---- sample.hip
// One token per row of bf16 logits [B, V] (rows row_stride elements apart,
// any alignment): temperature, top-k (0 = off, ties at the threshold kept),
// top-p (>= 1 = off, on the top-k survivors) and a Gumbel-max draw keyed by
// (seed, step, row, index); temperature == 0 is the argmax and ignores the
// filters. Outputs by ordinary stores: token int64 [B] in [0, V), logprob
// fp32 [B], thr bf16 [B], n_kept int32 [B]. done (uint8 [B], nullable): a set
// flag makes the row's token eos_id (in [0, V)) with nothing drawn, otherwise
// done[b] = (token == eos_id). One workgroup per row, bitwise reproducible.
void acco_sample_logits(const void* logits, long long row_stride, int B,
                        int V, float temperature, int top_k, double top_p,
                        unsigned long long seed, unsigned long long step,
                        unsigned char* done, long long eos_id,
                        long long* token, float* logprob, void* thr,
                        int* n_kept, hipStream_t s);

// ---- gemm_nt.hip
void acco_gemm_nt(const void* A, const void* B, void* C, int M, int N, int K,
                  hipStream_t stream);

// ---- attention_fwd.hip, attention_fwd32.hip
// The 32x32 launchers take document bounds for packed rows: doc_start (fwd,
// dq) / doc_end (dkv), int32 [B, S] on the device, or nullptr for the plain
// causal / window kernels.
void acco_attn_fwd(const void* q, const void* k, const void* v, void* o,
                   float* lse, int B, int S, int H, int Hkv, int D,
                   float scale, int window, hipStream_t stream);
void acco_attn_fwd32(const void* q, const void* k, const void* v, void* o,
                     float* lse, int B, int S, int H, int Hkv, int D,
                     float scale, int window, long long q_rs, long long kv_rs,
                     long long o_rs, const int* doc_start,
                     hipStream_t stream);

// host only: attn::block_order for every block id, out[2 * id] = row block,
// out[2 * id + 1] = b * H + h (for the tests of the order)
void acco_attn_block_order(int* out, int n_blk, int B, int H,
                           bool heavy_last);

// ---- attention_bwd.hip, attention_bwd32.hip
void acco_attn_bwd_dq(const void* q, const void* k, const void* v,
                      const void* dO, const float* lse, const float* delta,
                      void* dq, int B, int S, int H, int Hkv, int D,
                      float scale, int window, hipStream_t stream);
void acco_attn_bwd_dkv(const void* q, const void* k, const void* v,
                       const void* dO, const float* lse, const float* delta,
                       void* dk, void* dv, int B, int S, int H, int Hkv,
                       int D, float scale, int window, hipStream_t stream);
void acco_attn_bwd32_dq(const void* q, const void* k, const void* v,
                        const void* dO, const float* lse, const float* delta,
                        void* dq, int B, int S, int H, int Hkv, int D,
                        float scale, int window, long long q_rs,
                        long long kv_rs, long long do_rs, long long dq_rs,
                        const float* rope_cos, const float* rope_sin,
                        const int* doc_start, hipStream_t stream);
void acco_attn_bwd32_dkv(const void* q, const void* k, const void* v,
                         const void* dO, const float* lse,
                         const float* delta, void* dk, void* dv, int B,
                         int S, int H, int Hkv, int D, float scale,
                         int window, long long q_rs, long long kv_rs,
                         long long do_rs, const int* doc_end,
                         hipStream_t stream);

// ---- delta.hip
void acco_attn_delta(const void* dO, const void* O, float* delta, long long B,
                     int S, int H, int D, hipStream_t stream);
void acco_attn_gqa_reduce(const void* dkq, const void* dvq, void* dqkv,
                          long long T, int Hkv, int rep, int D, long long W,
                          long long k_off, long long v_off,
                          hipStream_t stream);
void acco_attn_gqa_reduce_rope(const void* dkq, const void* dvq, void* dqkv,
                               const float* cos_t, const float* sin_t,
                               long long T, int S, int Hkv, int rep, int D,
                               long long W, long long k_off, long long v_off,
                               hipStream_t stream);

}  // extern "C"
