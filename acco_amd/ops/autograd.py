"""torch.autograd.Function wrappers around the gfx950 HIP kernels.

Only imported on the GPU path (ops/__init__ dispatch); each Function pairs a
hand-written forward kernel with its hand-written backward kernel, with
fp32 row statistics saved between them. Numerics tests compare each against
the fp32 torch reference (tests/test_gpu_kernels.py).
"""

from __future__ import annotations

import torch

from acco_amd import ops


class SwiGLUFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gate, up):
        gate = gate.contiguous()
        up = up.contiguous()
        ctx.save_for_backward(gate, up)
        return ops.hip_ext().swiglu_fwd(gate, up)

    @staticmethod
    def backward(ctx, dout):
        gate, up = ctx.saved_tensors
        dg, du = ops.hip_ext().swiglu_bwd(dout.contiguous(), gate, up)
        return dg, du


class SwiGLUPackedFn(torch.autograd.Function):
    """SwiGLU over the packed [.., 2I] fused gate_up output: no
    split/contiguous forward, single dgu write backward (no cat)."""

    @staticmethod
    def forward(ctx, gu):
        gu = gu.contiguous()
        ctx.save_for_backward(gu)
        return ops.hip_ext().swiglu_packed_fwd(gu)

    @staticmethod
    def backward(ctx, dout):
        (gu,) = ctx.saved_tensors
        return ops.hip_ext().swiglu_packed_bwd(dout.contiguous(), gu)


class GeluNewFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = x.contiguous()
        ctx.save_for_backward(x)
        return ops.hip_ext().gelu_fwd(x)

    @staticmethod
    def backward(ctx, dout):
        (x,) = ctx.saved_tensors
        return ops.hip_ext().gelu_bwd(dout.contiguous(), x)


class RMSNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, eps):
        x = x.contiguous()
        y, rstd = ops.hip_ext().rmsnorm_fwd(x, weight.contiguous(), eps)
        ctx.save_for_backward(x, weight, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, rstd = ctx.saved_tensors
        dx, dw = ops.hip_ext().rmsnorm_bwd(dy.contiguous(), x,
                                           weight.contiguous(), rstd, None)
        return dx, dw, None


class AddRMSNormFn(torch.autograd.Function):
    """Fused residual-add + RMSNorm: (y, s) = (rmsnorm(x+res)·w, bf16(x+res)).
    The backward folds the residual branch's grad (ds) into the norm-bwd
    kernel's dx write — the eager add/accumulate kernels at every residual
    site disappear (guide: fuse elementwise work into the producing kernel)."""

    @staticmethod
    def forward(ctx, x, res, weight, eps):
        y, s, rstd = ops.hip_ext().add_rmsnorm_fwd(
            x.contiguous(), res.contiguous(), weight.contiguous(), eps)
        ctx.save_for_backward(s, weight, rstd)
        return y, s

    @staticmethod
    def backward(ctx, dy, ds):
        s, weight, rstd = ctx.saved_tensors
        dadd = ds.contiguous() if ds is not None else None
        dx, dw = ops.hip_ext().rmsnorm_bwd(dy.contiguous(), s,
                                           weight.contiguous(), rstd, dadd)
        # d(x) == d(res): both inputs feed the same sum
        return dx, dx, dw, None


class LayerNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, eps):
        x = x.contiguous()
        y, mean, rstd = ops.hip_ext().layernorm_fwd(x, weight.contiguous(),
                                                    bias.contiguous(), eps)
        ctx.save_for_backward(x, weight, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, mean, rstd = ctx.saved_tensors
        dx, dw, db = ops.hip_ext().layernorm_bwd(dy.contiguous(), x,
                                                 weight.contiguous(), mean,
                                                 rstd, None)
        return dx, dw, db, None


class AddLayerNormFn(torch.autograd.Function):
    """Fused residual-add + LayerNorm (GPT-Neo blocks); see AddRMSNormFn."""

    @staticmethod
    def forward(ctx, x, res, weight, bias, eps):
        y, s, mean, rstd = ops.hip_ext().add_layernorm_fwd(
            x.contiguous(), res.contiguous(), weight.contiguous(),
            bias.contiguous(), eps)
        ctx.save_for_backward(s, weight, mean, rstd)
        return y, s

    @staticmethod
    def backward(ctx, dy, ds):
        s, weight, mean, rstd = ctx.saved_tensors
        dadd = ds.contiguous() if ds is not None else None
        dx, dw, db = ops.hip_ext().layernorm_bwd(dy.contiguous(), s,
                                                 weight.contiguous(), mean,
                                                 rstd, dadd)
        return dx, dx, dw, db, None


class RoPEFn(torch.autograd.Function):
    """q: [B,S,H,D], k: [B,S,Hkv,D]; cos/sin fp32 [S,D] host-precomputed."""

    @staticmethod
    def forward(ctx, q, k, cos, sin):
        cos = cos.float().contiguous()
        sin = sin.float().contiguous()
        ext = ops.hip_ext()
        q2 = ext.rope_fwd(q.contiguous(), cos, sin, False)
        k2 = ext.rope_fwd(k.contiguous(), cos, sin, False)
        ctx.save_for_backward(cos, sin)
        return q2, k2

    @staticmethod
    def backward(ctx, dq, dk):
        cos, sin = ctx.saved_tensors
        ext = ops.hip_ext()
        dq0 = ext.rope_fwd(dq.contiguous(), cos, sin, True)
        dk0 = ext.rope_fwd(dk.contiguous(), cos, sin, True)
        return dq0, dk0, None, None


class CausalLMLossFn(torch.autograd.Function):
    """Fused shifted CE: logits [B,S,V] bf16, labels [B,S] int64.
    epsilon != 0 adds HF-LabelSmoother semantics inside the same kernel
    pass."""

    @staticmethod
    def forward(ctx, logits, labels, epsilon=0.0):
        logits = logits.contiguous()
        if logits.data_ptr() % 16 != 0:
            # the kernels load 16-byte vectors from a 16-byte aligned base;
            # GEMM outputs are, an offset view into a larger buffer may not be
            logits = logits.clone()
        labels = labels.contiguous()
        acc, lse = ops.hip_ext().ce_fwd(logits, labels, float(epsilon))
        ctx.save_for_backward(logits, labels, lse, acc)
        ctx.epsilon = float(epsilon)
        return acc[0] / acc[1].clamp(min=1.0)

    @staticmethod
    def backward(ctx, grad_out):
        logits, labels, lse, acc = ctx.saved_tensors
        # the upstream grad is read on-device — float(grad_out) would be a
        # D2H sync stalling the backward launch pipeline every micro
        dlogits = ops.hip_ext().ce_bwd_dev(
            logits, labels, lse, acc,
            grad_out.reshape(1).to(logits.device, torch.float32), ctx.epsilon)
        return dlogits, None, None


class HipRows:
    """Row kernels of the chunked lm_head + loss (ce.hip, Rows policy):
    per-row lse and loss in fp32, dlogits in place, the loss summed in
    double in a fixed order by the finalize kernel."""

    @staticmethod
    def stat_dtype(dtype):
        return torch.float32

    @staticmethod
    def fwd(lg, tg, lse, tok, eps):
        ops.hip_ext().ce_rows_fwd(lg, tg, lse, tok, eps)

    @staticmethod
    def bwd_(lg, tg, lse, scale, eps):
        ops.hip_ext().ce_rows_bwd_(lg, tg, lse, scale, eps)

    @staticmethod
    def total(tok):
        out = torch.empty(1, dtype=torch.float32, device=tok.device)
        ops.hip_ext().sumsq_finalize(tok, out)
        return out


class LinearCausalLMLossFn(torch.autograd.Function):
    """lm_head GEMM + shifted CE, `chunk_tokens` rows of logits at a time
    (torch_ref.chunked_lm_loss_forward / _backward hold the chunk loop):
    hidden2 [T, H] and weight [V, H] bf16 contiguous, targets int64 [T]
    already shifted, n_valid a device scalar. Saves no logits."""

    @staticmethod
    def forward(ctx, hidden2, weight, targets, n_valid, epsilon, chunk_tokens,
                grad_view):
        return ops.torch_ref.chunked_lm_loss_forward(
            ctx, HipRows, hidden2, weight, targets, n_valid, epsilon,
            chunk_tokens, grad_view)

    @staticmethod
    def backward(ctx, grad_out):
        dh, dw = ops.torch_ref.chunked_lm_loss_backward(ctx, grad_out)
        return dh, dw, None, None, None, None, None


class AttnQKVPackedFn(torch.autograd.Function):
    """The whole attention core over the PACKED fused projection output
    [B, S, (H+2Hkv)·D]: optional RoPE + flash attention v4 forward; backward
    emits one packed grad — no torch.split forward copies, no cat backward.
    D in {64, 128}, S%256==0. Section offsets support both packing orders
    (Llama q|k|v, GPT-Neo k|v|q); window>0 = GPT-Neo local attention.

    With RoPE the q|k sections of `qkv` are rotated IN PLACE by one launch
    (the producer, FusedArenaLinearFn, saves only its inputs; the unroped
    projection is never read again) and the inverse rotation of the grad is
    folded into the dq kernel's epilogue and the GQA reduce; the call then
    returns (o, qkv), since a tensor marked dirty has to be an output.
    Without RoPE (cos is None) it returns o alone.

    doc_start / doc_end (int32 [B, S], both or neither): document-boundary
    masking of packed rows, the DOC builds of the three kernels."""

    @staticmethod
    def forward(ctx, qkv, cos, sin, H, Hkv, D, scale, window, offs,
                doc_start=None, doc_end=None):
        ext = ops.hip_ext()
        qkv = qkv.contiguous()
        q_off, k_off, v_off = offs
        if cos is not None:
            cos = cos.float().contiguous()
            sin = sin.float().contiguous()
            if qkv._is_view() or (qkv.is_leaf and qkv.requires_grad):
                # autograd forbids in-place on these: rotate a private copy
                qkv = qkv.clone()
            else:
                ctx.mark_dirty(qkv)
            ext.rope_qk_inplace(qkv, cos, sin, H, Hkv, D, q_off, k_off)
        roped = qkv
        if (doc_start is None) != (doc_end is None):
            raise RuntimeError("doc_start and doc_end must both be given "
                               "or both be None")
        if doc_start is None:
            o, lse = ext.attn_fwd_packed(roped, H, Hkv, D, float(scale),
                                         int(window or 0), q_off, k_off,
                                         v_off)
        else:
            o, lse = ext.attn_fwd_packed(roped, H, Hkv, D, float(scale),
                                         int(window or 0), q_off, k_off,
                                         v_off, doc_start)
        ctx.save_for_backward(roped, o, lse,
                              cos if cos is not None else torch.empty(0),
                              sin if sin is not None else torch.empty(0),
                              *(() if doc_start is None
                                else (doc_start, doc_end)))
        ctx.meta = (H, Hkv, D, float(scale), int(window or 0), offs)
        if cos is None:
            return o                 # [B, S, H*D]; qkv untouched
        ctx.set_materialize_grads(False)   # no zeros for the unused output
        return o, roped

    @staticmethod
    def backward(ctx, dO, _droped=None):
        ext = ops.hip_ext()
        roped, o, lse, cos, sin, *doc = ctx.saved_tensors
        doc_start, doc_end = doc if doc else (None, None)
        H, Hkv, D, scale, window, offs = ctx.meta
        q_off, k_off, v_off = offs
        B, S, W = roped.shape
        dO = dO.contiguous()
        delta = ext.attn_delta(dO.view(B, S, H, D), o.view(B, S, H, D))
        dqkv = torch.empty_like(roped)
        rope = cos.numel() > 0
        # with RoPE the dq kernel rotates its result by -theta in the
        # epilogue (bit-equal to the stand-alone inverse rope pass)
        dkq, dvq = ext.attn_bwd_packed(roped, dO, lse, delta, dqkv, H, Hkv,
                                       D, scale, window, q_off, k_off, v_off,
                                       cos if rope else None,
                                       sin if rope else None,
                                       doc_start, doc_end)
        rep = H // Hkv
        if rope:
            # group-sum + inverse rotation of dk + bf16 cast in one pass
            ext.attn_gqa_reduce_rope(dkq, dvq, dqkv, cos, sin, Hkv, rep, D,
                                     k_off, v_off)
        else:
            # one pass: group-sum over the rep query heads + bf16 cast +
            # strided write into the packed grad's k|v sections (replaces
            # two dim-3 sums, two casts and two strided copies per layer)
            ext.attn_gqa_reduce(dkq, dvq, dqkv, Hkv, rep, D, k_off, v_off)
        return (dqkv, None, None, None, None, None, None, None, None,
                None, None)


class AttentionFn(torch.autograd.Function):
    """Flash-style causal attention, gfx950 MFMA (fwd: online softmax;
    bwd: FA2-style recompute, dq + dkv kernels). [B,S,H,D] layout,
    D ∈ {64,128}, S % 64 == 0 (the dispatch falls back to torch_ref for
    other shapes). doc_start / doc_end (int32 [B, S], both or neither):
    document-boundary masking of packed rows; needs S % 256 == 0."""

    @staticmethod
    def forward(ctx, q, k, v, scale, window, doc_start=None, doc_end=None):
        import math
        if scale is None:
            scale = 1.0 / math.sqrt(q.shape[-1])
        w = int(window) if window else 0
        q = q.contiguous()
        k = k.contiguous()
        v = v.contiguous()
        if (doc_start is None) != (doc_end is None):
            raise RuntimeError("doc_start and doc_end must both be given "
                               "or both be None")
        if doc_start is None:
            o, lse = ops.hip_ext().attn_fwd(q, k, v, float(scale), w)
            ctx.save_for_backward(q, k, v, o, lse)
        else:
            o, lse = ops.hip_ext().attn_fwd(q, k, v, float(scale), w,
                                            doc_start)
            ctx.save_for_backward(q, k, v, o, lse, doc_start, doc_end)
        ctx.scale = float(scale)
        ctx.window = w
        return o

    @staticmethod
    def backward(ctx, dO):
        q, k, v, o, lse, *doc = ctx.saved_tensors
        doc_start, doc_end = doc if doc else (None, None)
        dO = dO.contiguous()
        # Delta[b,h,s] = rowsum(dO ∘ O) in fp32, laid out [B,H,S] (one
        # fused kernel; was a 4-kernel ATen cast/mul/reduce chain)
        delta = ops.hip_ext().attn_delta(dO, o)
        dq, dkq, dvq = ops.hip_ext().attn_bwd(q, k, v, dO, lse, delta,
                                              ctx.scale, ctx.window,
                                              doc_start, doc_end)
        B, S, H, D = q.shape
        Hkv = k.shape[2]
        if Hkv != H:
            rep = H // Hkv
            dk = dkq.view(B, S, Hkv, rep, D).sum(3, dtype=torch.float32).to(k.dtype)
            dv = dvq.view(B, S, Hkv, rep, D).sum(3, dtype=torch.float32).to(v.dtype)
        else:
            dk, dv = dkq, dvq
        return dq, dk, dv, None, None, None, None
