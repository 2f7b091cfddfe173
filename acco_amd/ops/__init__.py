"""Op dispatch: hand-written gfx950 HIP kernels on GPU, torch reference on CPU.

Policy (deliberate, per the MI355X-native mandate): when a tensor is on a
CUDA/HIP device, the op MUST run through the in-tree HIP extension
``acco_amd._hip_ops``; if the extension is missing we raise instead of
silently falling back to ATen. ``ACCO_FORCE_REF=1`` overrides for A/B
numerics debugging only.
"""

from __future__ import annotations

import os
from typing import Optional, Tuple

import torch

from acco_amd.ops import torch_ref

_EXT = None
_EXT_ERR: Optional[str] = None


def _check_fresh(mod) -> None:
    """Warn if the in-tree .so predates any kernel source (a stale binary
    silently satisfies the import and defeats the fail-loud policy —
    round-1 advisor finding)."""
    import glob
    import warnings
    so = getattr(mod, "__file__", None)
    if not so or not os.path.exists(so):
        return
    so_mtime = os.path.getmtime(so)
    csrc = os.path.join(os.path.dirname(so), "ops", "csrc")
    stale = [os.path.basename(f)
             for f in glob.glob(os.path.join(csrc, "*.hip"))
             + glob.glob(os.path.join(csrc, "*.cpp"))
             + glob.glob(os.path.join(csrc, "*.h"))
             if not f.endswith("_hip.hip") and os.path.getmtime(f) > so_mtime]
    if stale:
        warnings.warn(
            f"acco_amd._hip_ops is OLDER than kernel sources {stale}; "
            "rebuild with `python setup.py build_ext --inplace`",
            RuntimeWarning, stacklevel=3)


def _load_ext():
    global _EXT, _EXT_ERR
    if _EXT is not None or _EXT_ERR is not None:
        return _EXT
    try:
        from acco_amd import _hip_ops  # built by setup.py build_ext --inplace
        _check_fresh(_hip_ops)
        _EXT = _hip_ops
    except ImportError as e:  # remember why, for the loud failure below
        _EXT_ERR = str(e)
    return _EXT


def hip_ext():
    """The HIP extension module, or a loud failure on a GPU box."""
    ext = _load_ext()
    if ext is None:
        raise RuntimeError(
            "acco_amd._hip_ops is not built but a CUDA tensor reached an op. "
            "Build it in-tree with `python setup.py build_ext --inplace` "
            f"(import error: {_EXT_ERR})"
        )
    return ext


def ext_available() -> bool:
    return _load_ext() is not None


def have_kernel(name: str) -> bool:
    ext = _load_ext()
    return ext is not None and hasattr(ext, name)


def _use_ref(t: torch.Tensor, kernel: str = "") -> bool:
    """torch-reference path when: CPU tensor, forced via env, or the HIP
    kernel for this op has not been built yet. On a GPU box with the
    extension entirely missing, ops fail loudly instead (hip_ext raises) —
    the kernel registry only tolerates per-op gaps during bring-up."""
    if not t.is_cuda:
        return True
    if os.environ.get("ACCO_FORCE_REF") == "1":
        return True
    if kernel:
        if not ext_available():
            hip_ext()  # raises with the build instructions
        return not have_kernel(kernel)
    return False


# ---------------------------------------------------------------- model ops

def rms_norm(x: torch.Tensor, weight: torch.Tensor, eps: float) -> torch.Tensor:
    if _use_ref(x, "rmsnorm_fwd"):
        return torch_ref.rms_norm(x, weight, eps)
    from acco_amd.ops.autograd import RMSNormFn
    return RMSNormFn.apply(x, weight, eps)


def layer_norm(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor,
               eps: float) -> torch.Tensor:
    if _use_ref(x, "layernorm_fwd"):
        return torch_ref.layer_norm(x, weight, bias, eps)
    from acco_amd.ops.autograd import LayerNormFn
    return LayerNormFn.apply(x, weight, bias, eps)


def add_rms_norm(x: torch.Tensor, res: Optional[torch.Tensor],
                 weight: torch.Tensor, eps: float):
    """(rmsnorm(x+res)·w, x+res) in ONE kernel pass (residual-add fusion);
    res=None degenerates to a plain norm with s = x.
    ACCO_NO_ADDNORM_FUSE=1 keeps the eager add + plain norm (same-box A/B)."""
    if res is None:
        return rms_norm(x, weight, eps), x
    if os.environ.get("ACCO_NO_ADDNORM_FUSE") == "1":
        s = x + res
        return rms_norm(s, weight, eps), s
    if _use_ref(x, "add_rmsnorm_fwd"):
        s = x + res
        return torch_ref.rms_norm(s, weight, eps), s
    from acco_amd.ops.autograd import AddRMSNormFn
    return AddRMSNormFn.apply(x, res, weight, eps)


def add_layer_norm(x: torch.Tensor, res: Optional[torch.Tensor],
                   weight: torch.Tensor, bias: torch.Tensor, eps: float):
    """(layernorm(x+res)·w+b, x+res) in ONE kernel pass; res=None → plain."""
    if res is None:
        return layer_norm(x, weight, bias, eps), x
    if os.environ.get("ACCO_NO_ADDNORM_FUSE") == "1":
        s = x + res
        return layer_norm(s, weight, bias, eps), s
    if _use_ref(x, "add_layernorm_fwd"):
        s = x + res
        return torch_ref.layer_norm(s, weight, bias, eps), s
    from acco_amd.ops.autograd import AddLayerNormFn
    return AddLayerNormFn.apply(x, res, weight, bias, eps)


def gelu_new(x: torch.Tensor) -> torch.Tensor:
    if _use_ref(x, "gelu_fwd"):
        return torch_ref.gelu_new(x)
    from acco_amd.ops.autograd import GeluNewFn
    return GeluNewFn.apply(x)


def swiglu(gate: torch.Tensor, up: torch.Tensor) -> torch.Tensor:
    if _use_ref(gate, "swiglu_fwd"):
        return torch_ref.swiglu(gate, up)
    from acco_amd.ops.autograd import SwiGLUFn
    return SwiGLUFn.apply(gate, up)


def rope_apply(q: torch.Tensor, k: torch.Tensor, cos: torch.Tensor,
               sin: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    if _use_ref(q, "rope_fwd"):
        return torch_ref.rope_apply(q, k, cos, sin)
    from acco_amd.ops.autograd import RoPEFn
    return RoPEFn.apply(q, k, cos, sin)


def doc_start_from_eos(input_ids: torch.Tensor,
                       eos_token_id: int) -> torch.Tensor:
    """int32 [B, S] document starts of packed rows (torch_ref docstring);
    plain torch ops on the device of `input_ids`, no host sync."""
    return torch_ref.doc_start_from_eos(input_ids, eos_token_id)


def doc_end_from_start(doc_start: torch.Tensor) -> torch.Tensor:
    """int32 [B, S] exclusive document ends, the second array the attention
    backward (dkv) needs; derive it once per batch, not per layer."""
    return torch_ref.doc_end_from_start(doc_start)


def causal_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                     scale: Optional[float] = None,
                     window: Optional[int] = None,
                     doc_start: Optional[torch.Tensor] = None,
                     doc_end: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`doc_start` (int32 [B, S]): document-boundary masking of packed rows.
    `doc_end` is doc_end_from_start(doc_start) when the caller has it already
    (the models derive it once per forward); None derives it here."""
    if doc_start is None:
        if _use_ref(q, "attn_fwd"):
            return torch_ref.causal_attention(q, k, v, scale=scale,
                                              window=window)
        S, D = q.shape[1], q.shape[3]
        if S % 64 != 0 or D not in (64, 128) or q.dtype != torch.bfloat16:
            # shapes outside the flash kernel's contract (rare: tests, odd
            # eval batches) run the reference math
            return torch_ref.causal_attention(q, k, v, scale=scale,
                                              window=window)
        from acco_amd.ops.autograd import AttentionFn
        return AttentionFn.apply(q, k, v, scale, window)
    S, D = q.shape[1], q.shape[3]
    if (_use_ref(q, "attn_fwd") or S % 256 != 0 or D not in (64, 128)
            or q.dtype != torch.bfloat16
            or (scale is not None and not 0 < scale < 1e30)):
        # document masks exist in the 32x32 kernels only (and those take a
        # positive scale with them); every other call runs the reference
        # math with the mask
        return torch_ref.causal_attention(q, k, v, scale=scale, window=window,
                                          doc_start=doc_start)
    from acco_amd.ops.autograd import AttentionFn
    doc_start = doc_start.to(torch.int32).contiguous()
    if doc_end is None:
        doc_end = doc_end_from_start(doc_start)
    return AttentionFn.apply(q, k, v, scale, window, doc_start,
                             doc_end.to(torch.int32).contiguous())


# ------------------------------------------------ KV cache (generation)

def _decode_contract(q_heads: int, k_cache: torch.Tensor) -> bool:
    """What the cache kernels take: bf16, D in {64, 128}, 1 <= H/Hkv <= 8."""
    Hkv, D = k_cache.shape[1], k_cache.shape[3]
    return (k_cache.dtype == torch.bfloat16 and D in (64, 128)
            and q_heads % Hkv == 0 and 1 <= q_heads // Hkv <= 8)


def kv_append(k_cache: torch.Tensor, v_cache: torch.Tensor,
              cache_len: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
              q: Optional[torch.Tensor] = None,
              cos: Optional[torch.Tensor] = None,
              sin: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
    """Append k, v [B, T, Hkv, D] to the caches [B, Hkv, Smax, D] at row
    cache_len[b] + t, in place; rows at or beyond Smax are dropped and
    `cache_len` (int32 [B], on the device) is left alone (torch_ref.kv_append
    has the semantics). With cos / sin ([>= Smax, D] fp32) K is rotated by its
    absolute position and the rotated `q` [B, T, H, D] is returned.

    k, v and q may be views of the packed projection output (a column
    section `[..., off:off + h*D]` viewed as [B, T, h, D]): the HIP kernel
    reads them through their row stride, no copies. One launch, no host
    sync."""
    heads = q.shape[2] if q is not None else k_cache.shape[1]
    if (_use_ref(k_cache, "kv_append") or k.dtype != torch.bfloat16
            or not _decode_contract(heads, k_cache)):
        return torch_ref.kv_append(k_cache, v_cache, cache_len, k, v, q,
                                   cos, sin)
    return hip_ext().kv_append(q if cos is not None else None, k, v, cos,
                               sin, k_cache, v_cache, cache_len)


def decode_attention(q: torch.Tensor, k_cache: torch.Tensor,
                     v_cache: torch.Tensor, cache_len: torch.Tensor,
                     scale: Optional[float] = None,
                     window: Optional[int] = None) -> torch.Tensor:
    """o [B, H, D] of one query token per sequence, q [B, H, D], against the
    caches [B, Hkv, Smax, D]: the query is the last of cache_len[b] cached
    tokens and attends keys [max(0, L - window), L), L = clamp(cache_len[b],
    0, Smax) (torch_ref.decode_attention has the semantics). HIP
    flash-decoding kernel for bf16, D in {64, 128}, 1 <= H/Hkv <= 8; the
    torch reference outside that contract. No host sync."""
    if (_use_ref(q, "attn_decode") or q.dtype != torch.bfloat16
            or not _decode_contract(q.shape[1], k_cache)):
        return torch_ref.decode_attention(q, k_cache, v_cache, cache_len,
                                          scale=scale, window=window)
    if scale is None:
        scale = q.shape[2] ** -0.5
    return hip_ext().attn_decode(q, k_cache, v_cache, cache_len,
                                 float(scale), int(window or 0))


def decode_attention_splits(bhkv: int, smax: int) -> Tuple[int, int]:
    """(n_split, chunk) of the HIP decode attention for B·Hkv (sequence, kv
    head) pairs and a cache of Smax rows: workgroup i of a pair owns keys
    [i·chunk, (i+1)·chunk). A host function of its two arguments only."""
    n_split, chunk = hip_ext().attn_decode_grid(int(bhkv), int(smax))
    return int(n_split), int(chunk)


def sample_logits(logits: torch.Tensor, *, temperature: float, top_k: int = 0,
                  top_p: float = 1.0, seed: int, step: int,
                  done: Optional[torch.Tensor] = None, eos_id: int = -1
                  ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor,
                             torch.Tensor]:
    """One token per row of logits [B, V], drawn on the logits' device:
    (token int64 [B] in [0, V), logprob fp32 [B], thr bf16 [B], n_kept int32
    [B]). temperature > 0: top-k (0 = off), then top-p (>= 1 = off), then a
    Gumbel-max draw from a counter-based generator keyed by (seed, step, row,
    index): a pure function of its arguments, bitwise reproducible.
    temperature == 0: the argmax. `done` (uint8 [B], updated in place) with
    0 <= eos_id < V pins finished rows to eos_id (torch_ref.sample_logits has
    the semantics). The caller counts `step`; nothing is read from the device.
    One HIP kernel for bf16 on the GPU; the fp64 reference for CPU tensors,
    other dtypes and ACCO_FORCE_REF=1."""
    if _use_ref(logits) or logits.dtype != torch.bfloat16:
        return torch_ref.sample_logits(
            logits, temperature=temperature, top_k=top_k, top_p=top_p,
            seed=seed, step=step, done=done, eos_id=eos_id)
    mask = (1 << 64) - 1
    token, logprob, thr, n_kept = hip_ext().sample_logits(
        logits, float(temperature), int(top_k), float(top_p),
        int(seed) & mask, int(step) & mask, done, int(eos_id))
    return token, logprob, thr, n_kept


def causal_lm_loss(logits: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    if _use_ref(logits, "ce_fwd"):
        return torch_ref.causal_lm_loss(logits, labels)
    from acco_amd.ops.autograd import CausalLMLossFn
    return CausalLMLossFn.apply(logits, labels)


def label_smoothed_causal_lm_loss(logits: torch.Tensor, labels: torch.Tensor,
                                  epsilon: float) -> torch.Tensor:
    """HF-LabelSmoother-equivalent shifted loss fused into the CE kernel
    (reference utils/trainer_utils.py:862-902)."""
    if epsilon == 0.0:
        return causal_lm_loss(logits, labels)
    if _use_ref(logits, "ce_fwd"):
        return torch_ref.label_smoothed_causal_lm_loss(logits, labels, epsilon)
    from acco_amd.ops.autograd import CausalLMLossFn
    return CausalLMLossFn.apply(logits, labels, epsilon)


def linear_causal_lm_loss(hidden: torch.Tensor, weight: torch.Tensor,
                          labels: torch.Tensor, epsilon: float = 0.0,
                          chunk_tokens: int = 4096,
                          grad_view: Optional[torch.Tensor] = None
                          ) -> torch.Tensor:
    """lm_head + shifted causal-LM loss without the [B, S, V] logits: the
    scalar mean loss of `hidden @ weight^T` (hidden [B, S, H], weight [V, H],
    no bias) against labels [B, S] over the valid shifted tokens (a label is
    valid iff 0 <= label < V), with HF-LabelSmoother smoothing for
    epsilon != 0. Logits exist for `chunk_tokens` rows at a time, in one
    reused buffer of chunk_tokens·V elements; the backward recomputes them
    (one extra head GEMM per step) and overwrites them with dlogits in
    place. The loss is summed in a fixed order: bitwise reproducible.

    With `grad_view` (the grad-arena view aliasing `weight`) dW accumulates
    into it in place, one chunk at a time, the producer notifier fires once
    after the last chunk and no weight gradient is returned; without it the
    chunks accumulate in fp32 and dW comes back cast once.

    On the GPU: bf16 contiguous hidden and weight, row kernels of
    ce.hip. CPU tensors and ACCO_FORCE_REF=1 run the same chunking in
    torch math."""
    if _use_ref(hidden):
        return torch_ref.linear_causal_lm_loss(hidden, weight, labels,
                                               epsilon, chunk_tokens,
                                               grad_view)
    hip_ext()   # a missing extension is an error, not a fallback
    if int(chunk_tokens) < 1:
        raise ValueError(f"chunk_tokens must be >= 1, got {chunk_tokens}")
    if not (hidden.dtype == weight.dtype == torch.bfloat16
            and hidden.is_contiguous() and weight.is_contiguous()
            and hidden.dim() == 3 and weight.dim() == 2
            and weight.shape[1] == hidden.shape[2]):
        raise RuntimeError(
            "linear_causal_lm_loss on the GPU needs contiguous bf16 hidden "
            f"[B, S, H] and weight [V, H], got {hidden.dtype} "
            f"{tuple(hidden.shape)} (contiguous={hidden.is_contiguous()}) and "
            f"{weight.dtype} {tuple(weight.shape)} "
            f"(contiguous={weight.is_contiguous()})")
    from acco_amd.ops.autograd import LinearCausalLMLossFn
    targets, n_valid = torch_ref.shifted_targets(labels, weight.shape[0])
    return LinearCausalLMLossFn.apply(
        hidden.view(-1, hidden.shape[-1]), weight, targets, n_valid,
        float(epsilon), int(chunk_tokens), grad_view)


# ------------------------------------------------------------- trainer ops

def grad_sumsq_partials(n: int, dtype: torch.dtype, device=None) -> int:
    """Number of fp32 partials `grad_sumsq` writes for `n` elements of
    `dtype` on `device` (default: the GPU when there is one): the kernel's
    block count on the GPU, 1 for the CPU reference."""
    if device is None:
        device = "cuda" if torch.cuda.is_available() else "cpu"
    if (torch.device(device).type != "cuda"
            or os.environ.get("ACCO_FORCE_REF") == "1"):
        return 1
    return int(hip_ext().grad_sumsq_grid(int(n), dtype == torch.bfloat16))


def grad_sumsq(g: torch.Tensor, partials: torch.Tensor) -> int:
    """Sum of squares of a bf16 / fp32 gradient segment into fp32 partial
    sums `partials[:count]`; returns count (= grad_sumsq_partials). Every
    slot is stored, zero included, so the workspace needs no clearing; the
    rest of `partials` is left alone. One streaming HIP kernel on GPU."""
    if _use_ref(g):
        return torch_ref.grad_sumsq(g, partials)
    return int(hip_ext().grad_sumsq(g, partials))


def sumsq_finalize(partials: torch.Tensor, out: torch.Tensor) -> None:
    """out (1-element fp32) = sum of all of `partials`, in double, in a
    fixed order. One single-block HIP kernel on GPU."""
    if _use_ref(partials):
        torch_ref.sumsq_finalize(partials, out)
        return
    hip_ext().sumsq_finalize(partials, out)


def clip_grad_scale(sumsq: torch.Tensor, grad_scale, max_norm: float,
                    eps: float = 1e-6):
    """(scale, norm, coef) of global-norm clipping, clip_grad_norm_'s formula
    folded into the AdamW gradient scale (torch_ref docstring). A few torch
    ops on 1-element tensors on sumsq's device, no host sync: the scalar
    all-reduce sits between the finalize kernel and this step."""
    return torch_ref.clip_grad_scale(sumsq, grad_scale, max_norm, eps)


def fused_adamw_step(p: torch.Tensor, g: torch.Tensor, m: torch.Tensor,
                     v: torch.Tensor, step: int, lr: float, beta1: float,
                     beta2: float, eps: float, weight_decay: float,
                     grad_scale: float = 1.0,
                     out_bf16: Optional[torch.Tensor] = None,
                     commit: bool = True) -> None:
    """Sharded AdamW on the local fp32 shard, with bf16-grad cast, 1/count
    scale, optional bf16 write-out, and the ACCO tentative (no-commit) mode.
    One HIP kernel on GPU (K3+K4+K5+K7 of SURVEY.md §2.5 fused)."""
    if _use_ref(p):
        torch_ref.fused_adamw_step(p, g, m, v, step, lr, beta1, beta2, eps,
                                   weight_decay, grad_scale, out_bf16, commit)
        return
    if isinstance(grad_scale, torch.Tensor):
        scale, scale_dev = 1.0, grad_scale.float()
    else:
        scale = float(grad_scale)
        scale_dev = torch.empty(0, device=p.device, dtype=torch.float32)
    if out_bf16 is None:
        out_bf16 = torch.empty(0, device=p.device, dtype=g.dtype)
    hip_ext().fused_adamw(p, g, m, v, int(step), float(lr), float(beta1),
                          float(beta2), float(eps), float(weight_decay),
                          scale, scale_dev, out_bf16, bool(commit))
