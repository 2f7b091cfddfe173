"""FP8 (e4m3) weight-only linears for generation: every projection of a model
stored as one-byte codes with one fp32 scale per output row
(torch_ref.weight_quantize), half the weight bytes a decode step streams and
half the weight memory of a model that is only generated from. Activations
stay bf16; `ops.linear_w8` is the product for up to 64 rows of activations
(decode) and `ops.gemm_w8` for more (prefill, long extends, batched
speculative rounds), both HIP kernels that read the codes as codes. Nothing
here trains.

The same in OCP MXFP4 (`W4Linear`, `ops.linear_w4` / `ops.gemm_w4`): e2m1
codes with one power-of-two scale per 32 weights
(torch_ref.weight_quantize_mxfp4), about 0.53 bytes per weight. With
`act_dtype=torch.float8_e4m3fn` a W4Linear also rounds the activations of its
wide calls (65 rows and more) to OCP MXFP8 and multiplies both code sets on
the block-scaled MFMA (`ops.gemm_w4a8`); decode-width calls stay
weight-only."""

from __future__ import annotations

import copy
from typing import Optional

import torch
import torch.nn as nn

from acco_amd import ops
from acco_amd.models.fuse import _FUSE_ATTRS


def _check_act_dtype(act_dtype) -> None:
    if act_dtype not in (None, torch.float8_e4m3fn):
        raise ValueError("act_dtype must be None or torch.float8_e4m3fn, got "
                         f"{act_dtype}")


class _QuantLinear(nn.Module):
    """What W8Linear and W4Linear share: the weight as two buffers, `codes`
    and the one `_SCALE` names (as is the optional `bias`), pinned to the
    dtypes `_DTYPES`. A subclass gives those, `_quantize` and `forward`."""

    def __init__(self, codes: torch.Tensor, scale: torch.Tensor,
                 bias: Optional[torch.Tensor] = None):
        super().__init__()
        self.register_buffer("codes", codes)
        self.register_buffer(self._SCALE, scale)
        self.register_buffer("bias", bias)

    @classmethod
    def from_linear(cls, lin: nn.Linear):
        codes, scale = cls._quantize(lin.weight.detach())
        bias = None if lin.bias is None else lin.bias.detach()
        return cls(codes, scale, bias)

    def _apply(self, fn, recurse=True):
        """Moves and casts as any module, but the weight keeps its format: a
        dtype cast of the model (.double(), .to(torch.bfloat16)) reaches the
        bias only. e4m3 -> any wider float -> e4m3 is exact; a floating-point
        cast leaves MXFP4's integer buffers alone, and an explicit cast to
        another integer type is undone here."""
        super()._apply(fn, recurse)
        for name, dtype in zip(("codes", self._SCALE), self._DTYPES):
            setattr(self, name, getattr(self, name).to(dtype))
        return self

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """Routed by the rows of x over `_OPS` = (skinny, tiled, cap): up to
        64 rows ops.`skinny`, more ops.`tiled` up to its measured cap
        ops.`cap` (None: none), past that ops.`skinny` again, whose M > 64
        path dequantises to a temporary."""
        skinny, tiled, cap = self._OPS
        rows, cap = x.numel() // max(x.shape[-1], 1), getattr(ops, cap)
        op = tiled if rows > 64 and (cap is None or rows <= cap) else skinny
        return getattr(ops, op)(x, self.codes, getattr(self, self._SCALE),
                                self.bias)

    def extra_repr(self) -> str:
        return (f"in_features={self.in_features}, out_features="
                f"{self.out_features}, bias={self.bias is not None}")


class W8Linear(_QuantLinear):
    """A linear whose weight is e4m3 `codes` [out, in] and fp32 `scale` [out]
    (buffers, as is the optional `bias`): forward is ops.linear_w8 up to 64
    rows of x and ops.gemm_w8 beyond."""

    _SCALE, _DTYPES = "scale", (torch.float8_e4m3fn, torch.float32)
    _OPS = ("linear_w8", "gemm_w8", "W8_GEMM_MAX_ROWS")
    _quantize = staticmethod(ops.torch_ref.weight_quantize)

    def __init__(self, codes, scale, bias=None):
        super().__init__(codes, scale, bias)
        self.out_features, self.in_features = codes.shape


class W4Linear(_QuantLinear):
    """A linear whose weight is MXFP4: uint8 `codes` [out, in / 2] and uint8
    `scales` [out, in / 32] (buffers, as is the optional `bias`): forward is
    ops.linear_w4 up to 64 rows of x and ops.gemm_w4 beyond. in_features must
    be a multiple of 32.
    act_dtype: None, or torch.float8_e4m3fn: calls of at least
    max(65, ops.W4A8_GEMM_MIN_ROWS) rows (65 when that is None) go to
    ops.gemm_w4a8, which rounds x to MXFP8; fewer rows are routed as without
    it."""

    _SCALE, _DTYPES = "scales", (torch.uint8, torch.uint8)
    _OPS = ("linear_w4", "gemm_w4", "W4_GEMM_MAX_ROWS")
    _quantize = staticmethod(ops.torch_ref.weight_quantize_mxfp4)

    def __init__(self, codes, scales, bias=None, act_dtype=None):
        super().__init__(codes, scales, bias)
        self.out_features, self.in_features = codes.shape[0], 2 * codes.shape[1]
        _check_act_dtype(act_dtype)
        self.act_dtype = act_dtype

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if self.act_dtype is not None:
            rows = x.numel() // max(x.shape[-1], 1)
            if rows >= max(65, ops.W4A8_GEMM_MIN_ROWS or 65):
                return ops.gemm_w4a8(x, self.codes, self.scales, self.bias)
        return super().forward(x)


FP4 = torch.float4_e2m1fn_x2


def _copy_module(mod: nn.Module, dtype: torch.dtype,
                 act_dtype: Optional[torch.dtype] = None) -> nn.Module:
    """A new module tree over the same tensors: nn.Linear -> W8Linear (or
    W4Linear), every other module a shallow copy with its own parameter /
    buffer / child tables, so embeddings and norm weights are shared with the
    original."""
    if isinstance(mod, nn.Linear):
        if dtype != FP4:
            return W8Linear.from_linear(mod)
        # MXFP4 blocks are 32 wide: a linear they do not tile stays as it is
        if mod.in_features % 32 != 0:
            return mod
        new = W4Linear.from_linear(mod)
        new.act_dtype = act_dtype
        return new
    new = copy.copy(mod)
    new._parameters = dict(mod._parameters)
    new._buffers = dict(mod._buffers)
    new._modules = {name: None if child is None
                    else _copy_module(child, dtype, act_dtype)
                    for name, child in mod._modules.items()}
    for attr in _FUSE_ATTRS:
        # arena views of the bf16 weights: the copy takes the per-projection
        # paths, which call the modules
        if getattr(new, attr, None) is not None:
            setattr(new, attr, None)
    return new


@torch.no_grad()
def quantize_weights(model: nn.Module,
                     dtype: torch.dtype = torch.float8_e4m3fn,
                     act_dtype: Optional[torch.dtype] = None) -> nn.Module:
    """A copy of `model` (LlamaForCausalLM or GPTNeoForCausalLM, in eval mode)
    for generation whose every nn.Linear is a W8Linear of the same weight; a
    tied lm_head gets codes of its own and the embedding stays as it is.
    Embeddings and norm weights are the original's tensors, not copies.
    prefill, decode_step, extend and forward work on the result unchanged;
    the original is not modified.
    dtype: torch.float8_e4m3fn (W8Linear) or torch.float4_e2m1fn_x2: MXFP4
    W4Linears, except that a linear whose in_features is not a multiple of 32
    stays the original's bf16 nn.Linear in the copy.
    act_dtype: None, or torch.float8_e4m3fn with the MXFP4 dtype only: every
    W4Linear then sends its calls of 65 rows and more (the prefill, long
    extends) to ops.gemm_w4a8, which rounds the activations to MXFP8;
    decode-width calls stay weight-only. Anything else raises ValueError."""
    _check_act_dtype(act_dtype)
    if act_dtype is not None and dtype != FP4:
        raise ValueError("quantize_weights: act_dtype needs dtype="
                         f"torch.float4_e2m1fn_x2, got {dtype}")
    if model.training:
        raise ValueError("quantize_weights is for generation: call "
                         "model.eval() first")
    if dtype not in (torch.float8_e4m3fn, FP4):
        raise ValueError("quantize_weights: dtype must be torch.float8_e4m3fn "
                         f"or torch.float4_e2m1fn_x2, got {dtype}")
    return _copy_module(model, dtype, act_dtype).eval()


def has_quantized_linears(model: nn.Module) -> bool:
    return any(isinstance(m, (W8Linear, W4Linear)) for m in model.modules())
