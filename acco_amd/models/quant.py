"""FP8 (e4m3) weight-only linears for generation: every projection of a model
stored as one-byte codes with one fp32 scale per output row
(torch_ref.weight_quantize), half the weight bytes a decode step streams and
half the weight memory of a model that is only generated from. Activations
stay bf16; `ops.linear_w8` is the product. Nothing here trains."""

from __future__ import annotations

import copy
from typing import Optional

import torch
import torch.nn as nn

from acco_amd import ops
from acco_amd.models.fuse import _FUSE_ATTRS


class W8Linear(nn.Module):
    """A linear whose weight is e4m3 `codes` [out, in] and fp32 `scale` [out]
    (buffers, as is the optional `bias`): forward is ops.linear_w8."""

    def __init__(self, codes: torch.Tensor, scale: torch.Tensor,
                 bias: Optional[torch.Tensor] = None):
        super().__init__()
        self.out_features, self.in_features = codes.shape
        self.register_buffer("codes", codes)
        self.register_buffer("scale", scale)
        self.register_buffer("bias", bias)

    @classmethod
    def from_linear(cls, lin: nn.Linear) -> "W8Linear":
        codes, scale = ops.torch_ref.weight_quantize(lin.weight.detach())
        bias = None if lin.bias is None else lin.bias.detach()
        return cls(codes, scale, bias)

    def _apply(self, fn, recurse=True):
        """Moves and casts as any module, but the weight keeps its format: a
        dtype cast of the model (.double(), .to(torch.bfloat16)) reaches the
        bias only. e4m3 -> any wider float -> e4m3 is exact."""
        super()._apply(fn, recurse)
        self.codes = self.codes.to(torch.float8_e4m3fn)
        self.scale = self.scale.to(torch.float32)
        return self

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return ops.linear_w8(x, self.codes, self.scale, self.bias)

    def extra_repr(self) -> str:
        return (f"in_features={self.in_features}, out_features="
                f"{self.out_features}, bias={self.bias is not None}")


def _copy_module(mod: nn.Module) -> nn.Module:
    """A new module tree over the same tensors: nn.Linear -> W8Linear, every
    other module a shallow copy with its own parameter / buffer / child
    tables, so embeddings and norm weights are shared with the original."""
    if isinstance(mod, nn.Linear):
        return W8Linear.from_linear(mod)
    new = copy.copy(mod)
    new._parameters = dict(mod._parameters)
    new._buffers = dict(mod._buffers)
    new._modules = {name: None if child is None else _copy_module(child)
                    for name, child in mod._modules.items()}
    for attr in _FUSE_ATTRS:
        # arena views of the bf16 weights: the copy takes the per-projection
        # paths, which call the modules
        if getattr(new, attr, None) is not None:
            setattr(new, attr, None)
    return new


@torch.no_grad()
def quantize_weights(model: nn.Module) -> nn.Module:
    """A copy of `model` (LlamaForCausalLM or GPTNeoForCausalLM, in eval mode)
    for generation whose every nn.Linear is a W8Linear of the same weight; a
    tied lm_head gets codes of its own and the embedding stays as it is.
    Embeddings and norm weights are the original's tensors, not copies.
    prefill, decode_step, extend and forward work on the result unchanged;
    the original is not modified."""
    if model.training:
        raise ValueError("quantize_weights is for generation: call "
                         "model.eval() first")
    return _copy_module(model).eval()


def has_w8_linears(model: nn.Module) -> bool:
    return any(isinstance(m, W8Linear) for m in model.modules())
