"""ops.gemm_w8 / ops.gemm_w4 on the CPU are the torch reference, and the
modules' routing by row count changes nothing there."""

import pytest
import torch

from acco_amd import ops
from acco_amd.models import W4Linear, W8Linear
from acco_amd.ops import torch_ref


@pytest.mark.parametrize("fmt,cls,quantize", [
    ("w8", W8Linear, torch_ref.weight_quantize),
    ("w4", W4Linear, torch_ref.weight_quantize_mxfp4)])
def test_cpu_is_the_reference(fmt, cls, quantize):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(5, 13, 128, generator=g).bfloat16()         # 65 rows
    weight = quantize(torch.randn(33, 128, generator=g))
    bias = torch.randn(33, generator=g).bfloat16()
    want = getattr(torch_ref, "linear_" + fmt)(x, *weight, bias)
    assert torch.equal(getattr(ops, "gemm_" + fmt)(x, *weight, bias), want)
    assert torch.equal(cls(*weight, bias)(x), want)
    assert getattr(ops, "gemm_" + fmt)(x[:0], *weight).shape == (0, 13, 33)
