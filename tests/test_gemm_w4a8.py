"""The W4A8 semantics on the CPU: torch_ref.act_quantize_mxfp8 on hand-made
blocks, its round trip, torch_ref.linear_w4a8 against an fp64 product written
out here, and the act_dtype option of quantize_weights / W4Linear. Also home
of the inputs tests/test_gpu_gemm_w4a8.py shares (hand_blocks, every_act_code),
checked here before the GPU sees them."""

import pytest
import torch
import torch.nn as nn

from acco_amd import ops
from acco_amd.models import W4Linear, quantize_weights
from acco_amd.ops import torch_ref as R

FP8, FP4 = torch.float8_e4m3fn, torch.float4_e2m1fn_x2


def hand_blocks():
    """(x bf16 [6, 32], scale bytes [6], (row, col, code value) spot checks):
    a zero block; amax an exact power of two (8 = 256 * 2^-5); 480 = 1.875 *
    2^8 in (448, 512), which clips; 17 and 19 under amax 256, ties between
    e4m3 neighbours 16 | 18 and 18 | 20, to the even significand; 2^-115,
    below the clamp of e at -120; the largest finite bf16, e = 119 (finite
    input cannot reach the clamp at 120)."""
    x = torch.zeros(6, 32)
    x[1, :3] = torch.tensor([8.0, -3.0, 0.015625])
    x[2, :2] = torch.tensor([480.0, -300.0])
    x[3, :4] = torch.tensor([256.0, 17.0, -19.0, 21.0])
    x[4, :2] = torch.tensor([2.0 ** -115, -2.0 ** -117])
    x[5, :2] = torch.tensor([2.0 ** 127 * 1.9921875, 2.0 ** 119])
    spots = [(1, 0, 256.0), (1, 1, -96.0), (1, 2, 0.5), (2, 0, 448.0),
             (2, 1, -288.0), (3, 1, 16.0), (3, 2, -20.0), (3, 3, 20.0),
             (4, 0, 32.0), (4, 1, -8.0), (5, 0, 448.0), (5, 1, 1.0)]
    return x.bfloat16(), [127, 122, 127, 127, 7, 246], spots


def every_act_code(M=512, K=512):
    """x bf16 [M, K] = every finite e4m3 code in every k slot (the two NaN
    codes as 0) times block scales 2^(s - 127), s in [20, 219]; one slot of
    every block holds a code of exponent 8, so the quantiser finds s again."""
    m, k = torch.arange(M)[:, None], torch.arange(K)[None, :]
    c = (m + 5 * k) % 256
    c = torch.where(c % 128 == 127, torch.zeros_like(c), c)
    top = 0x78 + (m + k // 32) % 7 + 128 * (m % 2)
    c = torch.where(k % 32 == m % 32, top, c).to(torch.uint8)
    s = (20 + (7 * (k[:, ::32] // 32) + 3 * m) % 200).to(torch.uint8)
    return R.act_dequantize_mxfp8(c.view(FP8), s, torch.bfloat16), c, s


def test_act_quantize_hand_blocks():
    x, want_s, spots = hand_blocks()
    codes, scales = R.act_quantize_mxfp8(x)
    assert codes.dtype == FP8 and scales.dtype == torch.uint8
    assert scales.flatten().tolist() == want_s
    assert torch.equal(codes[0].view(torch.uint8), torch.zeros(32).byte())
    for r, c, v in spots:
        assert float(codes[r, c]) == v, (r, c, float(codes[r, c]), v)
    with pytest.raises(ValueError):
        R.act_quantize_mxfp8(torch.zeros(2, 48))


def test_act_round_trip():
    """dequant(quantise(x)) == x, codes and scales recovered, for x made of
    e4m3 values times a block scale."""
    x, c, s = every_act_code()
    codes, scales = R.act_quantize_mxfp8(x)
    assert torch.equal(scales, s)
    assert torch.equal(codes.view(torch.uint8), c)
    assert torch.equal(R.act_dequantize_mxfp8(codes, scales, torch.bfloat16), x)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float64])
def test_linear_w4a8_reference(dtype):
    g = torch.Generator().manual_seed(11)
    x = (torch.randn(5, 3, 64, generator=g) * 7).to(dtype)
    codes, scales = R.weight_quantize_mxfp4(torch.randn(9, 64, generator=g))
    bias = torch.randn(9, generator=g).to(dtype)
    xc, xs = R.act_quantize_mxfp8(x)
    xd = (xc.double().reshape(5, 3, 2, 32)
          * torch.exp2(xs.double() - 127)[..., None]).reshape(5, 3, 64)
    # half a step of 32 below 448 * 2^e, up to 64 of 512 where a value clips
    assert (xd - x.double()).abs().max() <= 2.0 ** -3 * x.double().abs().max()
    f = xd @ R.weight_dequantize_mxfp4(codes, scales, torch.float64).t() \
        + bias.double()
    y = R.linear_w4a8(x, codes, scales, bias)
    assert y.dtype == dtype and y.shape == (5, 3, 9)
    tol = 2.0 ** -8 if dtype == torch.bfloat16 else 1e-12
    assert (y.double() - f).abs().max() <= tol * f.abs().max()


def test_quantize_weights_act_dtype(monkeypatch):
    model = nn.Sequential(nn.Linear(128, 16)).eval()
    for bad in (dict(dtype=FP4, act_dtype=torch.bfloat16),
                dict(dtype=FP4, act_dtype=FP4),
                dict(dtype=FP8, act_dtype=FP8)):
        with pytest.raises(ValueError):
            quantize_weights(model, **bad)
    assert quantize_weights(model, FP4)[0].act_dtype is None
    lin = quantize_weights(model, FP4, act_dtype=FP8)[0]
    assert isinstance(lin, W4Linear) and lin.act_dtype == FP8
    assert ops.W4A8_GEMM_MIN_ROWS is None or ops.W4A8_GEMM_MIN_ROWS >= 65
    monkeypatch.setattr(ops, "W4A8_GEMM_MIN_ROWS", 65)
    x = torch.randn(13, 5, 128, generator=torch.Generator().manual_seed(3))
    x = (x * 5).bfloat16()
    a8 = R.linear_w4a8(x, lin.codes, lin.scales, lin.bias)
    assert torch.equal(lin(x), a8)
    assert not torch.equal(a8, R.linear_w4(x, lin.codes, lin.scales, lin.bias))
    x64 = x.flatten(0, 1)[:64]
    assert torch.equal(lin(x64), R.linear_w4(x64, lin.codes, lin.scales,
                                             lin.bias))
