"""MXFP4 weight-only linears on the CPU: the weight format
(torch_ref.weight_quantize_mxfp4), the reference product
(torch_ref.linear_w4), models.quantize_weights(dtype=fp4) and
generate(weight_dtype=fp4)."""

import pytest
import torch
import torch.nn as nn

from acco_amd.models import W4Linear, generate, quantize_weights
from acco_amd.ops import torch_ref
from tests.test_linear_w8 import _tiny

FP4 = torch.float4_e2m1fn_x2
MAGS = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]


def test_quantizer_scale_rule_and_every_code():
    """Row i is every code times 2^p twice over (so amax = 6 * 2^p and the
    rule gives e = p, clamped into [-120, 120]), then a zero block."""
    exps = [-130, -122, -120, -3, 0, 7, 118, 125]
    vals = torch.tensor(MAGS + [-m for m in MAGS]).repeat(2)
    w = torch.stack([torch.cat([
        torch.ldexp(vals.double(), torch.tensor(p)).float(), torch.zeros(32)])
        for p in exps])
    codes, scales = torch_ref.weight_quantize_mxfp4(w)
    assert codes.shape == (8, 32) and codes.dtype == torch.uint8
    assert scales.shape == (8, 2) and scales.dtype == torch.uint8
    want_e = [max(-120, min(120, p)) for p in exps]
    assert scales[:, 0].tolist() == [e + 127 for e in want_e]
    assert scales[:, 1].tolist() == [127] * 8 and not codes[:, 16:].any()
    deq = torch_ref.weight_dequantize_mxfp4(codes, scales, torch.bfloat16)
    for i, p in enumerate(exps):
        if -120 <= p <= 120:        # representable: reproduced exactly
            assert torch.equal(deq[i].float(), w[i]), p
    # every nibble times every scale in range comes back exactly
    allc = (torch.arange(16) | ((15 - torch.arange(16)) << 4)).to(torch.uint8)
    allc = allc.repeat(2)[None].repeat(3, 1)                    # [3, 32]
    sc = torch.tensor([[7, 247], [127, 100], [200, 8]], dtype=torch.uint8)
    deq = torch_ref.weight_dequantize_mxfp4(allc, sc, torch.bfloat16).double()
    signed = torch.tensor(MAGS + [-m for m in MAGS], dtype=torch.float64)
    nib = torch.stack((allc & 15, allc >> 4), -1).reshape(3, 64).long()
    want = signed[nib] * torch.exp2(sc.double() - 127).repeat_interleave(32, 1)
    assert torch.equal(deq, want)
    # ties go to the even code, (6, 8) clips, and the block's own amax rules
    row = torch.zeros(1, 32)
    row[0, :8] = torch.tensor([7.9, 0.25, 0.75, 1.25, 2.5, 5.0, -7.0, -0.25])
    c, s = torch_ref.weight_quantize_mxfp4(row)
    got = torch_ref.weight_dequantize_mxfp4(c, s, torch.float32)[0, :8]
    assert s.item() == 127 and got.tolist() == [6, 0, 1, 1, 2, 4, -6, 0]
    with pytest.raises(ValueError):
        torch_ref.weight_quantize_mxfp4(torch.zeros(2, 48))


@pytest.mark.parametrize("bias", [False, True])
def test_reference_product_against_fp64(bias):
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 5, 128, generator=g).bfloat16()
    codes, scales = torch_ref.weight_quantize_mxfp4(
        torch.randn(33, 128, generator=g))
    b = torch.randn(33, generator=g).bfloat16() if bias else None
    y = torch_ref.linear_w4(x, codes, scales, b)
    assert y.shape == (2, 5, 33) and y.dtype == torch.bfloat16
    w64 = torch_ref.weight_dequantize_mxfp4(codes, scales, torch.float64)
    f = x.double() @ w64.t() + (b.double() if bias else 0.0)
    mag = x.double().abs() @ w64.abs().t()
    assert bool(((y.double() - f).abs()
                 <= 2.0 ** -8 * f.abs() + 130 * 2.0 ** -24 * mag).all())


@pytest.mark.parametrize("family,tie", [("llama", False), ("llama", True),
                                        ("gptneo", True)])
def test_quantize_weights_fp4(family, tie):
    model = _tiny(family, tie)
    q = quantize_weights(model, dtype=FP4)
    assert not q.training and q is not model
    lins = dict((n, m) for n, m in model.named_modules()
                if isinstance(m, nn.Linear))
    assert lins and not any(isinstance(m, nn.Linear) for m in q.modules())
    qmods = dict(q.named_modules())
    for name, lin in lins.items():
        w4 = qmods[name]
        assert isinstance(w4, W4Linear)
        assert (w4.out_features, w4.in_features) == tuple(lin.weight.shape)
        codes, scales = torch_ref.weight_quantize_mxfp4(lin.weight)
        assert torch.equal(w4.codes, codes) and torch.equal(w4.scales, scales)
        assert (w4.bias is None) == (lin.bias is None)
    shared = dict(model.named_parameters())
    kept = dict(q.named_parameters())
    assert kept and all(p is shared[n] for n, p in kept.items())
    assert all(n in kept for n in shared
               if "norm" in n or "ln_" in n or "embed" in n or "wte" in n
               or "wpe" in n)
    assert isinstance(model.lm_head, nn.Linear)       # the original: intact
    ids = torch.randint(0, 96, (2, 9))
    assert q(ids)[0].shape == (2, 9, 96)
    q = q.double()
    assert q.lm_head.codes.dtype == q.lm_head.scales.dtype == torch.uint8
    with pytest.raises(ValueError, match="dtype"):
        quantize_weights(model, dtype=torch.int8)


@pytest.mark.parametrize("family", ["llama", "gptneo"])
def test_generate_weight_dtype_fp4(family):
    model = _tiny(family)
    ids = torch.randint(0, 96, (3, 9))
    lens = torch.tensor([9, 4, 1])
    kw = dict(max_new=6, temperature=0.0, eos_token_id=None)
    pre, _ = generate(quantize_weights(model, dtype=FP4), ids, lens, **kw)
    got, n = generate(model, ids, lens, weight_dtype=FP4, **kw)
    assert torch.equal(got, pre) and got.shape == (3, 15) and n.shape == (3,)
    again, _ = generate(quantize_weights(model, dtype=FP4), ids, lens,
                        weight_dtype=FP4, **kw)
    assert torch.equal(again, pre)
