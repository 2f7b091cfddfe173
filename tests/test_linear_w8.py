"""FP8 weight-only linears on the CPU: the weight format
(torch_ref.weight_quantize), the reference product (torch_ref.linear_w8),
models.quantize_weights and generate(weight_dtype=...)."""

import pytest
import torch
import torch.nn as nn

from acco_amd.models import (GPTNeoConfig, GPTNeoForCausalLM, LlamaConfig,
                             LlamaForCausalLM, W8Linear, generate,
                             quantize_weights)
from acco_amd.ops import torch_ref

FP8 = torch.float8_e4m3fn


def _tiny(family, tie=False):
    torch.manual_seed(0)
    kw = dict(hidden_size=64, num_layers=2, num_heads=4, vocab_size=96,
              max_position_embeddings=64, tie_word_embeddings=tie)
    if family == "llama":
        return LlamaForCausalLM(LlamaConfig(num_kv_heads=2,
                                            intermediate_size=128, **kw)).eval()
    return GPTNeoForCausalLM(GPTNeoConfig(window_size=8, **kw)).eval()


def test_weight_quantize_is_kv_quantize_of_the_rows():
    g = torch.Generator().manual_seed(0)
    w = (torch.randn(7, 64, generator=g)
         * torch.logspace(-4, 2, 7)[:, None]).bfloat16()
    w[3] = 0
    codes, scale = torch_ref.weight_quantize(w)
    assert codes.shape == (7, 64) and codes.dtype == FP8
    assert scale.shape == (7,) and scale.dtype == torch.float32
    for i in range(7):
        c, s = torch_ref.kv_quantize(w[i])
        assert torch.equal(codes[i].view(torch.uint8), c.view(torch.uint8))
        assert torch.equal(scale[i], s)


@pytest.mark.parametrize("bias", [False, True])
def test_reference_product_against_fp64(bias):
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 5, 128, generator=g).bfloat16()
    codes, scale = torch_ref.weight_quantize(torch.randn(33, 128, generator=g))
    b = torch.randn(33, generator=g).bfloat16() if bias else None
    y = torch_ref.linear_w8(x, codes, scale, b)
    assert y.shape == (2, 5, 33) and y.dtype == torch.bfloat16
    w64 = codes.double() * scale.double()[:, None]
    f = x.double() @ w64.t() + (b.double() if bias else 0.0)
    mag = x.double().abs() @ w64.abs().t()
    assert bool(((y.double() - f).abs()
                 <= 2.0 ** -8 * f.abs() + 130 * 2.0 ** -24 * mag).all())


@pytest.mark.parametrize("family,tie", [("llama", False), ("llama", True),
                                        ("gptneo", True)])
def test_quantize_weights(family, tie):
    model = _tiny(family, tie)
    q = quantize_weights(model)
    assert not q.training and q is not model
    lins = dict((n, m) for n, m in model.named_modules()
                if isinstance(m, nn.Linear))
    assert lins and not any(isinstance(m, nn.Linear) for m in q.modules())
    qmods = dict(q.named_modules())
    for name, lin in lins.items():
        w8 = qmods[name]
        assert isinstance(w8, W8Linear)
        assert (w8.out_features, w8.in_features) == tuple(lin.weight.shape)
        codes, scale = torch_ref.weight_quantize(lin.weight)
        assert torch.equal(w8.codes.view(torch.uint8), codes.view(torch.uint8))
        assert torch.equal(w8.scale, scale)
        assert (w8.bias is None) == (lin.bias is None)
    shared = dict(model.named_parameters())
    kept = dict(q.named_parameters())
    assert kept and all(p is shared[n] for n, p in kept.items())
    assert all(n in kept for n in shared
               if "norm" in n or "ln_" in n or "embed" in n or "wte" in n
               or "wpe" in n)
    assert isinstance(model.lm_head, nn.Linear)       # the original: intact
    if tie:
        emb = (model.model.embed_tokens if family == "llama"
               else model.transformer.wte)
        assert model.lm_head.weight is emb.weight
        assert q.lm_head.codes.dtype == FP8
    ids = torch.randint(0, 96, (2, 9))
    assert q(ids)[0].shape == (2, 9, 96)
    assert q.double().lm_head.codes.dtype == FP8
    with pytest.raises(ValueError, match="eval"):
        quantize_weights(model.train())


@pytest.mark.parametrize("family", ["llama", "gptneo"])
def test_generate_weight_dtype(family):
    model = _tiny(family)
    ids = torch.randint(0, 96, (3, 9))
    lens = torch.tensor([9, 4, 1])
    kw = dict(max_new=6, temperature=0.0, eos_token_id=None)
    base, _ = generate(model, ids, lens, **kw)
    none, _ = generate(model, ids, lens, weight_dtype=None, **kw)
    assert torch.equal(base, none)
    pre, _ = generate(quantize_weights(model), ids, lens, **kw)
    got, n = generate(model, ids, lens, weight_dtype=FP8, **kw)
    assert torch.equal(got, pre) and got.shape == (3, 15) and n.shape == (3,)
    again, _ = generate(quantize_weights(model), ids, lens, weight_dtype=FP8,
                        **kw)
    assert torch.equal(again, pre)
    with pytest.raises(ValueError, match="weight_dtype"):
        generate(model, ids, lens, weight_dtype=torch.int8, **kw)
