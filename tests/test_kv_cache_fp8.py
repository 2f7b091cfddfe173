"""The e4m3 KV cache on the CPU: the quantiser that defines the format
(torch_ref.kv_quantize / kv_dequantize), the reference ops on an fp8 cache,
KVCache.allocate and generate(kv_dtype=...)."""

import pytest
import torch

from acco_amd import ops
from acco_amd.models import (GPTNeoConfig, GPTNeoForCausalLM, LlamaConfig,
                             LlamaForCausalLM, generate)
from acco_amd.models.kv_cache import KVCache
from acco_amd.ops import torch_ref

FP8 = torch.float8_e4m3fn


def _rows(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).bfloat16()


def test_quantiser_properties():
    x = _rows(5, 3, 64) * torch.logspace(-6, 3, 15).view(5, 3, 1).bfloat16()
    x[2, 1] = 0
    codes, scale = torch_ref.kv_quantize(x)
    assert codes.dtype == FP8 and scale.dtype == torch.float32
    amax = x.float().abs().amax(-1)
    inv = torch.where(amax > 0, 448.0 / amax.double(), 0.0).float()
    y, c = x.float() * inv[..., None], codes.float()
    # half a step of e4m3 at y: 3 mantissa bits, smallest normal 2^-6
    half = torch.exp2(torch.floor(torch.log2(y.abs().clamp(min=2.0 ** -6)))
                      - 4)
    assert bool(((c - y).abs() <= half).all())
    live = amax > 0
    assert bool((c.abs().amax(-1)[live] == 448).all())
    top = x.float().abs().argmax(-1, keepdim=True)
    assert torch.equal(c.gather(-1, top)[live], 448 * x.float().gather(
        -1, top).sign()[live])
    assert float(scale[2, 1]) == 0 and bool((c[2, 1] == 0).all())
    assert torch.equal(torch_ref.kv_dequantize(codes, scale),
                       c * scale[..., None])


def _fp8_case():
    B, Hkv, Smax, D, H, T = 2, 2, 24, 32, 4, 3
    kc, ks = torch_ref.kv_quantize(_rows(B, Hkv, Smax, D, seed=1))
    vc, vs = torch_ref.kv_quantize(_rows(B, Hkv, Smax, D, seed=2))
    q = _rows(B, T, H, D, seed=3).float()
    return q, kc, vc, ks, vs, torch.tensor([5, 20], dtype=torch.int32)


@pytest.mark.parametrize("window", [None, 4])
def test_reference_ops_on_an_fp8_cache(window):
    q, kc, vc, ks, vs, cl = _fp8_case()
    kd, vd = (torch_ref.kv_dequantize(c, s) for c, s in ((kc, ks), (vc, vs)))
    sc = dict(k_scale=ks, v_scale=vs)
    assert torch.equal(
        ops.decode_attention(q[:, 0], kc, vc, cl, window=window, **sc),
        ops.decode_attention(q[:, 0], kd, vd, cl, window=window))
    assert torch.equal(
        ops.extend_attention(q, kc, vc, cl, window=window, **sc),
        ops.extend_attention(q, kd, vd, cl, window=window))
    # append: the rows the bf16 append stores, quantised; the rest untouched
    k, v = _rows(2, 3, 2, 32, seed=4), _rows(2, 3, 2, 32, seed=5)
    kb, vb = kd.bfloat16(), vd.bfloat16()
    ops.kv_append(kb, vb, cl, k, v)
    want = {n: (c.clone(), s.clone()) for n, c, s in (("k", kc, ks),
                                                      ("v", vc, vs))}
    for b, L in enumerate(cl.tolist()):
        for n, new in (("k", kb), ("v", vb)):
            c, s = torch_ref.kv_quantize(new[b, :, L:L + 3])
            want[n][0][b, :, L:L + 3] = c
            want[n][1][b, :, L:L + 3] = s
    ops.kv_append(kc, vc, cl, k, v, **sc)
    for got, (c, s) in (((kc, ks), want["k"]), ((vc, vs), want["v"])):
        assert torch.equal(got[0].view(torch.uint8), c.view(torch.uint8))
        assert torch.equal(got[1], s)


def test_mismatched_cache_and_scales_raise():
    q, kc, vc, ks, vs, cl = _fp8_case()
    k = _rows(2, 3, 2, 32).float()
    for caches, sc in (((kc, vc), {}), ((kc, vc), dict(k_scale=ks)),
                       ((kc.float(), vc.float()),
                        dict(k_scale=ks, v_scale=vs))):
        with pytest.raises(ValueError, match="k_scale and v_scale"):
            ops.kv_append(*caches, cl, k, k, **sc)
        with pytest.raises(ValueError, match="k_scale and v_scale"):
            ops.decode_attention(q[:, 0], *caches, cl, **sc)
        with pytest.raises(ValueError, match="k_scale and v_scale"):
            ops.extend_attention(q, *caches, cl, **sc)


@pytest.mark.parametrize("family", ["llama", "gptneo"])
def test_allocate_and_generate_with_an_fp8_cache(family):
    torch.manual_seed(0)
    kw = dict(hidden_size=64, num_layers=2, num_heads=4, vocab_size=96,
              max_position_embeddings=64)
    model = (LlamaForCausalLM(LlamaConfig(num_kv_heads=2,
                                          intermediate_size=128, **kw))
             if family == "llama"
             else GPTNeoForCausalLM(GPTNeoConfig(window_size=8, **kw))).eval()
    hkv = 2 if family == "llama" else 4
    cache = KVCache.allocate(model, 3, 40, dtype=FP8)
    for c, s in zip(cache.k + cache.v, cache.k_scale + cache.v_scale):
        assert c.shape == (3, hkv, 40, 16) and c.dtype == FP8
        assert s.shape == (3, hkv, 40) and s.dtype == torch.float32
    assert len(cache.k_scale) == len(cache.v_scale) == 2
    plain = KVCache.allocate(model, 3, 40)
    assert plain.k_scale is None and plain.v_scale is None
    ids = torch.randint(0, 96, (3, 9))
    lens = torch.tensor([9, 4, 1])
    tokens, n = generate(model, ids, lens, max_new=6, temperature=0.0,
                         kv_dtype=FP8, eos_token_id=None)
    assert tokens.shape == (3, 15) and n.shape == (3,)
    assert bool(((tokens >= 0) & (tokens < 96)).all())
