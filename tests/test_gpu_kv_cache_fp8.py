"""The e4m3 KV cache on the GPU: acco_kv_append_fp8 bit for bit against
torch_ref.kv_quantize of the rows the bf16 append stores, acco_attn_decode_fp8
and acco_attn_extend_fp8 against an fp64 reference of double(code) *
double(scale) under the criterion of the bf16 kernels (quantisation is an
input, not an error), and prefill / decode_step / extend of both families on
an fp8 cache. MEASURED: RESULTS.md, "FP8 KV cache"."""

import copy
import math

import pytest
import torch

from acco_amd import ops
from acco_amd.models.kv_cache import KVCache
from acco_amd.ops.torch_ref import kv_quantize
from tests import attention_ref as AR
from tests import test_gpu_decode_attention as TD
from tests import test_gpu_extend_attention as TE
from tests.kv_cache_ref import teacher_forced

pytestmark = pytest.mark.gpu
DEV, FP8 = "cuda", torch.float8_e4m3fn


def _u8(t):
    return t.contiguous().view(torch.uint8)


def quantised(c):
    """(codes, scales, fp64 values) of a bf16 cache; its NaN rows (the rows no
    query may see) get NaN codes 0x7F and NaN scales."""
    dead = c[..., 0].isnan()
    codes, scale = (t.to(DEV) for t in kv_quantize(c.nan_to_num(0.0).cpu()))
    _u8(codes)[dead] = 0x7F
    scale[dead] = math.nan
    return codes, scale, codes.float().double() * scale.double()[..., None]


def check(kind, name, lens, T, rep, D, Smax, window=0, scale=None, Hkv=2,
          run=None):
    """Run an fp8 kernel and hold o to the criterion of the bf16 one."""
    scale = D ** -0.5 if scale is None else scale
    if kind == "decode":
        q, kc, vc, cl = TD.make_decode(name, lens, Hkv, rep, D, Smax)
    else:
        q, kc, vc, cl = TE.make_extend(name, lens, T, rep, D, Smax, Hkv)
    (kq, ks, k64), (vq, vs, v64) = quantised(kc), quantised(vc)
    run = run or getattr(ops.hip_ext(), "attn_%s_fp8" % kind)
    o = run(q, kq, vq, ks, vs, cl, scale, window)
    assert o.shape == q.shape and o.dtype == torch.bfloat16
    assert not torch.isnan(o.float()).any(), name
    if kind == "decode":
        f = TD.decode_ref64(q, k64, v64, cl, scale, window)
    else:
        f = TE.extend_ref64(q, k64, v64, cl, scale, window)
    floor = AR.floor_of(AR.fwd_floor_terms(f), "o", f["o"],
                        mult=AR.KERNEL_FLOOR)
    ratio, idx = AR.within(o.view(f["o"].shape), f["o"], floor)
    print("RATIO attn_%s_fp8 D%d rep%d %s lens=%s T=%d Smax=%d w=%d s=%g: "
          "%.4f" % (kind, D, rep, name, list(lens), T, Smax, window, scale,
                    ratio))
    assert ratio <= 1.0, (name, ratio, idx)
    for b, L in enumerate(lens):
        dead = o[b] if kind == "decode" else o[b, max(0, min(T, Smax - L)):]
        if kind == "extend" or L <= 0:
            assert bool((TD._bits(dead) == 0).all()), "no key: o = +0"
    again = run(q, kq, vq, ks, vs, cl, scale, window)
    assert torch.equal(TD._bits(o), TD._bits(again)), "same bits on every run"


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("order", ["qkv", "kvq"])
@pytest.mark.parametrize("T,lens", TD.APPEND_CASES)
def test_kv_append_fp8_bit_for_bit(D, order, T, lens):
    Hkv, rep, Smax, B = 2, 2, TD.APPEND_SMAX, 2
    g = AR.case_generator("kv_append_fp8_%d_%s_%d_%s" % (D, order, T, lens))
    src, _, q, k, v = TD._packed(order, T, Hkv, rep, D, g)
    src0 = src.clone()
    cl = torch.tensor(lens, dtype=torch.int32, device=DEV)
    rows = torch.arange(Smax, device=DEV)[None]
    new = ((rows >= cl[:, None]) & (rows < cl[:, None] + T))[:, None]
    for tables in (AR.rope_tables(Smax, D, DEV), (None, None)):
        rot = tables[0] is not None
        kb, vb = TD._sentinel_caches(B, Hkv, Smax, D, g)
        q_bf = ops.kv_append(kb, vb, cl, k, v, q if rot else None, *tables)
        caches = [torch.randint(0, 256, (B, Hkv, Smax, D), generator=g,
                                dtype=torch.uint8).to(DEV) for _ in "kv"]
        scales = [torch.randn(B, Hkv, Smax, generator=g).to(DEV) for _ in "kv"]
        c0, s0 = [c.clone() for c in caches], [s.clone() for s in scales]
        q_rot = ops.kv_append(caches[0].view(FP8), caches[1].view(FP8), cl, k,
                              v, q if rot else None, *tables,
                              k_scale=scales[0], v_scale=scales[1])
        for i, bf in enumerate((kb, vb)):
            codes, scale = (t.to(DEV) for t in kv_quantize(bf.cpu()))
            assert torch.equal(caches[i], torch.where(new[..., None],
                                                      _u8(codes), c0[i]))
            assert torch.equal(scales[i].view(torch.int32), torch.where(
                new, scale, s0[i]).view(torch.int32))
        assert (q_rot is None and q_bf is None) or torch.equal(
            TD._bits(q_rot), TD._bits(q_bf))
    assert torch.equal(TD._bits(src), TD._bits(src0))
    assert cl.tolist() == list(lens)


@pytest.mark.parametrize("D,rep", [(64, 1), (64, 4), (128, 2), (128, 8)])
def test_dequantisation_of_every_code(D, rep):
    """window 1 and a power-of-two scale: o is the dequantised V row, exact
    in bf16, through decode and through extend with T = 1. o is a sum that
    starts from +0, so the code -0 comes out as +0 (0 + -0), as it does in
    the bf16 kernels; every other code keeps its bits."""
    n = 256 // D                                   # rows that hold the codes
    codes = torch.arange(256, dtype=torch.uint8)
    codes[codes % 128 == 127] = 0                  # the two NaN codes
    g = AR.case_generator("all_codes")
    vq = torch.zeros(n, 1, 8, D, dtype=torch.uint8)
    vq[:, 0, :n] = codes.view(n, D)
    vs = torch.exp2(-torch.arange(8.0)).expand(n, 1, 8).contiguous().to(DEV)
    kq, ks = (t.to(DEV) for t in kv_quantize(
        torch.randn(n, 1, 8, D, generator=g).bfloat16()))
    vq = vq.to(DEV).view(FP8)
    q = torch.randn(n, rep, D, generator=g).bfloat16().to(DEV)
    L = torch.arange(1, n + 1, dtype=torch.int32, device=DEV)
    want = (vq.float() * vs[..., None])[torch.arange(n), 0, L.long() - 1]
    want = (want + 0.0).bfloat16()[:, None].expand(n, rep, D)
    sc = dict(k_scale=ks, v_scale=vs)
    o = ops.decode_attention(q, kq, vq, L, window=1, **sc)
    assert torch.equal(TD._bits(o), TD._bits(want))
    o = ops.extend_attention(q[:, None], kq, vq, L - 1, window=1, **sc)
    assert torch.equal(TD._bits(o[:, 0]), TD._bits(want))


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("rep", [1, 4, 8])
def test_attn_decode_fp8(D, rep):
    for lens in TD.LENS:
        check("decode", "len", lens, 1, rep, D, TD.SMAX)
    for window in (1, 300, TD.SMAX + 1):
        check("decode", "win", (700, TD.SMAX), 1, rep, D, TD.SMAX, window)
    check("decode", "scale1", (700, TD.SMAX), 1, rep, D, TD.SMAX, scale=1.0)


def test_attn_decode_fp8_other_grids():
    check("decode", "odd", (193, 300), 1, 3, 64, 300, Hkv=1)
    check("decode", "long", (4096,), 1, 8, 128, 4096, Hkv=1)   # 16 splits


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("rep", range(1, 9))
def test_attn_decode_fp8_every_group_size(D, rep):
    """The twin of TD.test_attn_decode_every_group_size."""
    check("decode", "odd", (193, 300), 1, rep, D, 300, Hkv=1)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("c", TE.CASES, ids=lambda c: "-".join(
    "%s%d" % kv for kv in c.items()))
def test_attn_extend_fp8_sweep(D, c):
    Smax, T = c["Smax"], c["T"]
    L0 = [(0, 0), (1, 63), (64, 65), (Smax - T, 0), (Smax - T + 3, 7)][c["L0"]]
    window = Smax + 1 if c["window"] < 0 else c["window"]
    check("extend", "sweep", L0, T, c["rep"], D, Smax, window)


def test_attn_extend_fp8_splits():
    for L0 in ((251, 255), (256, 257), (1019, 0)):   # 4 splits of 256 keys
        check("extend", "split", L0, 5, 4, 64, 1024, Hkv=1)
    check("extend", "split", (250, 600), 5, 4, 128, 1024, window=300, Hkv=1)
    check("extend", "direct", (195, 64), 65, 4, 64, 200, window=70)  # 1 split


def test_fp8_ops_dispatch_to_hip(monkeypatch):
    spy = TD._Spy(ops.hip_ext())
    monkeypatch.setattr(ops, "hip_ext", lambda: spy)

    def boom(*a, **k):
        raise AssertionError("torch reference reached inside the contract")
    for name in ("kv_append", "decode_attention", "extend_attention"):
        monkeypatch.setattr(ops.torch_ref, name, boom)

    def op(fn):
        return lambda q, kq, vq, ks, vs, cl, scale, window: fn(
            q, kq, vq, cl, window=window, k_scale=ks, v_scale=vs)
    check("decode", "dispatch", (40, 64), 1, 4, 64, 64,
          run=op(ops.decode_attention))
    check("extend", "dispatch", (40, 3), 9, 4, 64, 64,
          run=op(ops.extend_attention))
    k = torch.zeros(2, 1, 2, 64, dtype=torch.bfloat16, device=DEV)
    kq, ks, _ = quantised(k.expand(2, 64, 2, 64).transpose(1, 2).contiguous())
    cl = torch.zeros(2, dtype=torch.int32, device=DEV)
    ops.kv_append(kq, kq.clone(), cl, k, k, k_scale=ks, v_scale=ks.clone())
    assert spy.calls == ["attn_decode_fp8"] * 2 + ["attn_extend_fp8"] * 2 \
        + ["kv_append_fp8"], spy.calls


def extend_tail(model, ids, prefix, S):
    """kv_cache_ref.teacher_forced with the tokens after the prefill fed
    through `extend` in slices of 7; the same rows in the same order."""
    lens = torch.tensor(prefix, dtype=torch.int32, device=ids.device)
    cache = KVCache.allocate(model, len(prefix), S)
    got = [model.prefill(ids[:, :max(prefix)], lens, cache)]
    for done in range(0, S - max(prefix), 7):
        pos = lens.long()[:, None] + done + torch.arange(7, device=ids.device)
        got.append(model.extend(ids.gather(1, pos), cache)
                   .transpose(0, 1).flatten(0, 1))
    return torch.cat(got).double()


@pytest.mark.parametrize("family", ["llama", "gptneo"])
def test_e2e_fp8_cache(family, monkeypatch):
    """e_fp8 <= 2 sqrt(e_full^2 + e_q^2): e_full the bf16 GPU full forward
    and e_q the fp64 CPU model on an fp8 cache (pure quantisation error, by
    the reference path), both against the fp64 CPU forward."""
    model = TD._e2e_model(family)
    S, prefix = TD.E2E_S, TD.E2E_PREFIX
    assert (S - max(prefix)) % 7 == 0
    ids = torch.randint(0, 512, (len(prefix), S),
                        generator=torch.Generator().manual_seed(5))
    alloc = KVCache.allocate.__func__
    monkeypatch.setattr(KVCache, "allocate", classmethod(
        lambda cls, *a, **k: alloc(cls, *a, dtype=FP8, **k)))

    def rms(a, b):
        return float((a.cpu() - b).pow(2).mean().sqrt())
    m64, gpu = copy.deepcopy(model).double(), copy.deepcopy(model).to(DEV)
    q_dec, ref = teacher_forced(m64, ids, prefix, S)
    got, full = teacher_forced(gpu, ids.to(DEV), prefix, S)
    e_full = rms(full, ref)
    for tag, e_fp8, e_q in (
            ("decode_step", rms(got, ref), rms(q_dec, ref)),
            ("extend", rms(extend_tail(gpu, ids.to(DEV), prefix, S), ref),
             rms(extend_tail(m64, ids, prefix, S), ref))):
        print("E2E fp8 %s %s rms fp8 %.4e full %.4e quant %.4e bound %.4e"
              % (family, tag, e_fp8, e_full, e_q,
                 2 * math.hypot(e_full, e_q)))
        assert e_full > 0 and e_q > 0
        assert e_fp8 <= 2 * math.hypot(e_full, e_q), (family, tag)
