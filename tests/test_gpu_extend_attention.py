"""acco_attn_extend on the GPU against an fp64 reference under the flash
forward's criterion (attention_ref.py; in full: P is rounded to bf16), and
`extend` of both families in bf16. MEASURED: RESULTS.md, "Multi-token
attention on the KV cache"."""

import copy
import math

import pytest
import torch

from acco_amd import ops
from acco_amd.models import (GPTNeoConfig, GPTNeoForCausalLM, LlamaConfig,
                             LlamaForCausalLM)
from tests import attention_ref as AR
from tests.extend_ref import teacher_forced_extend

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _bits(t):
    return t.contiguous().view(torch.int16)


def extend_ref64(q, kc, vc, L0, scale, window):
    """In the form attention_ref.fwd_floor_terms reads; rows no query
    attends (NaN in the tests) are zeros before any arithmetic."""
    (B, T, H, D), Hkv, Smax = q.shape, kc.shape[1], kc.shape[2]
    p = L0.long().clamp(0, Smax)[:, None] + torch.arange(T, device=q.device)
    j = torch.arange(Smax, device=q.device)
    allow = (j <= p[..., None]) & (p < Smax)[..., None]
    if 0 < window < Smax:
        allow = allow & (j > p[..., None] - window)
    used = allow.any(1)[:, None, :, None]
    zero = torch.zeros((), dtype=torch.float64, device=q.device)
    kh = torch.where(used, kc.double(), zero).repeat_interleave(H // Hkv, 1)
    vh = torch.where(used, vc.double(), zero).repeat_interleave(H // Hkv, 1)
    s = torch.einsum("bthd,bhjd->bhtj", q.double(), kh) * scale
    s = s.masked_fill(~allow[:, None], -math.inf)
    e = torch.exp(s - s.amax(-1, keepdim=True).clamp(min=-1e300))
    P = e / e.sum(-1, keepdim=True).clamp(min=1e-300)
    return dict(o=(P @ vh).permute(0, 2, 1, 3).contiguous(), P=P, vh=vh,
                allow=allow[:, None])


def make_extend(name, L0, T, rep, D, Smax, Hkv=2):
    """q [B,T,H,D], caches with every row at or beyond min(L0 + T, Smax) NaN."""
    g = AR.case_generator(name)
    B = len(L0)
    q = (0.5 * torch.randn(B, T, Hkv * rep, D, generator=g)).bfloat16().to(DEV)
    kc = (0.5 * torch.randn(B, Hkv, Smax, D, generator=g)).bfloat16().to(DEV)
    vc = (0.5 * torch.randn(B, Hkv, Smax, D, generator=g)).bfloat16().to(DEV)
    cl = torch.tensor(L0, dtype=torch.int32, device=DEV)
    beyond = torch.arange(Smax, device=DEV)[None] >= (cl + T)[:, None]
    kc.masked_fill_(beyond[:, None, :, None], float("nan"))
    vc.masked_fill_(beyond[:, None, :, None], float("nan"))
    return q, kc, vc, cl


def check_extend(name, L0, T, rep, D, Smax, window=0, run=None, Hkv=2):
    q, kc, vc, cl = make_extend(name, L0, T, rep, D, Smax, Hkv)
    scale = D ** -0.5
    o = (run or ops.hip_ext().attn_extend)(q, kc, vc, cl, scale, window)
    assert o.shape == q.shape and o.dtype == torch.bfloat16
    assert not torch.isnan(o.float()).any(), name
    f = extend_ref64(q, kc, vc, cl, scale, window)
    floor = AR.floor_of(AR.fwd_floor_terms(f), "o", f["o"],
                        mult=AR.KERNEL_FLOOR)
    ratio, idx = AR.within(o, f["o"], floor)
    print("RATIO attn_extend D%d rep%d %s L0=%s T=%d Smax=%d w=%d: %.4f"
          % (D, rep, name, list(L0), T, Smax, window, ratio))
    assert ratio <= 1.0, (name, ratio, idx)
    for b, L in enumerate(L0):
        live = max(0, min(T, Smax - L))
        assert bool((_bits(o[b, live:]) == 0).all()), "dropped rows are +0"
        if window == 1:
            v = vc[b, :, L:L + live].transpose(0, 1).repeat_interleave(rep, 1)
            assert torch.equal(_bits(o[b, :live]), _bits(v)), "window 1: o = V"
    return q, kc, vc, cl, o, f, floor


# one axis at a time from a base case, then corners; L0 is an index into the
# issue's five pairs, window -1 means Smax + 1
BASE = dict(rep=3, Smax=300, T=33, L0=1, window=0)
AXES = dict(rep=[1, 8], Smax=[320], T=[1, 5, 64, 65], L0=[0, 2, 3, 4],
            window=[1, 16, 70, -1])
CASES = [BASE] + [dict(BASE, **{k: x}) for k, xs in AXES.items() for x in xs] \
    + [dict(rep=8, Smax=300, T=65, L0=4, window=70),
       dict(rep=1, Smax=320, T=64, L0=2, window=16),
       dict(rep=8, Smax=320, T=5, L0=3, window=1),
       dict(rep=1, Smax=300, T=1, L0=4, window=0),
       dict(rep=8, Smax=320, T=64, L0=0, window=1),
       dict(rep=3, Smax=300, T=65, L0=3, window=-1)]


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("c", CASES, ids=lambda c: "-".join(
    "%s%d" % kv for kv in c.items()))
def test_attn_extend_sweep(D, c):
    Smax, T = c["Smax"], c["T"]
    L0 = [(0, 0), (1, 63), (64, 65), (Smax - T, 0), (Smax - T + 3, 7)][c["L0"]]
    window = Smax + 1 if c["window"] < 0 else c["window"]
    check_extend("sweep", L0, T, c["rep"], D, Smax, window)


def test_attn_extend_split_grid_and_direct():
    # (B*Hkv, cols, Smax): 4 splits of 256 keys; the direct, one-split path
    assert ops.extend_attention_splits(2, 20, 1024) == (1, 4, 256)
    assert ops.extend_attention_splits(4, 260, 200) == (3, 1, 256)
    for L0 in ((251, 255), (256, 257), (1019, 0)):   # around a boundary
        check_extend("split", L0, 5, 4, 64, 1024, Hkv=1)
    check_extend("split", (250, 600), 5, 4, 128, 1024, window=300, Hkv=1)
    for L0, window in (((0, 130), 0), ((195, 64), 70), ((135, 7), 1)):
        check_extend("direct", L0, 65, 4, 64, 200, window)
        check_extend("direct", L0, 5, 8, 128, 200, window)
    q, kc, vc, cl = make_extend("twice", (251, 1019), 5, 4, 64, 1024, Hkv=1)
    a, b = (ops.hip_ext().attn_extend(q, kc, vc, cl, 0.125, 0) for _ in "ab")
    assert torch.equal(_bits(a), _bits(b))


def test_attn_extend_one_token_strided_q_and_wild_lens():
    ext = ops.hip_ext()
    # T = 1: the decode kernel meets the same floor of the same reference
    q, kc, vc, cl, o, f, floor = check_extend("t1", (0, 299), 1, 4, 64, 300)
    dec = ops.decode_attention(q[:, 0], kc, vc, cl + 1)
    assert AR.within(dec[:, None], f["o"], floor)[0] <= 1.0
    # q as a section of a packed row: same bits
    q, kc, vc, cl, o, _, _ = check_extend("strided", (3, 100), 33, 2, 64, 200)
    B, T, H, D = q.shape
    packed = torch.zeros(B, T, 3 * H * D, dtype=torch.bfloat16, device=DEV)
    packed[..., H * D:2 * H * D] = q.flatten(2)
    qv = packed[..., H * D:2 * H * D].unflatten(-1, (H, D))
    assert not qv.is_contiguous()
    assert torch.equal(_bits(ext.attn_extend(qv, kc, vc, cl, 0.125, 0)),
                       _bits(o))
    # cache_len is clamped: -1 is 0, 2^31 - 1 is Smax (every token dropped)
    kc, vc = (t.nan_to_num(0.25) for t in (kc, vc))
    wild = torch.tensor([-1, 2 ** 31 - 1], dtype=torch.int32, device=DEV)
    tame = torch.tensor([0, 200], dtype=torch.int32, device=DEV)
    a = ext.attn_extend(q, kc, vc, wild, 0.125, 0)
    b = ext.attn_extend(q, kc, vc, tame, 0.125, 0)
    assert torch.equal(_bits(a), _bits(b))
    assert bool((_bits(a[1]) == 0).all()) and bool((a[0] != 0).any())


def test_attn_extend_binding_checks():
    ext = ops.hip_ext()
    q, kc, vc, cl = make_extend("checks", (5, 9), 3, 2, 64, 64)
    z96 = torch.zeros(2, 2, 64, 96, dtype=torch.bfloat16, device=DEV)
    buf = torch.zeros(q.numel() + 8, dtype=torch.bfloat16, device=DEV)
    for match, args in [
            ("q must be CUDA bf16", (q.half(), kc, vc, cl, 0.125, 0)),
            ("k_cache must be contiguous", (q, kc.float(), vc, cl, 0.125, 0)),
            ("H/Hkv <= 8", (q.repeat(1, 1, 8, 1), kc, vc, cl, 0.125, 0)),
            ("D in", (q[..., :1].expand(2, 3, 4, 96).contiguous(), z96, z96,
                      cl, 0.125, 0)),
            ("q must be 16-byte aligned",
             (buf[1:1 + q.numel()].view_as(q), kc, vc, cl, 0.125, 0)),
            ("cache_len", (q, kc, vc, cl.long(), 0.125, 0)),
            ("window", (q, kc, vc, cl, 0.125, -1)),
            (r"\[B, T, H, D\]", (q[:, 0], kc, vc, cl, 0.125, 0)),
            ("1 <= T", (q[:, :0], kc, vc, cl, 0.125, 0))]:
        with pytest.raises(RuntimeError, match=match):
            ext.attn_extend(*args)


def test_extend_op_dispatches_to_hip(monkeypatch):
    """Inside the contract the reference is never reached; rep = 16 takes it
    and still meets the floor."""
    ext, calls = ops.hip_ext(), []

    class Spy:
        def __getattr__(self, name):
            calls.append(name)
            return getattr(ext, name)
    monkeypatch.setattr(ops, "hip_ext", Spy)

    def boom(*a, **k):
        raise AssertionError("torch reference reached inside the contract")

    def op(q, kc, vc, cl, scale, window):
        return ops.extend_attention(q, kc, vc, cl, window=window)
    with monkeypatch.context() as mp:
        mp.setattr(ops.torch_ref, "extend_attention", boom)
        check_extend("dispatch", (40, 3), 9, 4, 64, 64, run=op)
    assert calls == ["attn_extend"], calls
    check_extend("dispatch16", (40, 3), 9, 16, 64, 64, run=op)
    assert calls == ["attn_extend"], calls


# ------------------------------------------------------------- end to end
E2E_S, E2E_PREFIX = 256, [5, 70, 200]


@pytest.mark.parametrize("family", ["llama", "gptneo"])
def test_e2e_extend_bf16(family):
    """RMS error of the logits against the fp64 CPU forward of the same
    bf16-rounded weights at most 2x that of the full bf16 forward."""
    torch.manual_seed(0)
    kw = dict(num_layers=2, vocab_size=512, max_position_embeddings=512)
    model = (LlamaForCausalLM(LlamaConfig(
        hidden_size=256, num_heads=4, num_kv_heads=2, intermediate_size=512,
        **kw)) if family == "llama" else GPTNeoForCausalLM(GPTNeoConfig(
            hidden_size=128, num_heads=2, window_size=16, **kw)))
    model = model.to(torch.bfloat16).eval()
    ids = torch.randint(0, 512, (3, E2E_S),
                        generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        ref = copy.deepcopy(model).double()(ids)[0]
        model = model.to(DEV)
        full = model(ids.to(DEV))[0].double().cpu()
    for width in (7, 64):
        got, b, pos, _ = teacher_forced_extend(model, ids.to(DEV), E2E_PREFIX,
                                               width, 512)
        b, pos = b.cpu(), pos.cpu()
        e_ext = float((got.cpu() - ref[b, pos]).pow(2).mean().sqrt())
        e_full = float((full[b, pos] - ref[b, pos]).pow(2).mean().sqrt())
        print("E2E extend %s width %d rms %.4e full %.4e ratio %.3f"
              % (family, width, e_ext, e_full, e_ext / e_full))
        assert e_full > 0 and e_ext <= 2 * e_full, (family, width)
