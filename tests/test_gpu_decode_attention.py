"""The KV-cache kernels on the GPU: acco_kv_append (rope.hip) bit for bit
against the existing RoPE kernels, acco_attn_decode (attention_decode.hip)
against an fp64 reference under the criterion of the attention kernels
(tests/attention_ref.py: half-ulp of bf16 plus the floor of the forward's o at
KERNEL_FLOOR), and prefill / decode_step of both model families in bf16
against one full forward, with an fp64 CPU forward of the same bf16-rounded
weights as the yardstick.

The decode kernel keeps P in fp32 (there is no second MFMA to round it for),
so the bf16 term of that floor is slack here; the RATIO lines show how much of
the limit is used.

MEASURED (MI355X): RESULTS.md, "KV-cache generation".
"""

import copy
import math

import pytest
import torch

from acco_amd import ops
from acco_amd.models import (GPTNeoConfig, GPTNeoForCausalLM, LlamaConfig,
                             LlamaForCausalLM)
from acco_amd.models.kv_cache import KVCache
from tests import attention_ref as AR
from tests.kv_cache_ref import teacher_forced

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _ext():
    return ops.hip_ext()


def _bits(t):
    return t.contiguous().view(torch.int16)


# ------------------------------------------------------------- kv_append
APPEND_SMAX = 128
# (T, cache_len of the two sequences)
APPEND_CASES = [(1, (0, 0)), (1, (37, 100)), (70, (0, 0)), (70, (0, 50)),
                (3, (APPEND_SMAX - 1, 5))]


def _packed(order, T, Hkv, rep, D, g):
    """src [B, T, W] bf16 with spare columns, and (q, k, v) views of it."""
    B, H = 2, Hkv * rep
    W, q_off, k_off, v_off = AR.gqa_layout(Hkv, D, rep, order)
    src = torch.randn(B, T, W, generator=g).bfloat16().to(DEV)
    q = src[..., q_off:q_off + H * D].unflatten(-1, (H, D))
    k = src[..., k_off:k_off + Hkv * D].unflatten(-1, (Hkv, D))
    v = src[..., v_off:v_off + Hkv * D].unflatten(-1, (Hkv, D))
    return src, (W, q_off, k_off, v_off), q, k, v


def _sentinel_caches(B, Hkv, Smax, D, g):
    kc = torch.randn(B, Hkv, Smax, D, generator=g).bfloat16().to(DEV)
    vc = torch.randn(B, Hkv, Smax, D, generator=g).bfloat16().to(DEV)
    return kc, vc


def _expected_cache(before, new, lens, Smax):
    """`before` with new [B, T, Hkv, D] written at rows lens[b] + t < Smax."""
    want = before.clone()
    for b, cl in enumerate(lens):
        n = max(0, min(new.shape[1], Smax - cl))
        want[b, :, cl:cl + n] = new[b, :n].permute(1, 0, 2)
    return want


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("order", ["qkv", "kvq"])
@pytest.mark.parametrize("T,lens", APPEND_CASES)
def test_kv_append_bit_for_bit(D, order, T, lens):
    ext = _ext()
    Hkv, rep, Smax, B = 2, 2, APPEND_SMAX, 2
    H = Hkv * rep
    g = AR.case_generator("kv_append_%d_%s_%d_%s" % (D, order, T, lens))
    src, (W, q_off, k_off, v_off), q, k, v = _packed(order, T, Hkv, rep, D, g)
    src0 = src.clone()
    cl = torch.tensor(lens, dtype=torch.int32, device=DEV)
    cos, sin = AR.rope_tables(Smax, D, DEV)

    # without tables: K and V are the input bits, q is not asked for
    kc, vc = _sentinel_caches(B, Hkv, Smax, D, g)
    k0, v0 = kc.clone(), vc.clone()
    assert ops.kv_append(kc, vc, cl, k, v) is None
    assert torch.equal(_bits(kc), _bits(_expected_cache(k0, k, lens, Smax)))
    assert torch.equal(_bits(vc), _bits(_expected_cache(v0, v, lens, Smax)))

    # with tables: the tokens at their absolute positions of a [B, Smax, W]
    # row, rotated by the existing in-place kernel
    full = torch.zeros(B, Smax, W, dtype=torch.bfloat16, device=DEV)
    kept = [max(0, min(T, Smax - c)) for c in lens]
    for b, c in enumerate(lens):
        full[b, c:c + kept[b]] = src[b, :kept[b]]
    # and K alone through the out-of-place RoPE kernel
    k_full = full[..., k_off:k_off + Hkv * D].unflatten(-1, (Hkv, D)) \
        .contiguous()
    k_rope = ext.rope_fwd(k_full, cos, sin, False)
    ext.rope_qk_inplace(full, cos, sin, H, Hkv, D, q_off, k_off)
    fq = full[..., q_off:q_off + H * D].unflatten(-1, (H, D))
    fk = full[..., k_off:k_off + Hkv * D].unflatten(-1, (Hkv, D))
    assert torch.equal(_bits(fk), _bits(k_rope))
    kc, vc = k0.clone(), v0.clone()
    q_rot = ops.kv_append(kc, vc, cl, k, v, q, cos, sin)
    assert q_rot.shape == (B, T, H, D) and q_rot.is_contiguous()
    k_new = torch.zeros(B, T, Hkv, D, dtype=torch.bfloat16, device=DEV)
    for b, c in enumerate(lens):
        n = kept[b]
        k_new[b, :n] = fk[b, c:c + n]
        assert torch.equal(_bits(q_rot[b, :n]), _bits(fq[b, c:c + n]))
    assert torch.isfinite(q_rot.float()).all()
    assert torch.equal(_bits(kc), _bits(_expected_cache(k0, k_new, lens, Smax)))
    assert torch.equal(_bits(vc), _bits(_expected_cache(v0, v, lens, Smax)))
    # the source is read only, cache_len too
    assert torch.equal(_bits(src), _bits(src0))
    assert cl.tolist() == list(lens)


def test_kv_append_separate_tensors_and_checks():
    ext = _ext()
    B, T, Hkv, H, D, Smax = 2, 5, 2, 4, 64, 16
    g = AR.case_generator("kv_append_separate")
    q = torch.randn(B, T, H, D, generator=g).bfloat16().to(DEV)
    k = torch.randn(B, T, Hkv, D, generator=g).bfloat16().to(DEV)
    v = torch.randn(B, T, Hkv, D, generator=g).bfloat16().to(DEV)
    kc, vc = _sentinel_caches(B, Hkv, Smax, D, g)
    k0 = kc.clone()
    lens = (3, 14)
    cl = torch.tensor(lens, dtype=torch.int32, device=DEV)
    ops.kv_append(kc, vc, cl, k, v)
    assert torch.equal(_bits(kc), _bits(_expected_cache(k0, k, lens, Smax)))
    # a cache_len outside [0, Smax] is clamped, never an index
    wild = torch.tensor([-5, 2 ** 31 - 1], dtype=torch.int32, device=DEV)
    kc2 = k0.clone()
    ops.kv_append(kc2, vc, wild, k, v)
    assert torch.equal(_bits(kc2),
                       _bits(_expected_cache(k0, k, (0, Smax), Smax)))
    cos, sin = AR.rope_tables(Smax, D, DEV)
    none = None
    with pytest.raises(RuntimeError, match="cache_len"):
        ext.kv_append(none, k, v, none, none, kc, vc, cl.long())
    with pytest.raises(RuntimeError, match="k must be"):
        ext.kv_append(none, k.float(), v, none, none, kc, vc, cl)
    with pytest.raises(RuntimeError, match="v must"):
        ext.kv_append(none, k, v.transpose(1, 2).contiguous().transpose(1, 2),
                      none, none, kc, vc, cl)
    with pytest.raises(RuntimeError, match="D in"):
        ext.kv_append(none, k[..., :32].contiguous(), v[..., :32].contiguous(),
                      none, none, kc[..., :32].contiguous(),
                      vc[..., :32].contiguous(), cl)
    with pytest.raises(RuntimeError, match="cos"):
        ext.kv_append(q, k, v, cos[:Smax - 1], sin[:Smax - 1], kc, vc, cl)
    with pytest.raises(RuntimeError, match="q is rotated"):
        ext.kv_append(q, k, v, none, none, kc, vc, cl)


# ------------------------------------------------------------ attn_decode
def decode_ref64(q, kc, vc, lens, scale, window):
    """fp64 reference of one query row per sequence, in the form
    attention_ref.fwd_floor_terms reads: o [B,1,H,D], P [B,H,1,Smax],
    vh [B,H,Smax,D], allow [B,1,1,Smax]. Rows outside the key range are
    replaced by zeros before any arithmetic (the tests fill them with NaN)."""
    B, H, D = q.shape
    Hkv, Smax = kc.shape[1], kc.shape[2]
    L = lens.long().clamp(0, Smax)[:, None]
    j = torch.arange(Smax, device=q.device)[None]
    allow = j < L
    if 0 < window < Smax:
        allow = allow & (j >= L - window)
    a4 = allow[:, None, :, None]
    zero = torch.zeros((), dtype=torch.float64, device=q.device)
    rep = H // Hkv
    kh = torch.where(a4, kc.double(), zero).repeat_interleave(rep, dim=1)
    vh = torch.where(a4, vc.double(), zero).repeat_interleave(rep, dim=1)
    s = torch.einsum("bhd,bhjd->bhj", q.double(), kh) * scale
    s = s.masked_fill(~allow[:, None], -math.inf)
    m = s.amax(-1, keepdim=True).clamp(min=-1e300)
    p = torch.exp(s - m)
    P = (p / p.sum(-1, keepdim=True).clamp(min=1e-300))[:, :, None, :]
    o = (P @ vh).permute(0, 2, 1, 3).contiguous()          # [B,1,H,D]
    return dict(o=o, P=P, vh=vh, allow=allow[:, None, None, :])


def make_decode(name, lens, Hkv, rep, D, Smax):
    """q [B,H,D], caches with every row at or beyond lens[b] NaN, lens."""
    g = AR.case_generator(name)
    B, H = len(lens), Hkv * rep
    q = (0.5 * torch.randn(B, H, D, generator=g)).bfloat16().to(DEV)
    kc = (0.5 * torch.randn(B, Hkv, Smax, D, generator=g)).bfloat16().to(DEV)
    vc = (0.5 * torch.randn(B, Hkv, Smax, D, generator=g)).bfloat16().to(DEV)
    cl = torch.tensor(lens, dtype=torch.int32, device=DEV)
    beyond = torch.arange(Smax, device=DEV)[None] >= cl[:, None]
    kc.masked_fill_(beyond[:, None, :, None], float("nan"))
    vc.masked_fill_(beyond[:, None, :, None], float("nan"))
    return q, kc, vc, cl


def check_decode(name, lens, Hkv, rep, D, Smax, window=0, scale=None):
    """Run the kernel and hold o to the criterion; returns (o, ratio)."""
    scale = D ** -0.5 if scale is None else scale
    q, kc, vc, cl = make_decode(name, lens, Hkv, rep, D, Smax)
    o = _ext().attn_decode(q, kc, vc, cl, scale, window)
    assert o.shape == q.shape and o.dtype == torch.bfloat16
    assert not torch.isnan(o.float()).any(), name
    f = decode_ref64(q, kc, vc, cl, scale, window)
    floor = AR.floor_of(AR.fwd_floor_terms(f), "o", f["o"],
                        mult=AR.KERNEL_FLOOR)
    ratio, idx = AR.within(o[:, None], f["o"], floor)
    print("RATIO attn_decode D%d rep%d %s lens=%s Smax=%d w=%d s=%g: %.4f"
          % (D, rep, name, list(lens), Smax, window, scale, ratio))
    assert ratio <= 1.0, (name, ratio, idx)
    for b, L in enumerate(lens):
        if L <= 0:
            assert bool((_bits(o[b]) == 0).all()), "L = 0 gives o = +0"
        elif window == 1:
            last = vc[b, :, min(L, Smax) - 1].repeat_interleave(rep, dim=0)
            assert torch.equal(_bits(o[b]), _bits(last)), "window 1: o = V"
    return o, ratio


SMAX = 1024     # with B*Hkv = 4: 4 splits of 256 keys


def test_decode_split_grid():
    """The split count is a host function of (B*Hkv, Smax) alone; the shapes
    below rely on these values to sit on its edges."""
    assert ops.decode_attention_splits(4, SMAX) == (4, 256)
    assert ops.decode_attention_splits(1, 4096) == (16, 256)
    assert ops.decode_attention_splits(2, 300) == (2, 192)
    assert ops.decode_attention_splits(1024, 4096) == (1, 4096)
    assert ops.decode_attention_splits(1, 1) == (1, 64)
    n, chunk = ops.decode_attention_splits(1, 2 ** 30 - 1)
    assert n == 64 and n * chunk >= 2 ** 30 - 1


# one below / at / one above a split boundary, L = 1, L = Smax, a sequence
# whose splits are nearly all empty next to a full one, an empty sequence
LENS = [(1, SMAX), (255, 256), (257, SMAX), (0, SMAX), (SMAX, 700)]


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("rep", [1, 4, 8])
def test_attn_decode_lengths(D, rep):
    for lens in LENS:
        check_decode("len", lens, 2, rep, D, SMAX)
    # twice, same bits
    q, kc, vc, cl = make_decode("twice", (SMAX, 700), 2, rep, D, SMAX)
    a = _ext().attn_decode(q, kc, vc, cl, D ** -0.5, 0)
    b = _ext().attn_decode(q, kc, vc, cl, D ** -0.5, 0)
    assert torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize("D", [64, 128])
def test_attn_decode_windows_and_scale(D):
    lens = (700, SMAX)
    # 1; L - 1 and L of sequence 0; one that starts inside split 1 (key 400
    # of [256, 512)); at and beyond Smax (the binding hands the kernel 0)
    for window in (1, 699, 700, 300, SMAX, SMAX + 1, 2 ** 31 + 5):
        check_decode("win", lens, 2, 4, D, SMAX, window=window)
    check_decode("win", (1, 2), 2, 4, D, SMAX, window=1)
    # GPT-Neo: no scaling, a local layer's window
    check_decode("scale1", lens, 2, 1, D, SMAX, scale=1.0)
    check_decode("scale1", lens, 2, 1, D, SMAX, window=256, scale=1.0)


def test_attn_decode_other_grids():
    # 16 splits; a long cache of one (sequence, kv head) pair
    check_decode("long", (4096,), 1, 8, 128, 4096)
    check_decode("long", (1000,), 1, 8, 128, 4096, window=600)
    # Smax no multiple of the chunk, an odd group size: splits [0, 192) and
    # [192, 300)
    check_decode("odd", (191, 192), 1, 3, 64, 300)
    check_decode("odd", (193, 300), 1, 3, 64, 300)
    check_decode("odd", (300, 7), 1, 5, 128, 300, window=150)
    # one split only
    check_decode("one", (1, 200, 64, 65), 3, 2, 64, 200)
    # a cache_len outside [0, Smax] is clamped: -1 is empty, 2^31 - 1 is full
    q, kc, vc, cl = make_decode("wild", (0, 200), 1, 2, 64, 200)
    wild = torch.tensor([-1, 2 ** 31 - 1], dtype=torch.int32, device=DEV)
    a = _ext().attn_decode(q, kc, vc, cl, 0.125, 0)
    b = _ext().attn_decode(q, kc, vc, wild, 0.125, 0)
    assert torch.equal(_bits(a), _bits(b))


def test_attn_decode_strided_q():
    """q as the q section of a packed projection output (row stride W)."""
    q, kc, vc, cl = make_decode("strided", (100, 256), 2, 2, 64, 256)
    B, H, D = q.shape
    packed = torch.zeros(B, 3 * H * D, dtype=torch.bfloat16, device=DEV)
    packed[:, H * D:2 * H * D] = q.reshape(B, -1)
    qv = packed[:, H * D:2 * H * D].view(B, H, D)
    assert not qv.is_contiguous()
    a = _ext().attn_decode(q, kc, vc, cl, 0.125, 0)
    b = _ext().attn_decode(qv, kc, vc, cl, 0.125, 0)
    assert torch.equal(_bits(a), _bits(b))


def test_attn_decode_binding_checks():
    ext = _ext()
    q, kc, vc, cl = make_decode("checks", (5, 9), 2, 2, 64, 64)
    with pytest.raises(RuntimeError, match="q must be CUDA bf16"):
        ext.attn_decode(q.half(), kc, vc, cl, 0.125, 0)
    with pytest.raises(RuntimeError, match="k_cache must be contiguous"):
        ext.attn_decode(q, kc.float(), vc, cl, 0.125, 0)
    q16 = torch.zeros(2, 32, 64, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match="H/Hkv <= 8"):
        ext.attn_decode(q16, kc, vc, cl, 0.125, 0)       # rep = 16
    z = torch.zeros(2, 2, 64, 96, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match="D in"):
        ext.attn_decode(q[..., :1].expand(2, 4, 96).contiguous(), z, z, cl,
                        0.125, 0)                        # D = 96
    buf = torch.zeros(q.numel() + 8, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match="q must be 16-byte aligned"):
        ext.attn_decode(buf[1:1 + q.numel()].view_as(q), kc, vc, cl, 0.125, 0)
    cbuf = torch.zeros(kc.numel() + 8, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        ext.attn_decode(q, cbuf[1:1 + kc.numel()].view_as(kc), vc, cl, 0.125,
                        0)
    with pytest.raises(RuntimeError, match="cache_len"):
        ext.attn_decode(q, kc, vc, cl[:1], 0.125, 0)
    with pytest.raises(RuntimeError, match="window"):
        ext.attn_decode(q, kc, vc, cl, 0.125, -1)


# --------------------------------------------------------------- dispatch
class _Spy:
    """The extension, recording which entry points are reached."""

    def __init__(self, ext):
        self._ext, self.calls = ext, []

    def __getattr__(self, name):
        self.calls.append(name)
        return getattr(self._ext, name)


def test_decode_ops_dispatch_to_hip(monkeypatch):
    """Inside the contract both ops reach the kernels and never the torch
    reference; rep = 16 is outside it, takes the reference and still matches
    fp64."""
    spy = _Spy(_ext())
    monkeypatch.setattr(ops, "hip_ext", lambda: spy)

    def boom(*a, **k):
        raise AssertionError("torch reference reached inside the contract")
    q, kc, vc, cl = make_decode("dispatch", (40, 64), 2, 4, 64, 64)
    with monkeypatch.context() as mp:
        mp.setattr(ops.torch_ref, "decode_attention", boom)
        mp.setattr(ops.torch_ref, "kv_append", boom)
        o = ops.decode_attention(q, kc, vc, cl, window=None)
        k = torch.zeros(2, 1, 2, 64, dtype=torch.bfloat16, device=DEV)
        ops.kv_append(kc, vc, cl, k, k)
    assert spy.calls == ["attn_decode", "kv_append"], spy.calls
    assert torch.equal(_bits(o), _bits(_ext().attn_decode(
        q, *make_decode("dispatch", (40, 64), 2, 4, 64, 64)[1:], 0.125, 0)))

    spy.calls.clear()
    q, kc, vc, cl = make_decode("dispatch16", (40, 64), 1, 16, 64, 64)
    o = ops.decode_attention(q, kc, vc, cl)
    assert spy.calls == []
    f = decode_ref64(q, kc, vc, cl, 0.125, 0)
    floor = AR.floor_of(AR.fwd_floor_terms(f), "o", f["o"],
                        mult=AR.KERNEL_FLOOR)
    ratio, _ = AR.within(o[:, None], f["o"], floor)
    print("RATIO decode reference path rep16: %.4f" % ratio)
    assert ratio <= 1.0


# ------------------------------------------------------------- end to end
E2E_S = 256
E2E_PREFIX = [5, 70, 200]


def _e2e_model(family):
    torch.manual_seed(0)
    if family == "llama":
        cfg = LlamaConfig(hidden_size=256, num_layers=2, num_heads=4,
                          num_kv_heads=2, intermediate_size=512,
                          vocab_size=512, max_position_embeddings=512)
        model = LlamaForCausalLM(cfg)
    else:
        cfg = GPTNeoConfig(hidden_size=128, num_layers=2, num_heads=2,
                           vocab_size=512, max_position_embeddings=256,
                           window_size=16)
        model = GPTNeoForCausalLM(cfg)
    assert cfg.head_dim == 64
    return model.to(torch.bfloat16).eval()


@pytest.fixture(scope="module", params=["llama", "gptneo"])
def e2e(request):
    """The bf16 model, the token rows and the fp64 CPU logits of the same
    bf16-rounded weights at every compared position, computed once."""
    model = _e2e_model(request.param)
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(0, 512, (len(E2E_PREFIX), E2E_S), generator=g)
    model64 = copy.deepcopy(model).double()
    _, ref = teacher_forced(model64, ids, E2E_PREFIX, E2E_S)
    return dict(family=request.param, model=model, ids=ids, ref=ref)


def _e2e_check(tag, model, ids, ref):
    got, full = teacher_forced(model, ids.to(DEV), E2E_PREFIX, E2E_S)
    e_cached = float((got.cpu() - ref).pow(2).mean().sqrt())
    e_full = float((full.cpu() - ref).pow(2).mean().sqrt())
    print("E2E %s rms cached %.4e full %.4e ratio %.3f"
          % (tag, e_cached, e_full, e_cached / e_full))
    assert e_full > 0 and math.isfinite(e_cached)
    assert e_cached <= 2 * e_full, (tag, e_cached, e_full)


def test_e2e_teacher_forced_bf16(e2e):
    model = copy.deepcopy(e2e["model"]).to(DEV)
    _e2e_check(e2e["family"], model, e2e["ids"], e2e["ref"])


def test_e2e_teacher_forced_bf16_fused_arena(e2e):
    """The same with the projections fused on a parameter arena: the prefill
    takes the packed attention path, decode_step the per-projection weights,
    which alias the arena."""
    from acco_amd.engine import arena
    from acco_amd.models.fuse import install_fused_projections
    model = copy.deepcopy(e2e["model"])
    p = arena.flatten_params(model, torch.bfloat16, torch.device(DEV),
                             pad_to=256)
    gr = arena.attach_grad_arena(model, torch.bfloat16, torch.device(DEV),
                                 pad_to=256)
    assert install_fused_projections(model, p, gr) > 0
    _e2e_check(e2e["family"] + " fused", model, e2e["ids"], e2e["ref"])
