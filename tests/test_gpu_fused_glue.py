"""The fused glue kernels against the fp32 torch reference: in-place q|k
RoPE on the packed projection, the packed attention backward with the
inverse RoPE folded into the dq epilogue and the GQA reduce, the RMSNorm
forward at the row/width edge cases, and the one-launch norm weight-grad
finalize.
Tolerances are those of the corresponding tests in test_gpu_kernels.py
(test_rope_fwd_bwd, test_rmsnorm_fwd_bwd, the add-norm test) and
test_gpu_attention.py (run_case)."""

import hashlib
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "packed_attn_norope.json")


def _close_bf16(a, b, atol=3e-2, rtol=3e-2):
    return torch.allclose(a.float(), b.float(), atol=atol, rtol=rtol)


def _sha(t):
    return hashlib.sha256(
        t.detach().contiguous().view(torch.int16).cpu().numpy().tobytes()
    ).hexdigest()


def _packed_inputs(B, S, H, Hkv, D, seed):
    """CPU-generated (device-independent) packed projection + upstream grad."""
    g = torch.Generator().manual_seed(seed)
    W = (H + 2 * Hkv) * D
    qkv = (torch.randn(B, S, W, generator=g) * 0.5).bfloat16().cuda()
    dO = torch.randn(B, S, H * D, generator=g).bfloat16().cuda()
    return qkv, dO


def _ref_core(qkv, dO, H, Hkv, D, offs, cos, sin, scale, window):
    """fp32 reference of (RoPE +) attention over the packed layout; returns
    (o, dqkv) in fp32."""
    from acco_amd.ops import torch_ref
    B, S, _ = qkv.shape
    q_off, k_off, v_off = offs
    x = qkv.detach().float().requires_grad_(True)
    q = x[..., q_off:q_off + H * D].reshape(B, S, H, D)
    k = x[..., k_off:k_off + Hkv * D].reshape(B, S, Hkv, D)
    v = x[..., v_off:v_off + Hkv * D].reshape(B, S, Hkv, D)
    if cos is not None:
        q, k = torch_ref.rope_apply(q, k, cos, sin)
    o = torch_ref.causal_attention(q, k, v, scale=scale,
                                   window=window or None)
    o = o.reshape(B, S, H * D)
    o.backward(dO.float())
    return o.detach(), x.grad


# ------------------------------------------------------- in-place q|k RoPE
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("H,Hkv", [(4, 2), (2, 2)])
def test_rope_qk_inplace(D, H, Hkv):
    from acco_amd import ops
    from acco_amd.ops import torch_ref
    ext = ops.hip_ext()
    B, S = 2, 256
    torch.manual_seed(0)
    W = (H + 2 * Hkv) * D
    q_off, k_off, v_off = 0, H * D, (H + Hkv) * D
    qkv = torch.randn(B, S, W, device="cuda").bfloat16()
    cos, sin = torch_ref.rope_cos_sin(S, D, 10000.0, "cuda")

    want = torch.zeros_like(qkv)
    ext.rope_packed(qkv, want, cos, sin, q_off, H, D, False)
    ext.rope_packed(qkv, want, cos, sin, k_off, Hkv, D, False)

    got = qkv.clone()
    ext.rope_qk_inplace(got, cos, sin, H, Hkv, D, q_off, k_off)
    assert torch.equal(got[..., v_off:], qkv[..., v_off:]), "V was touched"
    assert _close_bf16(got[..., :v_off], want[..., :v_off])
    assert torch.equal(got[..., :v_off], want[..., :v_off])
    err =(got[..., :v_off].float() - want[..., :v_off].float()).abs().max()
    print(f"rope_qk_inplace vs rope_packed max abs diff {float(err):.3e}")

    q32 = qkv[..., :k_off].float().reshape(B, S, H, D)
    k32 = qkv[..., k_off:v_off].float().reshape(B, S, Hkv, D)
    qr, kr = torch_ref.rope_apply(q32, k32, cos, sin)
    assert _close_bf16(got[..., :k_off], qr.reshape(B, S, -1))
    assert _close_bf16(got[..., k_off:v_off], kr.reshape(B, S, -1))


# ---------------------------- packed attention core, folded inverse RoPE
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("H,Hkv", [(4, 2), (2, 2)])
def test_packed_core_bwd_folded_rope(D, H, Hkv):
    """S=512 = two 256-row blocks: the causal diagonal and an interior tile.
    dqkv (inverse RoPE applied inside the dq epilogue / the GQA reduce)
    against the fp32 reference of RoPE + attention."""
    from acco_amd.ops import torch_ref
    from acco_amd.ops.autograd import AttnQKVPackedFn
    B, S = 1, 512
    offs = (0, H * D, (H + Hkv) * D)
    qkv, dO = _packed_inputs(B, S, H, Hkv, D, seed=10 + D + H)
    cos, sin = torch_ref.rope_cos_sin(S, D, 10000.0, "cuda")
    o_ref, d_ref = _ref_core(qkv, dO, H, Hkv, D, offs, cos, sin,
                             D ** -0.5, 0)

    leaf = qkv.clone().requires_grad_(True)
    x = leaf * 1.0          # non-leaf: the Function rotates it in place
    o, roped = AttnQKVPackedFn.apply(x, cos, sin, H, Hkv, D, D ** -0.5, 0,
                                     offs)
    assert roped.data_ptr() == x.data_ptr()
    assert torch.equal(roped[..., offs[2]:], qkv[..., offs[2]:])
    atol, rtol = 4e-2, 4e-2                  # test_gpu_attention.run_case
    assert torch.allclose(o.float(), o_ref, atol=atol, rtol=rtol), \
        (o.float() - o_ref).abs().max()
    o.backward(dO)
    for name, lo, hi in (("dq", offs[0], offs[1]), ("dk", offs[1], offs[2]),
                         ("dv", offs[2], qkv.shape[-1])):
        got, want = leaf.grad[..., lo:hi].float(), d_ref[..., lo:hi]
        e = (got - want).abs().max().item()
        print(f"{name} max abs err {e:.3e}")
        assert torch.allclose(got, want, atol=atol * 2, rtol=rtol), \
            f"{name} err {e}"

    # the fold must not change results: the unfused sequence (dq and the
    # plain GQA reduce stored in bf16, then the stand-alone inverse rope
    # over the q and k grad sections) gives the same bits
    from acco_amd import ops
    ext = ops.hip_ext()
    q_off, k_off, v_off = offs
    o_d = o.detach()
    lse = ext.attn_fwd_packed(roped.detach(), H, Hkv, D, D ** -0.5, 0,
                              *offs)[1]
    delta = ext.attn_delta(dO.view(B, S, H, D), o_d.view(B, S, H, D))
    d_seq = torch.empty_like(qkv)
    dkq, dvq = ext.attn_bwd_packed(roped.detach(), dO, lse, delta, d_seq, H,
                                   Hkv, D, D ** -0.5, 0, *offs)
    ext.attn_gqa_reduce(dkq, dvq, d_seq, Hkv, H // Hkv, D, k_off, v_off)
    ext.rope_packed(d_seq, d_seq, cos, sin, q_off, H, D, True)
    ext.rope_packed(d_seq, d_seq, cos, sin, k_off, Hkv, D, True)
    assert torch.equal(leaf.grad, d_seq), \
        (leaf.grad.float() - d_seq.float()).abs().max()

    # a leaf input must survive untouched (rotated on a private copy)
    leaf2 = qkv.clone().requires_grad_(True)
    o2, _ = AttnQKVPackedFn.apply(leaf2, cos, sin, H, Hkv, D, D ** -0.5, 0,
                                  offs)
    assert torch.equal(leaf2.detach(), qkv)
    o2.backward(dO)
    assert torch.equal(o2, o) and torch.equal(leaf2.grad, leaf.grad)


NOROPE_CASES = [
    # name, H, Hkv, D, offs-kind, scale, window
    ("qkv_h4_kv2_d64", 4, 2, 64, "qkv", None, 0),
    ("qkv_h2_kv2_d64", 2, 2, 64, "qkv", None, 0),
    ("qkv_h4_kv2_d128", 4, 2, 128, "qkv", None, 0),
    ("qkv_h2_kv2_d128", 2, 2, 128, "qkv", None, 0),
    ("kvq_gptneo_h4_d64_w64", 4, 4, 64, "kvq", 1.0, 64),
]


def norope_case(name):
    """Run one cos=None case of the packed core; returns (o, dqkv, refs).
    Module-level so the golden hashes can be regenerated with the same
    inputs from any build of the package."""
    from acco_amd.ops.autograd import AttnQKVPackedFn
    _, H, Hkv, D, kind, scale, window = next(
        c for c in NOROPE_CASES if c[0] == name)
    B, S = 1, 512
    d = H * D
    offs = (0, H * D, (H + Hkv) * D) if kind == "qkv" else (2 * d, 0, d)
    scale = D ** -0.5 if scale is None else scale
    qkv, dO = _packed_inputs(B, S, H, Hkv, D, seed=len(name) + D + H)
    leaf = qkv.clone().requires_grad_(True)
    o = AttnQKVPackedFn.apply(leaf * 1.0, None, None, H, Hkv, D, scale,
                              window, offs)
    o.backward(dO)
    ref = _ref_core(qkv, dO, H, Hkv, D, offs, None, None, scale, window)
    return o.detach(), leaf.grad, ref


@pytest.mark.parametrize("name", [c[0] for c in NOROPE_CASES])
def test_packed_core_norope_unchanged(name):
    """cos=None (incl. the GPT-Neo k|v|q order with a local window) must
    give the results of the path before the RoPE fold, bit for bit: the
    sha256 of o and dqkv recorded from that build are the golden values."""
    o, dqkv, (o_ref, d_ref) = norope_case(name)
    assert torch.allclose(o.float(), o_ref, atol=4e-2, rtol=4e-2)
    assert torch.allclose(dqkv.float(), d_ref, atol=8e-2, rtol=4e-2)
    with open(GOLDEN) as f:
        gold = json.load(f)[name]
    assert _sha(o) == gold["o"]
    assert _sha(dqkv) == gold["dqkv"]


# ------------------------------------------------------------- RMSNorm fwd
ROWS = [1, 5, 1027]       # fewer rows than waves in a block; odd tail
DIMS = [256, 768, 2048, 4096]


def _norm_inputs(R, D):
    torch.manual_seed(R * 7 + D)
    x = torch.randn(R, D, device="cuda").bfloat16()
    res = torch.randn(R, D, device="cuda").bfloat16()
    w = (torch.randn(D, device="cuda") * 0.1 + 1.0).bfloat16()
    return x, res, w


@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("R", ROWS)
def test_rmsnorm_fwd_with_and_without_residual(R, D):
    from acco_amd import ops
    from acco_amd.ops import torch_ref
    ext = ops.hip_ext()
    x, res, w = _norm_inputs(R, D)
    ref = torch_ref.rms_norm(x.float(), w.float(), 1e-5)
    s32 = x.float() + res.float()
    ref_add = torch_ref.rms_norm(s32, w.float(), 1e-5)
    rstd_ref = torch.rsqrt(x.float().pow(2).mean(-1) + 1e-5)
    y, rstd = ext.rmsnorm_fwd(x, w, 1e-5)
    assert _close_bf16(y, ref), (y.float() - ref).abs().max()
    # fp32 statistics on both sides: only the summation order differs
    assert torch.allclose(rstd, rstd_ref, atol=1e-5, rtol=1e-4)
    y2, s, rstd2 = ext.add_rmsnorm_fwd(x, res, w, 1e-5)
    assert _close_bf16(y2, ref_add, atol=3e-2, rtol=3e-2)
    assert _close_bf16(s, s32, atol=1e-2, rtol=1e-2)
    assert torch.equal(s, s32.bfloat16())
    assert rstd2.shape == (R,)


# ------------------------------------------------- norm backward weight grad
@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("R", ROWS)
def test_rmsnorm_bwd_weight_grad(R, D):
    """dW through the one-launch finalize (partial rows → bf16). R=1 and
    R=5 leave waves / row groups of the last block without a live row, so
    the scratch holds partial rows that saw no data."""
    from acco_amd import ops
    from acco_amd.ops import torch_ref
    x, res, w = _norm_inputs(R, D)
    dout = torch.randn(R, D, device="cuda").bfloat16()
    dsum = torch.randn(R, D, device="cuda").bfloat16()

    xg = x.clone().requires_grad_(True)
    wg = w.clone().requires_grad_(True)
    ops.rms_norm(xg, wg, 1e-5).backward(dout)
    x32 = x.float().requires_grad_(True)
    w32 = w.float().requires_grad_(True)
    torch_ref.rms_norm(x32, w32, 1e-5).backward(dout.float())
    assert wg.grad.dtype == torch.bfloat16 and wg.grad.shape == (D,)
    assert _close_bf16(xg.grad, x32.grad)
    e = (wg.grad.float() - w32.grad).abs().max().item()
    print(f"rmsnorm dW max abs err {e:.3e}")
    assert _close_bf16(wg.grad, w32.grad, atol=0.1, rtol=0.05)

    # fused residual form (add-norm test's tolerances)
    xg = x.clone().requires_grad_(True)
    rg = res.clone().requires_grad_(True)
    wg = w.clone().requires_grad_(True)
    y, s = ops.add_rms_norm(xg, rg, wg, 1e-5)
    ((y.float() * dout.float()).sum() + (s.float() * dsum.float()).sum()
     ).backward()
    x32 = x.float().requires_grad_(True)
    r32 = res.float().requires_grad_(True)
    w32 = w.float().requires_grad_(True)
    s32 = x32 + r32
    y32 = torch_ref.rms_norm(s32, w32, 1e-5)
    ((y32 * dout.float()).sum() + (s32 * dsum.float()).sum()).backward()
    assert _close_bf16(xg.grad, x32.grad, atol=3e-2, rtol=5e-2)
    assert _close_bf16(rg.grad, r32.grad, atol=3e-2, rtol=5e-2)
    assert torch.allclose(wg.grad.float(), w32.grad, atol=0.3, rtol=5e-2)


@pytest.mark.parametrize("D", [768, 2048])
@pytest.mark.parametrize("R", ROWS)
def test_layernorm_bwd_weight_bias_grad(R, D):
    """LayerNorm dW and dB leave the same finalize launch."""
    from acco_amd import ops
    from acco_amd.ops import torch_ref
    x, _, w = _norm_inputs(R, D)
    b = (torch.randn(D, device="cuda") * 0.1).bfloat16()
    dout = torch.randn(R, D, device="cuda").bfloat16()
    xg = x.clone().requires_grad_(True)
    wg = w.clone().requires_grad_(True)
    bg = b.clone().requires_grad_(True)
    ops.layer_norm(xg, wg, bg, 1e-5).backward(dout)
    x32 = x.float().requires_grad_(True)
    w32 = w.float().requires_grad_(True)
    b32 = b.float().requires_grad_(True)
    torch_ref.layer_norm(x32, w32, b32, 1e-5).backward(dout.float())
    assert _close_bf16(xg.grad, x32.grad)
    assert _close_bf16(wg.grad, w32.grad, atol=0.1, rtol=0.05)
    assert _close_bf16(bg.grad, b32.grad, atol=0.1, rtol=0.05)


# --------------------------------------------------------------- end to end
def test_packed_core_checkpointing_on_off_same_grads():
    """The 2-layer model of test_packed_qkv_core_matches_standard_path with
    gradient checkpointing on and off: the recompute re-runs the in-place
    RoPE on a fresh projection output, so the gradients must agree (to that
    test's own bound)."""
    from acco_amd.engine import arena
    from acco_amd.models import LlamaConfig, LlamaForCausalLM
    from acco_amd.models.fuse import install_fused_projections

    cfg = LlamaConfig(hidden_size=256, num_layers=2, num_heads=4,
                      num_kv_heads=2, intermediate_size=512, vocab_size=512,
                      max_position_embeddings=512)
    dev = torch.device("cuda")
    torch.manual_seed(0)
    ids = torch.randint(0, 512, (2, 256), device=dev)
    out = []
    for ckpt in (False, True):
        torch.manual_seed(0)
        m = LlamaForCausalLM(cfg)
        p = arena.flatten_params(m, torch.bfloat16, dev, pad_to=256)
        g = arena.attach_grad_arena(m, torch.bfloat16, dev, pad_to=256)
        assert install_fused_projections(m, p, g) > 0
        m.model.gradient_checkpointing = ckpt
        loss, _ = m(ids, labels=ids)
        loss.backward()
        out.append((loss.item(), g[:arena.live_numel(m)].float().clone()))
    (l1, g1), (l2, g2) = out
    assert abs(l1 - l2) < 2e-2, (l1, l2)
    cos = torch.nn.functional.cosine_similarity(g1, g2, dim=0)
    print(f"ckpt on/off: loss {l1} vs {l2}, grad cosine {float(cos)}, "
          f"max abs diff {float((g1 - g2).abs().max()):.3e}")
    assert cos > 0.995, f"grad cosine {cos}"
