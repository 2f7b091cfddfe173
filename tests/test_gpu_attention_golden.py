"""Every attention kernel instantiation and tile-range edge, called straight
through the extension: each output against the fp32 torch reference
(tolerances of test_gpu_attention.run_case) AND bit for bit against sha256
prefixes recorded from the build named in golden/attention_parent.json, i.e.
the attention kernels before their shared code moved into
csrc/attention_common.h.

Inputs come from a CPU generator seeded from the case name, so the hashes do
not depend on the device RNG; the attention kernels hold no atomics, so the
outputs are run-to-run deterministic.

The second half checks that the bindings turn wrong arguments into a
RuntimeError instead of a launch."""

import hashlib
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "attention_parent.json")

# name: (B, S, H, Hkv, D, window, scale)   scale None = D ** -0.5
# S % 256 != 0 -> the 16x16 kernels <D, QW>; QW = 32 when S % 128 == 0, D = 64
UNPACKED = {
    "d64_s64": (2, 64, 2, 1, 64, 0, None),        # QW16, one tile, b/GQA index
    "d64_s192": (1, 192, 4, 2, 64, 0, None),      # QW16, three blocks
    "d64_s192_w64": (1, 192, 2, 2, 64, 64, 1.0),  # QW16, j_lo > 0, GPT-Neo
    "d64_s128": (1, 128, 2, 2, 64, 0, None),      # QW32, one block
    "d64_s384_w96": (1, 384, 2, 1, 64, 96, None),  # QW32, j_lo>0, clipped qt_hi
    "d128_s64": (1, 64, 2, 1, 128, 0, None),      # D128 QW16
    "d128_s192_w64": (1, 192, 2, 1, 128, 64, None),   # D128, window
    # S % 256 == 0 -> the 32x32 kernels <D>
    "d64_s256": (2, 256, 2, 1, 64, 0, None),      # one block, per-wave skip
    "d64_s768": (1, 768, 2, 2, 64, 0, None),      # three blocks, interior tiles
    "d64_s512_w96": (1, 512, 4, 2, 64, 96, None),  # j_lo>0, window skip, qt_hi
    "d64_s512_w64": (1, 512, 2, 2, 64, 64, 1.0),  # GPT-Neo scaling
    "d128_s256": (1, 256, 2, 1, 128, 0, None),    # D128, non-resident K/V dkv
    "d128_s512_w96": (1, 512, 2, 2, 128, 96, None),   # D128, window
}

# packed entry points, B = 2 (batch stride over W): name: (D, order, rope)
PACKED = {
    "packed_qkv_d64_rope": (64, "qkv", True),
    "packed_kvq_d128": (128, "kvq", False),
}
PACKED_BSHK = (2, 256, 4, 2)

CASES = list(UNPACKED) + list(PACKED)


def _sha(t):
    raw = t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()
    return hashlib.sha256(raw).hexdigest()[:16]


def _gen(name):
    seed = int.from_bytes(hashlib.sha256(name.encode()).digest()[:4], "big")
    return torch.Generator().manual_seed(seed)


def _unpacked_case(name, ext):
    from acco_amd.ops import torch_ref
    B, S, H, Hkv, D, window, scale = UNPACKED[name]
    scale = D ** -0.5 if scale is None else scale
    g = _gen(name)
    q = (torch.randn(B, S, H, D, generator=g) * 0.5).bfloat16().cuda()
    k = (torch.randn(B, S, Hkv, D, generator=g) * 0.5).bfloat16().cuda()
    v = (torch.randn(B, S, Hkv, D, generator=g) * 0.5).bfloat16().cuda()
    dO = torch.randn(B, S, H, D, generator=g).bfloat16().cuda()

    outs = {}
    outs["o"], outs["lse"] = ext.attn_fwd(q, k, v, scale, window)
    outs["delta"] = ext.attn_delta(dO, outs["o"])
    outs["dq"], outs["dk"], outs["dv"] = ext.attn_bwd(
        q, k, v, dO, outs["lse"], outs["delta"], scale, window)

    q32, k32, v32 = (t.float().requires_grad_(True) for t in (q, k, v))
    o32 = torch_ref.causal_attention(q32, k32, v32, scale=scale,
                                     window=window or None)
    o32.backward(dO.float())

    def group_sum(t):        # per-query-head grads -> kv heads, as AttentionFn
        return t.view(B, S, Hkv, H // Hkv, D).sum(
            3, dtype=torch.float32).bfloat16()

    got = {"o": outs["o"], "dq": outs["dq"], "dk": group_sum(outs["dk"]),
           "dv": group_sum(outs["dv"])}
    refs = {"o": o32.detach(), "dq": q32.grad, "dk": k32.grad, "dv": v32.grad}
    return outs, got, refs


def _packed_case(name, ext):
    from acco_amd.ops import torch_ref
    D, order, rope = PACKED[name]
    B, S, H, Hkv = PACKED_BSHK
    W = (H + 2 * Hkv) * D
    offs = ((0, H * D, (H + Hkv) * D) if order == "qkv"
            else (2 * Hkv * D, 0, Hkv * D))
    q_off, k_off, v_off = offs
    scale = D ** -0.5
    g = _gen(name)
    qkv = (torch.randn(B, S, W, generator=g) * 0.5).bfloat16().cuda()
    dO = torch.randn(B, S, H * D, generator=g).bfloat16().cuda()
    cos = sin = None
    roped = qkv.clone()
    if rope:
        cos, sin = (t.cuda() for t in
                    torch_ref.rope_cos_sin(S, D, 10000.0, "cpu"))
        ext.rope_qk_inplace(roped, cos, sin, H, Hkv, D, q_off, k_off)

    outs = {}
    outs["o"], outs["lse"] = ext.attn_fwd_packed(roped, H, Hkv, D, scale, 0,
                                                 *offs)
    delta = ext.attn_delta(dO.view(B, S, H, D), outs["o"].view(B, S, H, D))
    dqkv = torch.zeros_like(qkv)
    outs["dkq"], outs["dvq"] = ext.attn_bwd_packed(
        roped, dO, outs["lse"], delta, dqkv, H, Hkv, D, scale, 0, *offs, cos,
        sin)
    outs["dq"] = dqkv[..., q_off:q_off + H * D].clone()
    # group-summed dk/dv (inverse RoPE folded in) into the k|v sections
    if rope:
        ext.attn_gqa_reduce_rope(outs["dkq"], outs["dvq"], dqkv, cos, sin,
                                 Hkv, H // Hkv, D, k_off, v_off)
    else:
        ext.attn_gqa_reduce(outs["dkq"], outs["dvq"], dqkv, Hkv, H // Hkv, D,
                            k_off, v_off)

    x = qkv.float().requires_grad_(True)
    q = x[..., q_off:q_off + H * D].reshape(B, S, H, D)
    k = x[..., k_off:k_off + Hkv * D].reshape(B, S, Hkv, D)
    v = x[..., v_off:v_off + Hkv * D].reshape(B, S, Hkv, D)
    if rope:
        q, k = torch_ref.rope_apply(q, k, cos, sin)
    o32 = torch_ref.causal_attention(q, k, v, scale=scale).reshape(B, S, H * D)
    o32.backward(dO.float())

    def sec(t, off, heads):
        return t[..., off:off + heads * D]

    got = {"o": outs["o"], "dq": sec(dqkv, q_off, H),
           "dk": sec(dqkv, k_off, Hkv), "dv": sec(dqkv, v_off, Hkv)}
    refs = {"o": o32.detach(), "dq": sec(x.grad, q_off, H),
            "dk": sec(x.grad, k_off, Hkv), "dv": sec(x.grad, v_off, Hkv)}
    return outs, got, refs


def attn_case(name):
    """Run one case through the extension; returns (outs, got, refs): the
    raw kernel outputs that are hashed, and o / dq / group-summed dk / dv
    next to their fp32 references. Module-level so the hashes can be
    recorded with the same inputs from any build."""
    from acco_amd import ops
    ext = ops.hip_ext()
    if name in UNPACKED:
        return _unpacked_case(name, ext)
    return _packed_case(name, ext)


def check_against_reference(got, refs):
    """Names of the outputs that miss run_case's tolerances."""
    bad = []
    for key, ref in refs.items():
        atol = 4e-2 if key == "o" else 8e-2
        if not torch.allclose(got[key].float(), ref, atol=atol, rtol=4e-2):
            err = (got[key].float() - ref).abs().max().item()
            bad.append(f"{key} (max abs err {err:.3e})")
    return bad


@pytest.mark.parametrize("name", CASES)
def test_attention_matches_reference_and_parent(name):
    outs, got, refs = attn_case(name)
    assert not check_against_reference(got, refs)
    with open(GOLDEN) as f:
        gold = json.load(f)["cases"][name]
    assert {k: _sha(v) for k, v in outs.items()} == gold


# ---------------------------------------------------------------- rejection
def _bf16(*shape, device="cuda"):
    return torch.zeros(*shape, dtype=torch.bfloat16, device=device)


def _fwd(B=1, S=64, H=2, Hkv=1, D=64, k_S=None, k_device="cuda"):
    return lambda ext: ext.attn_fwd(
        _bf16(B, S, H, D), _bf16(B, k_S or S, Hkv, D, device=k_device),
        _bf16(B, k_S or S, Hkv, D, device=k_device), D ** -0.5, 0)


def _bwd(lse_dtype=torch.float32, delta_short=0, dO_rows=64):
    B, S, H, D = 1, 64, 2, 64

    def call(ext):
        q = _bf16(B, S, H, D)
        lse = torch.zeros(B, H, S, dtype=lse_dtype, device="cuda")
        delta = torch.zeros(B * H * S - delta_short, device="cuda")
        return ext.attn_bwd(q, q, q, _bf16(B, dO_rows, H, D), lse, delta,
                            D ** -0.5, 0)
    return call


def _packed(S=256, W=None, offs=None, dqkv_shape=None, cos=None, sin=None,
            bwd=False):
    B, H, Hkv, D = 1, 2, 1, 64
    W = W or (H + 2 * Hkv) * D
    offs = offs or (0, H * D, (H + Hkv) * D)

    def call(ext):
        qkv = _bf16(B, S, W)
        if not bwd:
            return ext.attn_fwd_packed(qkv, H, Hkv, D, D ** -0.5, 0, *offs)
        stat = torch.zeros(B, H, S, device="cuda")
        tables = [None if t is None else
                  torch.zeros(*t, device="cuda") for t in (cos, sin)]
        return ext.attn_bwd_packed(qkv, _bf16(B, S, H * D), stat, stat,
                                   _bf16(*(dqkv_shape or (B, S, W))), H, Hkv,
                                   D, D ** -0.5, 0, *offs, *tables)
    return call


def _delta(ext):
    return ext.attn_delta(_bf16(1, 64, 2, 64), _bf16(1, 64, 2, 128))


def _gqa_reduce(ext):
    # W = 256, Hkv*D = 64: a k section at 256 lies beyond the row
    return ext.attn_gqa_reduce(_bf16(1, 64, 2, 64), _bf16(1, 64, 2, 64),
                               _bf16(1, 64, 256), 1, 2, 64, 256, 192)


REJECTED = {
    "fwd_S96": _fwd(S=96),
    "fwd_D32": _fwd(D=32),
    "fwd_H3_Hkv2": _fwd(H=3, Hkv=2),
    "fwd_k_other_S": _fwd(k_S=128),
    "fwd_k_on_cpu": _fwd(k_device="cpu"),
    "bwd_lse_fp64": _bwd(lse_dtype=torch.float64),
    "bwd_delta_one_short": _bwd(delta_short=1),
    "bwd_dO_wrong_numel": _bwd(dO_rows=128),
    "fwd_packed_S128": _packed(S=128),
    "fwd_packed_q_off_4": _packed(W=264, offs=(4, 136, 200)),
    "fwd_packed_v_past_W": _packed(offs=(0, 128, 200)),
    "fwd_packed_q_k_overlap": _packed(W=512, offs=(0, 64, 256)),
    "bwd_packed_dqkv_other_shape": _packed(bwd=True, dqkv_shape=(1, 256, 512)),
    "bwd_packed_cos_without_sin": _packed(bwd=True, cos=(256, 64)),
    "bwd_packed_empty_cos": _packed(bwd=True, cos=(0,), sin=(0,)),
    "delta_o_other_shape": _delta,
    "gqa_reduce_k_off_past_W": _gqa_reduce,
}


@pytest.mark.parametrize("name", list(REJECTED))
def test_attention_binding_rejects(name):
    from acco_amd import ops
    with pytest.raises(RuntimeError):
        REJECTED[name](ops.hip_ext())
    torch.cuda.synchronize()        # nothing was launched, nothing faulted
