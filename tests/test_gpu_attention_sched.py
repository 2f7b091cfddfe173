"""The order in which the attention grids' workgroups take their (row block,
head): attn::block_order in csrc/attention_common.h, the one function all six
kernels and the attn_block_order binding call.

First half, on the host: the order is a permutation, heaviest first within
every class id % 8 (the workgroups that share an XCD) and balanced across the
classes. These need the built extension and no GPU. The order does not
depend on H / Hkv: a variant that kept the query heads of one kv group in one
class was measured and not kept (RESULTS.md), so there is no such path to
check and no sweep over the group size.

Second half, on the GPU: grids beyond the few blocks of
test_gpu_attention_golden.py, each output against the fp32 torch reference
(the tolerances of test_gpu_attention.run_case) AND bit for bit against
sha256 prefixes recorded with these same inputs from the build named in
golden/attention_sched_parent.json, i.e. the kernels on their 2-D grid before
block_order. A block that no workgroup visits, or that two visit with
different heads, cannot pass both.
"""

import hashlib
import json
import os

import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "attention_sched_parent.json")


# ------------------------------------------------------------------ the order
@pytest.fixture(scope="module")
def ext():
    from acco_amd import ops
    return ops.hip_ext()


def _order(ext, n_blk, BH, heavy_last):
    # B = 1: only B * H enters the order
    return ext.attn_block_order(n_blk, 1, BH, heavy_last).tolist()


def _grids():
    for BH in range(1, 71):
        for n_blk in range(1, 17):
            for heavy_last in (True, False):
                yield n_blk, BH, heavy_last


def _cost(row_block, n_blk, heavy_last):
    return row_block + 1 if heavy_last else n_blk - row_block


def test_order_is_a_permutation(ext):
    for n_blk, BH, heavy_last in _grids():
        got = _order(ext, n_blk, BH, heavy_last)
        want = [[rb, bh] for rb in range(n_blk) for bh in range(BH)]
        assert sorted(got) == want, (n_blk, BH, heavy_last)


def test_each_class_runs_heaviest_first(ext):
    for n_blk, BH, heavy_last in _grids():
        order = _order(ext, n_blk, BH, heavy_last)
        for c in range(8):
            costs = [_cost(rb, n_blk, heavy_last) for rb, _ in order[c::8]]
            assert costs == sorted(costs, reverse=True), \
                (n_blk, BH, heavy_last, c)


def test_class_cost_sums_are_balanced(ext):
    for n_blk, BH, heavy_last in _grids():
        order = _order(ext, n_blk, BH, heavy_last)
        sums = [sum(_cost(rb, n_blk, heavy_last) for rb, _ in order[c::8])
                for c in range(8)]
        assert max(sums) - min(sums) <= n_blk, (n_blk, BH, heavy_last)
        if BH % 8 == 0:
            assert max(sums) == min(sums), (n_blk, BH, heavy_last)


def test_flagship_grid_is_exactly_balanced(ext):
    # b8 s1024 H32: every class gets 32 blocks of each of the 4 levels
    for heavy_last in (True, False):
        order = ext.attn_block_order(4, 8, 32, heavy_last).tolist()
        for c in range(8):
            rbs = [rb for rb, _ in order[c::8]]
            assert [rbs.count(r) for r in range(4)] == [32] * 4


def test_block_order_binding_rejects(ext):
    for args in ((0, 1, 8, True), (4, 1, 0, True), (4, 0, 8, True),
                 (4, 70000, 1, True), (1 << 20, 64, 1000, False)):
        with pytest.raises(RuntimeError):
            ext.attn_block_order(*args)


# ----------------------------------------------------------------- the grids
# name: (B, S, H, Hkv, D, window); scale = D ** -0.5
UNPACKED = {
    # 32x32 kernels (S % 256 == 0), 256-row blocks
    "s1024_b2_h8_kv2": (2, 1024, 8, 2, 64, 0),   # 64 blocks, 4 levels
    "s512_b4_h8_kv2": (4, 512, 8, 2, 64, 0),     # 64 blocks, B*Hkv = 8
    "s768_h3": (1, 768, 3, 3, 64, 0),            # 9 blocks, no multiple of 8
    "s512_h8_d128": (1, 512, 8, 8, 128, 0),      # D128
    "s768_h4_kv2_w96": (1, 768, 4, 2, 64, 96),   # window
    # 16x16 kernels
    "s320_h3_kv1": (1, 320, 3, 1, 64, 0),        # QW16, 5 levels, 15 blocks
    "s384_b2_h4_kv2": (2, 384, 4, 2, 64, 0),     # QW32, 24 blocks
}
# packed entry points: (B, S, H, Hkv, D), q|k|v with RoPE
PACKED = {"packed_s512_b4_h8_kv2_rope": (4, 512, 8, 2, 64)}

CASES = list(UNPACKED) + list(PACKED)


def _sha(t):
    raw = t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()
    return hashlib.sha256(raw).hexdigest()[:16]


def _gen(name):
    seed = int.from_bytes(hashlib.sha256(name.encode()).digest()[:4], "big")
    return torch.Generator().manual_seed(seed)


def _unpacked_case(name, ext):
    from acco_amd.ops import torch_ref
    B, S, H, Hkv, D, window = UNPACKED[name]
    scale = D ** -0.5
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
    B, S, H, Hkv, D = PACKED[name]
    W = (H + 2 * Hkv) * D
    offs = (0, H * D, (H + Hkv) * D)
    q_off, k_off, v_off = offs
    scale = D ** -0.5
    g = _gen(name)
    qkv = (torch.randn(B, S, W, generator=g) * 0.5).bfloat16().cuda()
    dO = torch.randn(B, S, H * D, generator=g).bfloat16().cuda()
    cos, sin = (t.cuda() for t in torch_ref.rope_cos_sin(S, D, 10000.0, "cpu"))
    roped = qkv.clone()
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
    ext.attn_gqa_reduce_rope(outs["dkq"], outs["dvq"], dqkv, cos, sin, Hkv,
                             H // Hkv, D, k_off, v_off)

    x = qkv.float().requires_grad_(True)
    q = x[..., q_off:q_off + H * D].reshape(B, S, H, D)
    k = x[..., k_off:k_off + Hkv * D].reshape(B, S, Hkv, D)
    v = x[..., v_off:v_off + Hkv * D].reshape(B, S, Hkv, D)
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


def sched_case(name):
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


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_grid_matches_reference_and_parent(name):
    outs, got, refs = sched_case(name)
    assert not check_against_reference(got, refs)
    with open(GOLDEN) as f:
        gold = json.load(f)["cases"][name]
    assert {k: _sha(v) for k, v in outs.items()} == gold
