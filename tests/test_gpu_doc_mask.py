"""Document-boundary masking in the 32x32 attention kernels (the DOC builds of
attn_fwd32 / attn_bwd32_dq / attn_bwd32_dkv), called straight through the
extension: against the fp32 torch reference with the same mask at the
tolerances of test_gpu_attention.run_case, bit-exact absence of leakage
across a boundary, the one-document case against the plain kernels, argument
rejection, clamped tile ranges, and both model families end to end.

Inputs come from a CPU generator seeded from the case name, as in
test_gpu_attention_golden.py."""

import functools
import hashlib

import pytest
import torch

pytestmark = pytest.mark.gpu

# one-token document, boundary on a tile edge (64, 128), boundaries inside a
# wave (1, 198); the second row of a batch is a single document
MIXED = [[0, 1, 64, 128, 198], [0]]

# name: (B, S, H, Hkv, D, window, scale, starts per row)   scale None = D**-0.5
UNPACKED = {
    "d64_s256_mixed": (2, 256, 2, 1, 64, 0, None, MIXED),
    # a document across a block edge (0..299), a boundary on a block edge
    # (512), first kv tile > 0, shortened last q tile of dkv
    "d64_s768": (1, 768, 4, 2, 64, 0, None, [[0, 300, 512, 700]]),
    # window and document bound both active
    "d64_s512_w96": (1, 512, 2, 2, 64, 96, 1.0, [[0, 200, 260]]),
    # D=128: the dkv build without register-resident K/V
    "d128_s512": (1, 512, 2, 1, 128, 0, None, [[0, 70, 330]]),
}
# packed entry points at (B, S, H, Hkv) = (2, 256, 4, 2): (D, order, rope)
PACKED = {
    "packed_qkv_d64_rope": (64, "qkv", True),
    "packed_kvq_d128": (128, "kvq", False),
}
PACKED_BSHK = (2, 256, 4, 2)


def _gen(name):
    seed = int.from_bytes(hashlib.sha256(name.encode()).digest()[:4], "big")
    return torch.Generator().manual_seed(seed)


def _doc_arrays(starts, S):
    """int32 [B, S] doc_start / doc_end on the GPU from per-row start lists."""
    from acco_amd import ops
    ds = torch.zeros(len(starts), S, dtype=torch.int32)
    for b, row in enumerate(starts):
        for s0 in row:
            ds[b, s0:] = s0
    ds = ds.cuda()
    return ds, ops.doc_end_from_start(ds)


def _ext():
    from acco_amd import ops
    return ops.hip_ext()


def _run_unpacked(ext, q, k, v, dO, scale, window, ds=None, de=None):
    doc_f = () if ds is None else (ds,)
    doc_b = () if ds is None else (ds, de)
    outs = {}
    outs["o"], outs["lse"] = ext.attn_fwd(q, k, v, scale, window, *doc_f)
    outs["delta"] = ext.attn_delta(dO, outs["o"])
    outs["dq"], outs["dk"], outs["dv"] = ext.attn_bwd(
        q, k, v, dO, outs["lse"], outs["delta"], scale, window, *doc_b)
    return outs


def _inputs(name, B, S, H, Hkv, D):
    g = _gen(name)
    q = (torch.randn(B, S, H, D, generator=g) * 0.5).bfloat16().cuda()
    k = (torch.randn(B, S, Hkv, D, generator=g) * 0.5).bfloat16().cuda()
    v = (torch.randn(B, S, Hkv, D, generator=g) * 0.5).bfloat16().cuda()
    dO = torch.randn(B, S, H, D, generator=g).bfloat16().cuda()
    return q, k, v, dO


def _reference(q, k, v, dO, scale, window, ds):
    from acco_amd.ops import torch_ref
    q32, k32, v32 = (t.float().requires_grad_(True) for t in (q, k, v))
    o32 = torch_ref.causal_attention(q32, k32, v32, scale=scale,
                                     window=window or None, doc_start=ds)
    o32.backward(dO.float())
    return {"o": o32.detach(), "dq": q32.grad, "dk": k32.grad, "dv": v32.grad}


def _group_sum(t, Hkv):       # per-query-head grads -> kv heads, as AttentionFn
    B, S, H, D = t.shape
    return t.view(B, S, Hkv, H // Hkv, D).sum(3, dtype=torch.float32).bfloat16()


def _misses(got, refs):
    """Names of the outputs outside run_case's tolerances (o: 4e-2, grads:
    8e-2 absolute, 4e-2 relative), each with its max abs error."""
    bad = []
    for key, ref in refs.items():
        atol = 4e-2 if key == "o" else 8e-2
        err = (got[key].float() - ref).abs().max().item()
        print(f"{key}: max abs err {err:.3e}")
        if not torch.allclose(got[key].float(), ref, atol=atol, rtol=4e-2):
            bad.append(f"{key} (max abs err {err:.3e})")
    return bad


# ------------------------------------------------------ kernel vs reference
@pytest.mark.parametrize("name", list(UNPACKED))
def test_doc_kernels_match_reference(name):
    B, S, H, Hkv, D, window, scale, starts = UNPACKED[name]
    scale = D ** -0.5 if scale is None else scale
    q, k, v, dO = _inputs(name, B, S, H, Hkv, D)
    ds, de = _doc_arrays(starts, S)
    outs = _run_unpacked(_ext(), q, k, v, dO, scale, window, ds, de)
    torch.cuda.synchronize()
    assert torch.isfinite(outs["lse"]).all()
    got = {"o": outs["o"], "dq": outs["dq"],
           "dk": _group_sum(outs["dk"], Hkv), "dv": _group_sum(outs["dv"], Hkv)}
    assert not _misses(got, _reference(q, k, v, dO, scale, window, ds))


@pytest.mark.parametrize("name", list(PACKED))
def test_doc_packed_entry_points_match_reference(name):
    from acco_amd.ops import torch_ref
    ext = _ext()
    D, order, rope = PACKED[name]
    B, S, H, Hkv = PACKED_BSHK
    W = (H + 2 * Hkv) * D
    offs = ((0, H * D, (H + Hkv) * D) if order == "qkv"
            else (2 * Hkv * D, 0, Hkv * D))
    q_off, k_off, v_off = offs
    scale = D ** -0.5
    g = _gen("doc_" + name)
    qkv = (torch.randn(B, S, W, generator=g) * 0.5).bfloat16().cuda()
    dO = torch.randn(B, S, H * D, generator=g).bfloat16().cuda()
    ds, de = _doc_arrays(MIXED, S)
    cos = sin = None
    roped = qkv.clone()
    if rope:
        cos, sin = (t.cuda() for t in
                    torch_ref.rope_cos_sin(S, D, 10000.0, "cpu"))
        ext.rope_qk_inplace(roped, cos, sin, H, Hkv, D, q_off, k_off)
    o, lse = ext.attn_fwd_packed(roped, H, Hkv, D, scale, 0, *offs, ds)
    delta = ext.attn_delta(dO.view(B, S, H, D), o.view(B, S, H, D))
    dqkv = torch.zeros_like(qkv)
    dkq, dvq = ext.attn_bwd_packed(roped, dO, lse, delta, dqkv, H, Hkv, D,
                                   scale, 0, *offs, cos, sin, ds, de)
    if rope:
        ext.attn_gqa_reduce_rope(dkq, dvq, dqkv, cos, sin, Hkv, H // Hkv, D,
                                 k_off, v_off)
    else:
        ext.attn_gqa_reduce(dkq, dvq, dqkv, Hkv, H // Hkv, D, k_off, v_off)
    torch.cuda.synchronize()

    x = qkv.float().requires_grad_(True)
    q = x[..., q_off:q_off + H * D].reshape(B, S, H, D)
    k = x[..., k_off:k_off + Hkv * D].reshape(B, S, Hkv, D)
    v = x[..., v_off:v_off + Hkv * D].reshape(B, S, Hkv, D)
    if rope:
        q, k = torch_ref.rope_apply(q, k, cos, sin)
    o32 = torch_ref.causal_attention(q, k, v, scale=scale,
                                     doc_start=ds).reshape(B, S, H * D)
    o32.backward(dO.float())

    def sec(t, off, heads):
        return t[..., off:off + heads * D]

    got = {"o": o, "dq": sec(dqkv, q_off, H), "dk": sec(dqkv, k_off, Hkv),
           "dv": sec(dqkv, v_off, Hkv)}
    refs = {"o": o32.detach(), "dq": sec(x.grad, q_off, H),
            "dk": sec(x.grad, k_off, Hkv), "dv": sec(x.grad, v_off, Hkv)}
    assert not _misses(got, refs)


# ------------------------------------------------------- no leakage, exact
# Starts that are multiples of 32 and not of 64: no wave holds rows of two
# documents while tiles do. Masked scores are set to -1e30 before the row
# max and their probabilities are exact zeros, and the only wave-wide
# decision (the defer-max __all) then sees one document per wave, so nothing
# of another document can reach a bit of the result.
LEAK_STARTS = [[0, 96, 224, 416]]
CUT = 224


@functools.lru_cache(maxsize=None)
def _leak_base():
    B, S, H, Hkv, D = 1, 512, 2, 1, 64
    q, k, v, dO = _inputs("leak", B, S, H, Hkv, D)
    ds, de = _doc_arrays(LEAK_STARTS, S)
    outs = _run_unpacked(_ext(), q, k, v, dO, D ** -0.5, 0, ds, de)
    return (q, k, v, dO, ds, de), outs


def test_no_leak_into_later_documents():
    (q, k, v, dO, ds, de), base = _leak_base()
    g = _gen("leak_before")
    q2, k2, v2 = q.clone(), k.clone(), v.clone()
    for t in (q2, k2, v2):
        t[:, :CUT] = torch.randn(t[:, :CUT].shape, generator=g).bfloat16().cuda()
    outs = _run_unpacked(_ext(), q2, k2, v2, dO, 64 ** -0.5, 0, ds, de)
    torch.cuda.synchronize()
    assert torch.equal(outs["o"][:, CUT:], base["o"][:, CUT:])
    assert torch.equal(outs["lse"][..., CUT:], base["lse"][..., CUT:])
    assert torch.equal(outs["dq"][:, CUT:], base["dq"][:, CUT:])


def test_no_leak_into_earlier_documents():
    (q, k, v, dO, ds, de), base = _leak_base()
    g = _gen("leak_after")
    q2, dO2 = q.clone(), dO.clone()
    for t in (q2, dO2):
        t[:, CUT:] = torch.randn(t[:, CUT:].shape, generator=g).bfloat16().cuda()
    outs = _run_unpacked(_ext(), q2, k, v, dO2, 64 ** -0.5, 0, ds, de)
    torch.cuda.synchronize()
    assert torch.equal(outs["dk"][:, :CUT], base["dk"][:, :CUT])
    assert torch.equal(outs["dv"][:, :CUT], base["dv"][:, :CUT])


# ------------------------------------- one document: DOC path == plain path
@pytest.mark.parametrize("D", [64, 128])
def test_one_document_equals_plain_kernels(D):
    B, S, H, Hkv = 1, 512, 2, 1
    q, k, v, dO = _inputs(f"one_doc_{D}", B, S, H, Hkv, D)
    ds, de = _doc_arrays([[0]], S)
    assert int(de.min()) == S
    ext = _ext()
    plain = _run_unpacked(ext, q, k, v, dO, D ** -0.5, 0)
    doc = _run_unpacked(ext, q, k, v, dO, D ** -0.5, 0, ds, de)
    torch.cuda.synchronize()
    got = {"o": doc["o"], "dq": doc["dq"], "dk": _group_sum(doc["dk"], Hkv),
           "dv": _group_sum(doc["dv"], Hkv)}
    assert not _misses(got, _reference(q, k, v, dO, D ** -0.5, 0, None))
    # same tiles, same order, same arithmetic: only the predicates differ
    same = {key: torch.equal(doc[key], plain[key]) for key in plain}
    print("bit-identical to the plain kernels:", same)
    assert all(same.values()), same


# ---------------------------------------------------------------- rejection
def _bf16(*shape):
    return torch.zeros(*shape, dtype=torch.bfloat16, device="cuda")


def _rej_fwd(S=256, doc_S=None, dtype=torch.int32, device="cuda",
             scale=0.125):
    def call(ext):
        q = _bf16(1, S, 2, 64)
        doc = torch.zeros(1, doc_S or S, dtype=dtype, device=device)
        return ext.attn_fwd(q, q, q, scale, 0, doc)
    return call


def _rej_bwd(with_start):
    def call(ext):
        q = _bf16(1, 256, 2, 64)
        stat = torch.zeros(1, 2, 256, device="cuda")
        doc = torch.zeros(1, 256, dtype=torch.int32, device="cuda")
        return ext.attn_bwd(q, q, q, q, stat, stat, 0.125, 0,
                            doc if with_start else None,
                            None if with_start else doc)
    return call


def _rej_packed(bwd, **bad):
    def call(ext):
        B, S, H, Hkv, D = 1, 256, 2, 1, 64
        qkv = _bf16(B, S, (H + 2 * Hkv) * D)
        offs = (0, H * D, (H + Hkv) * D)
        doc = torch.zeros(B, S, dtype=torch.int32, device="cuda")
        wrong = torch.zeros(B, bad.get("doc_S", S),
                            dtype=bad.get("dtype", torch.int32), device="cuda")
        if not bwd:
            return ext.attn_fwd_packed(qkv, H, Hkv, D, 0.125, 0, *offs, wrong)
        stat = torch.zeros(B, H, S, device="cuda")
        return ext.attn_bwd_packed(qkv, _bf16(B, S, H * D), stat, stat,
                                   torch.zeros_like(qkv), H, Hkv, D, 0.125, 0,
                                   *offs, None, None, doc, wrong)
    return call


REJECTED = {
    "fwd_doc_start_int64": _rej_fwd(dtype=torch.int64),
    "fwd_doc_start_one_short": _rej_fwd(doc_S=255),
    "fwd_doc_start_on_cpu": _rej_fwd(device="cpu"),
    "fwd_S192_with_doc_start": _rej_fwd(S=192),
    "fwd_scale_zero_with_doc_start": _rej_fwd(scale=0.0),
    "bwd_doc_end_without_doc_start": _rej_bwd(with_start=False),
    "bwd_doc_start_without_doc_end": _rej_bwd(with_start=True),
    "fwd_packed_doc_start_int64": _rej_packed(False, dtype=torch.int64),
    "bwd_packed_doc_end_one_short": _rej_packed(True, doc_S=255),
}


@pytest.mark.parametrize("name", list(REJECTED))
def test_doc_binding_rejects(name):
    with pytest.raises(RuntimeError):
        REJECTED[name](_ext())
    torch.cuda.synchronize()        # nothing was launched, nothing faulted


def test_autograd_functions_reject_one_array_alone():
    from acco_amd.ops.autograd import AttentionFn
    q = _bf16(1, 256, 2, 64)
    doc = torch.zeros(1, 256, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError):
        AttentionFn.apply(q, q, q, None, None, doc, None)


# ------------------------------------------------------------ bounds safety
# The arrays are data: every tile index derived from them is clamped into
# [0, S/64 - 1] (attn::clamp_tile via kv_tile_lo_doc / q_tile_hi_doc), the
# values themselves are only compared, and the arrays are indexed by
# position, never by content. Wrong content gives wrong numbers, not wrong
# addresses.
@pytest.mark.parametrize("fill", ["past_the_end", "negative", "alternating"])
def test_wrong_doc_arrays_stay_in_bounds(fill):
    B, S, H, Hkv, D = 1, 512, 2, 1, 64
    q, k, v, dO = _inputs("bounds", B, S, H, Hkv, D)
    ds = torch.full((B, S), S + 1000, dtype=torch.int32)
    if fill == "negative":
        ds.fill_(-5)
    elif fill == "alternating":
        ds[:, ::2] = -5
    ds = ds.cuda()
    outs = _run_unpacked(_ext(), q, k, v, dO, D ** -0.5, 0, ds, ds.clone())
    torch.cuda.synchronize()
    assert outs["o"].shape == q.shape and outs["dq"].shape == q.shape
    assert outs["dk"].shape == q.shape and outs["dv"].shape == q.shape
    assert outs["lse"].shape == (B, H, S)


# --------------------------------------------------------------- full model
def _ids_with_eos(B, S, vocab, eos, ends, seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(eos + 1, vocab, (B, S), generator=g)
    for b, row in enumerate(ends):
        for e in row:
            ids[b, e] = eos
    return ids


def _model_gpu_vs_cpu(make, fused, S=256):
    from acco_amd import ops
    from acco_amd.engine import arena
    from acco_amd.models.fuse import install_fused_projections
    eos = 0
    # documents end inside a wave, on a tile edge and at the row's end
    ids = _ids_with_eos(2, S, 512, eos, [[0, 63, 127, 197], [S - 1]], seed=11)
    ds = ops.doc_start_from_eos(ids, eos)
    assert ds.unique().numel() == 5

    torch.manual_seed(0)
    m_cpu = make()
    torch.manual_seed(0)
    m_gpu = make()
    cpu, dev = torch.device("cpu"), torch.device("cuda")
    arena.flatten_params(m_cpu, torch.float32, cpu, pad_to=256)
    g_cpu = arena.attach_grad_arena(m_cpu, torch.float32, cpu, pad_to=256)
    p_gpu = arena.flatten_params(m_gpu, torch.bfloat16, dev, pad_to=256)
    g_gpu = arena.attach_grad_arena(m_gpu, torch.bfloat16, dev, pad_to=256)
    if fused:
        assert install_fused_projections(m_gpu, p_gpu, g_gpu) > 0

    loss_c, _ = m_cpu(ids, labels=ids, doc_start=ds)
    loss_c.backward()
    loss_g, _ = m_gpu(ids.cuda(), labels=ids.cuda(), doc_start=ds.cuda())
    loss_g.backward()
    torch.cuda.synchronize()
    # and the mask reaches the GPU path: without it the loss is another one
    with torch.no_grad():
        loss_plain = float(m_cpu(ids, labels=ids)[0])
    n = arena.live_numel(m_cpu)
    loss_c, loss_g = float(loss_c.detach()), float(loss_g.detach())
    cos = torch.nn.functional.cosine_similarity(
        g_cpu[:n], g_gpu[:n].float().cpu(), dim=0)
    print(f"loss cpu {loss_c:.5f} gpu {loss_g:.5f} unmasked {loss_plain:.5f} "
          f"grad cosine {float(cos):.5f}")
    assert abs(loss_c - loss_g) / max(abs(loss_c), 1e-6) < 0.05
    assert cos > 0.98, f"grad cosine {cos}"


@pytest.mark.parametrize("fused", [True, False])
def test_llama_doc_mask_gpu_vs_cpu(fused):
    from acco_amd.models import LlamaConfig, LlamaForCausalLM
    # the smoke() model; S=256 and fused projections: the packed path
    cfg = LlamaConfig(hidden_size=256, num_layers=2, num_heads=4,
                      num_kv_heads=2, intermediate_size=512, vocab_size=1024,
                      max_position_embeddings=512)
    _model_gpu_vs_cpu(lambda: LlamaForCausalLM(cfg), fused)


@pytest.mark.parametrize("fused", [True, False])
def test_gptneo_doc_mask_gpu_vs_cpu(fused):
    from acco_amd.models import GPTNeoConfig, GPTNeoForCausalLM
    cfg = GPTNeoConfig(hidden_size=128, num_layers=2, num_heads=2,
                       vocab_size=512, max_position_embeddings=256,
                       window_size=32)
    _model_gpu_vs_cpu(lambda: GPTNeoForCausalLM(cfg), fused)
