"""The chunked lm_head + loss (ops.linear_causal_lm_loss, ce.hip rows) on the
GPU against fp64, next to the unfused path (F.linear + ops.causal_lm_loss /
label_smoothed_causal_lm_loss) on the same inputs.

Criterion: the fp64 reference is computed on the CPU from the same bf16
hidden, weight and labels. Both GPU paths round their logits to bf16, which
dominates their error, and hipBLASLt may pick another solution per M (the
chunk size), so the chunked path's error is a second draw of the same noise:
its loss, dh and dW may err by at most 2x the unfused path's own largest
error on that case. With a grad-arena destination dW is rounded to bf16 once
per chunk, which adds n_chunks · 0.5 · ulp_bf16(|ref|) per entry.

Worst fused-error / allowed-error ratios measured on an MI355X (the RATIO
lines of this module; 0.5 means the two paths err alike):
    loss 0.5000, dh 0.5000, dW through autograd 0.5000 (dh and dW came out
    bit-equal to the unfused path at every chunk size), dW into a grad view
    0.5146 (V = 1000, 8 chunks), model on the arena: lm_head.weight 0.5761,
    every other gradient <= 0.5843 (tied) / 0.5000 (untied).

Also here: the peak memory of forward + backward stays below one full logits
tensor, a tiny Llama on the grad arena with `fused_lm_loss` on against off,
and the loss is bitwise reproducible."""

import functools

import pytest
import torch
import torch.nn.functional as F

from tests import streaming_ref as sr

pytestmark = pytest.mark.gpu

UPSTREAM = 0.37
SHAPES = [(2, 64, 64, 1000), (1, 48, 64, 50257)]
CHUNKS = [16, 40, 4096]


def _inputs(shape):
    B, S, H, V = shape
    g = sr.case_generator("fused_lm_loss_%dx%dx%dx%d" % shape)
    hidden = torch.randn(B, S, H, generator=g).bfloat16()
    weight = (torch.randn(V, H, generator=g) * H ** -0.5).bfloat16()
    labels = torch.randint(0, V, (B, S), generator=g)
    labels[torch.rand(B, S, generator=g) < 0.2] = -100
    labels[0, 1], labels[0, 2] = 0, V - 1
    return hidden, weight, labels


def _loss64(logits, labels, eps):
    V = logits.shape[-1]
    sl = logits[:, :-1].reshape(-1, V)
    lab = labels[:, 1:].reshape(-1)
    valid = lab >= 0
    lse = torch.logsumexp(sl, -1)
    tok = lse - sl.gather(1, lab.clamp(min=0)[:, None]).squeeze(1)
    if eps != 0.0:
        tok = (1.0 - eps) * tok + eps * (lse - sl.sum(-1) / V)
    return torch.where(valid, tok, torch.zeros_like(tok)).sum() / \
        max(int(valid.sum()), 1)


@functools.lru_cache(maxsize=None)
def _reference(shape, eps):
    """fp64 (loss, dh, dW) on the CPU and the unfused GPU path's (loss, dh,
    dW), both from the same bf16 inputs; computed once per case."""
    from acco_amd import ops
    hidden, weight, labels = _inputs(shape)
    h = hidden.double().requires_grad_(True)
    w = weight.double().requires_grad_(True)
    loss = _loss64(F.linear(h, w), labels, eps)
    (loss * UPSTREAM).backward()
    ref = (loss.detach(), h.grad, w.grad)

    hg = hidden.cuda().requires_grad_(True)
    wg = weight.cuda().requires_grad_(True)
    lg = ops.label_smoothed_causal_lm_loss(F.linear(hg, wg), labels.cuda(),
                                           eps)
    (lg * UPSTREAM).backward()
    unfused = (lg.detach().cpu(), hg.grad.cpu(), wg.grad.cpu())
    return ref, unfused


def _err(got, ref64):
    return float((got.double().cpu() - ref64).abs().max())


def _compare(what, got, unfused, ref64, extra=None):
    """got within 2x the unfused path's largest error (+ extra per entry)."""
    base = 2.0 * _err(unfused, ref64)
    limit = torch.full_like(ref64, base)
    if extra is not None:
        limit = limit + extra
    err = (got.double().cpu() - ref64).abs()
    ratio = float((err / limit).max()) if base > 0 else float(err.max() > 0)
    print(f"RATIO {what} fused_err {float(err.max()):.3e} unfused_err "
          f"{base / 2:.3e} ratio {ratio:.4f}")
    assert ratio <= 1.0, (
        f"{what}: fused err {float(err.max()):.3e} > allowed (2x unfused "
        f"{base / 2:.3e}), ratio {ratio:.4f}")


@pytest.mark.parametrize("arena", [False, True], ids=["autograd", "grad_view"])
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("shape", SHAPES, ids=["V1000", "V50257"])
def test_against_fp64(shape, chunk, eps, arena):
    from acco_amd import ops
    B, S, H, V = shape
    (loss64, dh64, dw64), (loss_u, dh_u, dw_u) = _reference(shape, eps)
    hidden, weight, labels = _inputs(shape)
    h = hidden.cuda().requires_grad_(True)
    w = weight.cuda().requires_grad_(True)
    view = torch.zeros(V, H, device="cuda", dtype=torch.bfloat16) \
        if arena else None
    loss = ops.linear_causal_lm_loss(h, w, labels.cuda(), eps, chunk,
                                     grad_view=view)
    assert loss.dtype == torch.float32 and loss.shape == ()
    (loss * UPSTREAM).backward()
    what = "V%d_chunk%d_eps%g_%s" % (V, chunk, eps,
                                     "grad_view" if arena else "autograd")
    _compare(f"loss {what}", loss.detach().reshape(1), loss_u.reshape(1),
             loss64.reshape(1))
    _compare(f"dh {what}", h.grad, dh_u, dh64)
    if arena:
        assert w.grad is None
        n_chunks = -(-(B * S) // min(chunk, B * S))
        _compare(f"dW {what}", view, dw_u, dw64,
                 extra=n_chunks * 0.5 * sr.ulp_bf16(dw64))
    else:
        assert w.grad.dtype == torch.bfloat16
        _compare(f"dW {what}", w.grad, dw_u, dw64)
    # bitwise reproducible
    again = ops.linear_causal_lm_loss(hidden.cuda(), weight.cuda(),
                                      labels.cuda(), eps, chunk)
    assert torch.equal(again, loss.detach())


def test_gpu_contract():
    from acco_amd import ops
    hidden, weight, labels = (t.cuda() for t in _inputs(SHAPES[0]))
    with pytest.raises(RuntimeError):
        ops.linear_causal_lm_loss(hidden.float(), weight.float(), labels)
    with pytest.raises(RuntimeError):
        ops.linear_causal_lm_loss(hidden, weight.t().contiguous().t(), labels)
    with pytest.raises(ValueError):
        ops.linear_causal_lm_loss(hidden, weight, labels, chunk_tokens=0)


# -------------------------------------------------------------------- memory
def test_peak_memory_below_one_logits_tensor():
    from acco_amd import ops
    B, S, H, V, chunk = 2, 2048, 256, 8192, 256
    T = B * S
    g = sr.case_generator("fused_lm_loss_memory")
    hidden = torch.randn(B, S, H, generator=g).bfloat16().cuda()
    weight = (torch.randn(V, H, generator=g) * H ** -0.5).bfloat16().cuda()
    labels = torch.randint(0, V, (B, S), generator=g).cuda()
    hidden.requires_grad_(True)
    weight.requires_grad_(True)

    def peak(fn):
        hidden.grad = weight.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        loss = fn()
        loss.backward()
        torch.cuda.synchronize()
        used = torch.cuda.max_memory_allocated() - before
        del loss
        return used

    full = T * V * 2
    fused = peak(lambda: ops.linear_causal_lm_loss(hidden, weight, labels,
                                                   0.0, chunk))
    unfused = peak(lambda: ops.causal_lm_loss(F.linear(hidden, weight),
                                              labels))
    print(f"PEAK fused {fused} unfused {unfused} one_logits {full}")
    assert fused < full
    assert unfused > full          # logits and dlogits: the measurement sees


# --------------------------------------------------------------- model parity
def _llama(tie):
    from acco_amd.models import LlamaConfig, LlamaForCausalLM
    torch.manual_seed(0)
    return LlamaForCausalLM(LlamaConfig(
        hidden_size=256, num_layers=2, num_heads=4, num_kv_heads=2,
        intermediate_size=512, vocab_size=515, max_position_embeddings=512,
        tie_word_embeddings=tie))


@pytest.mark.parametrize("tie", [False, True], ids=["untied", "tied"])
def test_model_on_the_arena_on_equals_off(tie):
    from acco_amd.engine import arena
    from acco_amd.models.fuse import install_fused_projections
    dev = torch.device("cuda")
    chunk, n_chunks = 128, 4
    ids = torch.randint(0, 515, (2, 256),
                        generator=torch.Generator().manual_seed(1))
    labels = ids.clone()
    labels[0, 7] = -100
    assert ids.numel() == chunk * n_chunks

    def gpu(flag):
        m = _llama(tie)
        p = arena.flatten_params(m, torch.bfloat16, dev, pad_to=256)
        g = arena.attach_grad_arena(m, torch.bfloat16, dev, pad_to=256)
        assert install_fused_projections(m, p, g) > 0
        assert getattr(m.lm_head, "_arena_fuse", None) is not None
        m.fused_lm_loss = flag
        m.lm_loss_chunk_tokens = chunk
        out = m(ids.to(dev), labels=labels.to(dev))
        assert (out[1] is None) == flag
        (out[0] * UPSTREAM).backward()
        torch.cuda.synchronize()
        return (out[0].detach().float().cpu(),
                {n: q.grad.float().cpu() for n, q in m.named_parameters()},
                {n: q.detach().float().cpu() for n, q in m.named_parameters()})

    loss_off, grads_off, weights = gpu(False)
    loss_on, grads_on, weights_on = gpu(True)
    # the fp32 CPU model on the same bf16 weights
    ref = _llama(tie)
    with torch.no_grad():
        for n, q in ref.named_parameters():
            assert torch.equal(weights[n], weights_on[n])
            q.copy_(weights[n])
    loss_ref, _ = ref(ids, labels=labels)
    (loss_ref * UPSTREAM).backward()

    what = "llama_tied" if tie else "llama_untied"
    _compare(f"loss {what}", loss_on.reshape(1), loss_off.reshape(1),
             loss_ref.detach().double().reshape(1))
    head = "model.embed_tokens.weight" if tie else "lm_head.weight"
    for n, q in ref.named_parameters():
        r = q.grad.double()
        extra = n_chunks * 0.5 * sr.ulp_bf16(r) if n == head else None
        _compare(f"grad {what} {n}", grads_on[n], grads_off[n], r, extra)
