"""The chunked lm_head + loss (ops.linear_causal_lm_loss) on the CPU path:
chunked against unchunked math in fp64, degenerate labels, the grad-arena
destination and its single producer notification, both model families with
`fused_lm_loss` on against off, the config keys and the trainer wiring."""

import os

import pytest
import torch
import torch.nn.functional as F

from tests.conftest import run_distributed
from tests.dist_utils import teardown_worker

B, S, H, V = 2, 7, 6, 11
T = B * S


def _inputs(dtype=torch.float64, seed=0):
    g = torch.Generator().manual_seed(seed)
    hidden = torch.randn(B, S, H, generator=g, dtype=dtype)
    weight = torch.randn(V, H, generator=g, dtype=dtype)
    labels = torch.randint(0, V, (B, S), generator=g)
    labels[0, 3] = -100
    labels[1, 1] = -100
    return hidden, weight, labels


def _close(got, ref, rtol=1e-12):
    """Error relative to the largest reference entry: sums of products cancel
    in single entries of dh and dW, so an entry-wise relative bound would ask
    for more than fp64 summation in another order can give."""
    if not ref.abs().max() > 0:
        return not got.any()
    return float((got - ref).abs().max()) <= rtol * float(ref.abs().max())


def _torch_ref_loss(logits, labels, eps):
    from acco_amd.ops import torch_ref
    if eps == 0.0:
        return torch_ref.causal_lm_loss(logits, labels)
    return torch_ref.label_smoothed_causal_lm_loss(logits, labels, eps)


def _unchunked(hidden, weight, labels, eps):
    """Unchunked F.linear + the math of torch_ref.causal_lm_loss /
    label_smoothed_causal_lm_loss in the inputs' own dtype. Those two cast
    their logits to fp32 first, which would cap an fp64 comparison at 1e-7,
    so their formulas are repeated here without the cast and checked against
    them at fp32 accuracy."""
    logits = F.linear(hidden, weight)
    sl = logits[..., :-1, :].reshape(-1, logits.shape[-1])
    lab = labels[..., 1:].reshape(-1)
    if eps == 0.0:
        loss = F.cross_entropy(sl, lab, ignore_index=-100)
    else:
        logp = F.log_softmax(sl, dim=-1)
        mask = lab.eq(-100)
        nll = -logp.gather(-1, lab.clamp(min=0)[:, None]).squeeze(-1)
        nll = nll.masked_fill(mask, 0.0)
        smooth = -logp.sum(-1).masked_fill(mask, 0.0)
        n = (~mask).sum().clamp(min=1)
        loss = ((1.0 - eps) * nll.sum() / n
                + eps * smooth.sum() / (n * sl.shape[-1]))
    assert torch.allclose(loss.detach().float(),
                          _torch_ref_loss(logits.detach(), labels, eps),
                          rtol=1e-5, atol=0)
    return loss


# ------------------------------------------------- chunked against unchunked
@pytest.mark.parametrize("upstream", [1.0, 1.0 / 3.0])
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("chunk", [1, 5, T, 10 * T])
def test_chunked_equals_unchunked_fp64(chunk, eps, upstream):
    from acco_amd import ops
    hidden, weight, labels = _inputs()
    h1 = hidden.clone().requires_grad_(True)
    w1 = weight.clone().requires_grad_(True)
    h2 = hidden.clone().requires_grad_(True)
    w2 = weight.clone().requires_grad_(True)
    loss = ops.linear_causal_lm_loss(h1, w1, labels, epsilon=eps,
                                     chunk_tokens=chunk)
    want = _unchunked(h2, w2, labels, eps)
    assert loss.dtype == torch.float64 and want.dtype == torch.float64
    assert loss.shape == ()
    (loss * upstream).backward()
    (want * upstream).backward()
    for what, got, ref in (("loss", loss.detach(), want.detach()),
                           ("dh", h1.grad, h2.grad), ("dW", w1.grad, w2.grad)):
        assert _close(got, ref), (what, float((got - ref).abs().max()))
    # same inputs, same bits
    again = ops.linear_causal_lm_loss(hidden, weight, labels, epsilon=eps,
                                      chunk_tokens=chunk)
    assert torch.equal(again, loss.detach())


def test_public_and_reference_entry_points_agree():
    from acco_amd import ops
    from acco_amd.ops import torch_ref
    hidden, weight, labels = _inputs(torch.float32)
    assert torch.equal(
        ops.linear_causal_lm_loss(hidden, weight, labels, 0.1, 5),
        torch_ref.linear_causal_lm_loss(hidden, weight, labels, 0.1, 5))
    with pytest.raises(ValueError):
        ops.linear_causal_lm_loss(hidden, weight, labels, chunk_tokens=0)


# --------------------------------------------------------- degenerate labels
@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_all_labels_ignored(eps):
    from acco_amd import ops
    hidden, weight, _ = _inputs()
    hidden.requires_grad_(True)
    weight.requires_grad_(True)
    labels = torch.full((B, S), -100)
    loss = ops.linear_causal_lm_loss(hidden, weight, labels, eps, 5)
    loss.backward()
    assert float(loss.detach()) == 0.0
    assert not hidden.grad.any() and not weight.grad.any()


@pytest.mark.parametrize("bad", [V, V + 3, 2 ** 40, -1, -7])
def test_out_of_range_label_is_ignored(bad):
    from acco_amd import ops
    hidden, weight, labels = _inputs()
    with_bad = labels.clone()
    with_bad[0, 2] = bad
    with_ignored = labels.clone()
    with_ignored[0, 2] = -100
    res = []
    for lab in (with_bad, with_ignored):
        h = hidden.clone().requires_grad_(True)
        w = weight.clone().requires_grad_(True)
        loss = ops.linear_causal_lm_loss(h, w, lab, 0.1, 5)
        loss.backward()
        res.append((loss.detach(), h.grad, w.grad))
    for got, ref in zip(*res):
        assert torch.equal(got, ref)
    assert not res[0][1][0, 1].any()          # the row that label belongs to


# ------------------------------------------------------------ grad_view path
@pytest.mark.parametrize("chunk,n_chunks", [(T, 1), (4, 4)])
def test_grad_view_accumulates_and_notifies_once(chunk, n_chunks):
    from acco_amd import ops
    from acco_amd.models import fuse
    assert -(-T // chunk) == n_chunks
    hidden, weight, labels = _inputs()
    h1 = hidden.clone().requires_grad_(True)
    w1 = weight.clone().requires_grad_(True)
    (ops.linear_causal_lm_loss(h1, w1, labels, 0.1, chunk) / 3).backward()

    arena = torch.zeros(5 + V * H + 3, dtype=torch.float64)
    prior = torch.randn(V, H, dtype=torch.float64)
    view = arena[5:5 + V * H].view(V, H)
    view.copy_(prior)
    h2 = hidden.clone().requires_grad_(True)
    w2 = weight.clone().requires_grad_(True)
    calls = []
    fuse.set_grad_notifier(lambda off, num: calls.append((off, num)))
    try:
        loss = ops.linear_causal_lm_loss(h2, w2, labels, 0.1, chunk,
                                         grad_view=view)
        assert calls == []                      # nothing before backward
        (loss / 3).backward()
    finally:
        fuse.set_grad_notifier(None)
    assert calls == [(5, V * H)]
    assert w2.grad is None
    assert _close(view, prior + w1.grad)
    assert _close(h2.grad, h1.grad)
    assert not arena[:5].any() and not arena[5 + V * H:].any()


# -------------------------------------------------------------- model parity
def _tiny(family):
    from acco_amd.models import (GPTNeoConfig, GPTNeoForCausalLM, LlamaConfig,
                                 LlamaForCausalLM)
    torch.manual_seed(0)
    if family == "llama":               # GQA, untied
        return LlamaForCausalLM(LlamaConfig(
            hidden_size=32, num_layers=2, num_heads=4, num_kv_heads=2,
            intermediate_size=64, vocab_size=67, max_position_embeddings=64,
            tie_word_embeddings=False))
    return GPTNeoForCausalLM(GPTNeoConfig(      # tied
        hidden_size=32, num_layers=2, num_heads=2, vocab_size=67,
        max_position_embeddings=64, window_size=4))


@pytest.mark.parametrize("smoothing", [0.0, 0.1])
@pytest.mark.parametrize("family", ["llama", "gptneo"])
def test_model_fused_on_equals_off(family, smoothing):
    from acco_amd import ops
    model = _tiny(family)
    tied = model.cfg.tie_word_embeddings
    assert tied == (family == "gptneo")
    assert type(model).fused_lm_loss is False
    assert type(model).lm_loss_chunk_tokens == 4096
    ids = torch.randint(0, 67, (2, 12), generator=torch.Generator().manual_seed(1))
    labels = ids.clone()
    labels[0, 4] = -100

    kw = {"label_smoothing": smoothing} if smoothing else {}
    loss_off, logits = model(ids, labels=labels, **kw)
    assert logits.shape == (2, 12, 67)
    # the keyword is the smoothed loss on the logits
    assert torch.allclose(loss_off, ops.label_smoothed_causal_lm_loss(
        logits, labels, smoothing), rtol=1e-6, atol=0)
    loss_off.backward()
    grads_off = {n: p.grad.clone() for n, p in model.named_parameters()}
    model.zero_grad(set_to_none=True)

    model.fused_lm_loss = True
    model.lm_loss_chunk_tokens = 5
    out = model(ids, labels=labels, **kw)
    assert isinstance(out, tuple) and len(out) == 2 and out[1] is None
    out[0].backward()
    assert torch.allclose(out[0], loss_off, rtol=1e-5, atol=0)
    for n, p in model.named_parameters():
        assert p.grad is not None, n
        assert torch.allclose(p.grad, grads_off[n], rtol=1e-5, atol=1e-7), (
            n, float((p.grad - grads_off[n]).abs().max()))
    # without labels the flag changes nothing
    with torch.no_grad():
        (only,) = model(ids)
    assert torch.equal(only, logits.detach())


# -------------------------------------------------------------------- config
def test_config_keys_default_off():
    from acco_amd.config import load_config
    for name in ["acco", "ddp", "dpu", "acco-ft", "ddp-ft", "dpu-ft"]:
        cfg = load_config([f"train={name}"])
        assert cfg.train.fused_lm_loss is False
        assert cfg.train.lm_loss_chunk_tokens == 4096


# ------------------------------------------------------------------- trainer
def _trainer_worker(rank, world, port, tmpdir, method):
    os.environ.update({
        "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port),
        "RANK": str(rank), "LOCAL_RANK": str(rank), "WORLD_SIZE": str(world),
    })
    os.chdir(tmpdir)
    from acco_amd.config import load_config
    from acco_amd.data.synthetic import SyntheticCausalLMDataset
    from acco_amd.engine.trainer import DecoupledTrainer
    from acco_amd.models import GPTNeoConfig, GPTNeoForCausalLM

    class Recording(DecoupledTrainer):
        def forward_backward(self, inputs):
            loss = super().forward_backward(inputs)
            self.losses.append(float(loss))
            if self.ddp is not None and self.ddp.sync_enabled:
                self.coverage.append((list(self.ddp._got),
                                      list(self.ddp._req)))
            return loss

    def run(*extra):
        cfg = load_config([
            f"train={method}", "data=synthetic", "model=gptneo",
            "train.nb_steps_tot=8", "train.batch_size=2",
            "train.max_length=16", "train.use_mixed_precision=false",
            "train.save=false", "train.warmup=2", "train.n_warmup_steps=0",
            "train.dataloader_num_workers=0", "train.comm_buckets=2",
            "train.dataloader_persistent_workers=false", *extra])
        torch.manual_seed(42)
        mcfg = GPTNeoConfig(hidden_size=32, num_layers=2, num_heads=2,
                            vocab_size=64, max_position_embeddings=32,
                            window_size=8)
        model = GPTNeoForCausalLM(mcfg)
        Recording.losses, Recording.coverage = [], []
        t = Recording(model=model,
                      train_dataset=SyntheticCausalLMDataset(32, 16, 64,
                                                             seed=5 + rank),
                      eval_dataset=SyntheticCausalLMDataset(4, 16, 64, seed=9),
                      args=cfg.train, run_name="fusedloss")
        t.train()
        return {"flag": model.fused_lm_loss,
                "chunk": model.lm_loss_chunk_tokens,
                "losses": list(Recording.losses),
                "coverage": list(Recording.coverage),
                "eval": t.eval_loop(),
                "params": t.params[:t.n_live].clone()}

    on = ["train.fused_lm_loss=true", "train.lm_loss_chunk_tokens=64"]
    res = {"off": run(), "on": run(*on),
           "on_smooth": run(*on, "train.label_smoothing_factor=0.1",
                            "train.lm_loss_chunk_tokens=5")}
    torch.save(res, os.path.join(tmpdir, f"res_{rank}.pt"))
    teardown_worker()


@pytest.mark.parametrize("method", ["acco", "ddp"])
def test_trainer_with_fused_lm_loss(method):
    tmpdir = run_distributed(_trainer_worker, 2, args=(method,), timeout=300)
    res = [torch.load(os.path.join(tmpdir, f"res_{r}.pt"), weights_only=False)
           for r in range(2)]
    for key in ("off", "on", "on_smooth"):
        assert torch.equal(res[0][key]["params"], res[1][key]["params"]), key
    for r in res:
        assert r["off"]["flag"] is False and r["off"]["chunk"] == 4096
        assert r["on"]["flag"] is True and r["on"]["chunk"] == 64
        assert r["on_smooth"]["flag"] is True and r["on_smooth"]["chunk"] == 5
        for key in ("on", "on_smooth"):
            assert r[key]["losses"]
            assert torch.isfinite(torch.tensor(r[key]["losses"])).all()
            assert torch.isfinite(r[key]["params"]).all()
            assert r[key]["eval"] == r[key]["eval"]
        # the flag changes how the loss is computed, not what it is. Every
        # micro-batch of a DDP run; the first of an ACCO run, whose later
        # ones see whichever parameters the overlapped round has committed
        n = len(r["off"]["losses"]) if method == "ddp" else 1
        assert len(r["on"]["losses"]) >= n
        assert torch.allclose(torch.tensor(r["on"]["losses"][:n]),
                              torch.tensor(r["off"]["losses"][:n]),
                              rtol=1e-4, atol=0)
        if method == "ddp":
            for key in ("off", "on", "on_smooth"):
                assert r[key]["coverage"]
                for got, req in r[key]["coverage"]:
                    assert got == req, (key, got, req)
