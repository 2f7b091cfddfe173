"""Document-boundary masking of packed rows on the CPU path: the EOS-derived
`doc_start` array, the masked fp32 reference attention, both model families
(a packed row computes what its documents compute alone) and the trainer's
`train.doc_mask` flag."""

import os

import pytest
import torch

from tests.conftest import run_distributed
from tests.dist_utils import teardown_worker

EOS = 1


# ------------------------------------------------------- doc_start_from_eos
def _doc_start_loop(ids, eos):
    out = torch.zeros(ids.shape, dtype=torch.int32)
    for b in range(ids.shape[0]):
        start = 0
        for s in range(ids.shape[1]):
            out[b, s] = start
            if int(ids[b, s]) == eos:
                start = s + 1
    return out


def _check_invariants(ds):
    B, S = ds.shape
    pos = torch.arange(S)
    assert ds.dtype == torch.int32
    assert (ds[:, 1:] >= ds[:, :-1]).all()                 # non-decreasing
    assert (ds >= 0).all() and (ds <= pos[None]).all()
    assert torch.equal(torch.gather(ds.long(), 1, ds.long()), ds.long())


EOS_ROWS = {
    "eos_at_end": [[5, 3, 4, 2, 7, 6, 9, EOS]],
    "eos_at_0": [[EOS, 3, 4, 2, 7, 6, 9, 8]],
    "two_eos_in_a_row": [[5, 3, EOS, EOS, 7, 6, 9, 8]],
    "no_eos": [[5, 3, 4, 2, 7, 6, 9, 8]],
    "two_rows": [[5, EOS, 4, 2, 7, EOS, 9, 8], [5, 3, 4, EOS, 7, 6, EOS, EOS]],
}


@pytest.mark.parametrize("name", list(EOS_ROWS))
def test_doc_start_from_eos(name):
    from acco_amd import ops
    ids = torch.tensor(EOS_ROWS[name])
    ds = ops.doc_start_from_eos(ids, EOS)
    assert ds.device == ids.device and ds.shape == ids.shape
    assert torch.equal(ds, _doc_start_loop(ids, EOS))
    _check_invariants(ds)


def test_doc_end_is_the_next_start():
    from acco_amd import ops
    for rows in EOS_ROWS.values():
        ids = torch.tensor(rows)
        ds = ops.doc_start_from_eos(ids, EOS)
        de = ops.doc_end_from_start(ds)
        B, S = ids.shape
        for b in range(B):
            for s in range(S):
                same = [t for t in range(S) if ds[b, t] == ds[b, s]]
                assert int(de[b, s]) == same[-1] + 1


# --------------------------------------------------------- reference math
def _starts_to_doc_start(starts, S):
    ds = torch.zeros(S, dtype=torch.int32)
    for s0 in starts:
        ds[s0:] = s0
    return ds


@pytest.mark.parametrize("window", [None, 5])
def test_ref_attention_equals_per_document_slices(window):
    from acco_amd.ops import torch_ref
    torch.manual_seed(0)
    B, S, H, Hkv, D = 2, 24, 4, 2, 8
    q, k, v = (torch.randn(B, S, h, D) for h in (H, Hkv, Hkv))
    starts = [[0, 1, 9, 16], [0, 20]]
    ds = torch.stack([_starts_to_doc_start(st, S) for st in starts])
    out = torch_ref.causal_attention(q, k, v, window=window, doc_start=ds)
    for b, st in enumerate(starts):
        pieces = []
        for s0, s1 in zip(st, st[1:] + [S]):
            pieces.append(torch_ref.causal_attention(
                q[b:b + 1, s0:s1], k[b:b + 1, s0:s1], v[b:b + 1, s0:s1],
                window=window))
        want = torch.cat(pieces, dim=1)
        assert torch.allclose(out[b:b + 1], want, atol=1e-5, rtol=0)


@pytest.mark.parametrize("window", [None, 5])
def test_ref_attention_one_document_is_todays_output(window):
    from acco_amd import ops
    from acco_amd.ops import torch_ref
    torch.manual_seed(1)
    B, S, H, D = 2, 16, 2, 8
    q, k, v = (torch.randn(B, S, H, D) for _ in range(3))
    today = torch_ref.causal_attention(q, k, v, window=window)
    zeros = torch.zeros(B, S, dtype=torch.int32)
    assert torch.equal(torch_ref.causal_attention(
        q, k, v, window=window, doc_start=None), today)
    assert torch.equal(torch_ref.causal_attention(
        q, k, v, window=window, doc_start=zeros), today)
    # the public dispatch on CPU is the same math
    assert torch.equal(ops.causal_attention(q, k, v, window=window), today)
    assert torch.equal(ops.causal_attention(
        q, k, v, window=window, doc_start=zeros), today)


# ------------------------------------------------------------------ models
def _tiny(family):
    from acco_amd.models import (GPTNeoConfig, GPTNeoForCausalLM, LlamaConfig,
                                 LlamaForCausalLM)
    torch.manual_seed(0)
    if family == "llama":
        return LlamaForCausalLM(LlamaConfig(
            hidden_size=32, num_layers=2, num_heads=4, num_kv_heads=2,
            intermediate_size=64, vocab_size=64, max_position_embeddings=64))
    return GPTNeoForCausalLM(GPTNeoConfig(
        hidden_size=32, num_layers=2, num_heads=2, vocab_size=64,
        max_position_embeddings=64, window_size=4))


def _packed_row():
    g = torch.Generator().manual_seed(3)
    docs = []
    for n in (7, 9, 5):
        d = torch.randint(2, 64, (n,), generator=g)    # no EOS inside
        d[-1] = EOS
        docs.append(d)
    return docs, torch.cat(docs)[None]


@pytest.mark.parametrize("family", ["llama", "gptneo"])
def test_packed_row_logits_equal_documents_alone(family):
    from acco_amd import ops
    model = _tiny(family).eval()
    docs, row = _packed_row()
    ds = ops.doc_start_from_eos(row, EOS)
    with torch.no_grad():
        packed = model(row, doc_start=ds)[0]
        alone = torch.cat([model(d[None])[0] for d in docs], dim=1)
        plain = model(row)[0]
    assert torch.allclose(packed, alone, atol=2e-4, rtol=1e-4)
    # and the mask is what makes it so: the unmasked row differs after A
    assert not torch.allclose(plain[:, len(docs[0]):], alone[:, len(docs[0]):],
                              atol=2e-4, rtol=1e-4)
    # attention_mask stays accepted and unused
    with torch.no_grad():
        assert torch.equal(model(row, attention_mask=torch.ones_like(row),
                                 doc_start=ds)[0], packed)


@pytest.mark.parametrize("family", ["llama", "gptneo"])
@pytest.mark.parametrize("checkpointing", [False, True])
def test_no_gradient_across_a_boundary(family, checkpointing):
    from acco_amd import ops
    model = _tiny(family).train()
    inner = model.model if family == "llama" else model.transformer
    inner.gradient_checkpointing = checkpointing
    emb = inner.embed_tokens if family == "llama" else inner.wte
    kept = {}

    def keep(_mod, _inp, out):
        out.retain_grad()
        kept["emb"] = out
    handle = emb.register_forward_hook(keep)
    docs, row = _packed_row()
    a, b = len(docs[0]), len(docs[0]) + len(docs[1])
    ds = ops.doc_start_from_eos(row, EOS)
    logits = model(row, doc_start=ds)[0]
    handle.remove()
    # a loss on B's positions only
    loss = torch.nn.functional.cross_entropy(logits[0, a:b - 1],
                                             row[0, a + 1:b])
    loss.backward()
    grad = kept["emb"].grad
    assert torch.count_nonzero(grad[0, :a]) == 0       # exact zeros
    assert torch.count_nonzero(grad[0, b:]) == 0       # causal, as before
    assert torch.count_nonzero(grad[0, a:b]) > 0


def test_model_configs_read_eos_token_id():
    from acco_amd.models import GPTNeoConfig, LlamaConfig
    from acco_amd.config import load_config
    assert LlamaConfig().eos_token_id is None
    assert GPTNeoConfig().eos_token_id is None
    assert LlamaConfig.from_cfg({"eos_token_id": 2}).eos_token_id == 2
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = os.path.join(here, "acco_amd", "config", "model",
                        "gpt-neo-125M.json")
    assert GPTNeoConfig.from_hf_json(path).eos_token_id == 50256
    for name in ["acco", "ddp", "dpu", "acco-ft", "ddp-ft", "dpu-ft"]:
        assert load_config([f"train={name}"]).train.doc_mask is False


# ----------------------------------------------------------------- trainer
def _trainer_worker(rank, world, port, tmpdir):
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
            self.seen.append(sorted(inputs))
            if "doc_start" in inputs:
                assert torch.equal(
                    inputs["doc_start"].cpu(),
                    _doc_start_loop(inputs["input_ids"].cpu(), EOS))
            loss = super().forward_backward(inputs)
            self.losses.append(float(loss))
            return loss
    Recording.seen, Recording.losses = [], []

    def run(eos, *extra):
        cfg = load_config([
            "train=acco", "data=synthetic", "model=gptneo",
            "train.nb_steps_tot=4", "train.batch_size=2",
            "train.max_length=16", "train.use_mixed_precision=false",
            "train.save=false", "train.n_warmup_steps=0",
            "train.dataloader_num_workers=0", "train.comm_buckets=2",
            "train.dataloader_persistent_workers=false", *extra])
        torch.manual_seed(42)
        # a vocabulary of 4 puts several EOS into every 16-token row
        mcfg = GPTNeoConfig(hidden_size=32, num_layers=1, num_heads=2,
                            vocab_size=4, max_position_embeddings=64,
                            window_size=8, eos_token_id=eos)
        Recording.seen, Recording.losses = [], []
        t = Recording(model=GPTNeoForCausalLM(mcfg),
                      train_dataset=SyntheticCausalLMDataset(16, 16, 4, seed=3),
                      eval_dataset=SyntheticCausalLMDataset(4, 16, 4, seed=9),
                      args=cfg.train, run_name="docmask")
        t.train()
        return {"seen": list(Recording.seen), "losses": list(Recording.losses),
                "eval": t.eval_loop(),
                "batch_keys": sorted(t.load_next_batch())}

    res = {
        "on": run(EOS, "train.doc_mask=true"),
        "on_smooth": run(EOS, "train.doc_mask=true",
                         "train.label_smoothing_factor=0.1"),
        "off": run(EOS),
        "ragged": run(None, "train.doc_mask=true",
                      "train.const_len_batch=false"),
    }
    try:
        run(None, "train.doc_mask=true")
        res["no_eos_error"] = None
    except ValueError as e:
        res["no_eos_error"] = str(e)
    torch.save(res, os.path.join(tmpdir, "res.pt"))
    teardown_worker()


def test_trainer_doc_mask_flag():
    tmpdir = run_distributed(_trainer_worker, 1, timeout=300)
    res = torch.load(os.path.join(tmpdir, "res.pt"), weights_only=False)
    for key in ("on", "on_smooth"):
        r = res[key]
        assert r["batch_keys"] == ["doc_start", "input_ids"]
        assert r["seen"] and all(s == ["doc_start", "input_ids"]
                                 for s in r["seen"])
        assert all(torch.isfinite(torch.tensor(r["losses"])))
        assert r["eval"] == r["eval"]                  # finite, not nan
    assert res["off"]["batch_keys"] == ["input_ids"]
    assert all(s == ["input_ids"] for s in res["off"]["seen"])
    # the padded finetune collator is unaffected, and needs no EOS source
    assert res["ragged"]["batch_keys"] == ["input_ids", "labels"]
    assert res["no_eos_error"] and "eos" in res["no_eos_error"].lower()


def test_perplexity_eval_honours_doc_start():
    from torch.utils.data import DataLoader

    from acco_amd.data.synthetic import (DocMaskCollator,
                                         SyntheticCausalLMDataset,
                                         collate_input_ids,
                                         resolve_doc_mask_eos)
    from perplexity_eval import compute_perplexity
    model = _tiny("gptneo")
    model.cfg.eos_token_id = EOS
    assert resolve_doc_mask_eos(False, None, model) is None
    eos = resolve_doc_mask_eos(True, None, model)
    assert eos == EOS
    ds = SyntheticCausalLMDataset(4, 32, 4, seed=2)     # many EOS per row
    plain = compute_perplexity(
        model, DataLoader(ds, batch_size=2, collate_fn=collate_input_ids),
        torch.device("cpu"))
    masked = compute_perplexity(
        model, DataLoader(ds, batch_size=2, collate_fn=DocMaskCollator(eos)),
        torch.device("cpu"))
    assert masked == masked and plain == plain          # finite
    assert masked != plain
