"""ops.extend_attention's reference semantics and `extend` of both model
families, on the CPU in double. Bounds as in test_kv_cache.py: two fp64
attention rows differ by rounding only (1e-12 is far above D·L·2^-53 here),
teacher-forced fp64 logits by at most K·2^-53·max|logit|,
K = layers·(4·hidden + intermediate + S) + hidden."""

import pytest
import torch

from acco_amd import ops
from acco_amd.models import (GPTNeoConfig, GPTNeoForCausalLM, LlamaConfig,
                             LlamaForCausalLM, generate)
from acco_amd.models.kv_cache import KVCache
from acco_amd.ops import torch_ref
from tests.extend_ref import teacher_forced_extend

DT = torch.float64


@pytest.mark.parametrize("rep", [1, 2])
@pytest.mark.parametrize("window", [0, 5])
def test_ref_extend_is_last_rows_of_causal(rep, window):
    torch.manual_seed(0)
    Hkv, D, T, Smax = 2, 16, 6, 20
    L0 = [0, 9]
    q = torch.randn(2, 9 + T, Hkv * rep, D, dtype=DT)
    k = torch.randn(2, 9 + T, Hkv, D, dtype=DT)
    v = torch.randn(2, 9 + T, Hkv, D, dtype=DT)
    # the caches hold rows [0, L0 + T) of k, v; every other row is NaN
    beyond = torch.arange(Smax)[None] >= torch.tensor(L0)[:, None] + T
    kc, vc = (torch.nn.functional.pad(x, (0, 0, 0, 0, 0, Smax - 9 - T))
              .permute(0, 2, 1, 3).masked_fill(beyond[:, None, :, None],
                                               float("nan")) for x in (k, v))
    qn = torch.stack([q[b, L:L + T] for b, L in enumerate(L0)])
    got = ops.extend_attention(qn, kc, vc, torch.tensor(L0, dtype=torch.int32),
                               window=window)
    assert got.shape == qn.shape and got.dtype == DT
    for b, L in enumerate(L0):
        want = torch_ref.causal_attention(
            q[b:b + 1, :L + T], k[b:b + 1, :L + T], v[b:b + 1, :L + T],
            window=window or None)[0, L:]
        assert float((got[b] - want).abs().max()) <= 1e-12, (b, window, rep)


def test_ref_extend_one_token_is_decode_and_dropped_rows_are_zero():
    torch.manual_seed(1)
    B, H, D, Smax = 3, 4, 8, 12
    kc, vc = torch.randn(2, B, 2, Smax, D, dtype=DT)
    lens = torch.tensor([0, 5, Smax - 1], dtype=torch.int32)
    q = torch.randn(B, 1, H, D, dtype=DT)
    for window in (None, 3):
        a = torch_ref.extend_attention(q, kc, vc, lens, window=window)[:, 0]
        b = torch_ref.decode_attention(q[:, 0], kc, vc, lens + 1,
                                       window=window)
        assert float((a - b).abs().max()) <= 1e-12
    # L0 = Smax - 2, T = 4: tokens 2 and 3 were dropped by the append
    q = torch.randn(1, 4, H, D, dtype=DT)
    o = torch_ref.extend_attention(q, kc[:1], vc[:1],
                                   torch.tensor([Smax - 2], dtype=torch.int32))
    assert bool((o[0, :2].abs().amax((-1, -2)) > 0).all())
    assert bool((o[0, 2:] == 0).all()) and not bool(o[0, 2:].signbit().any())


# ------------------------------------------------------------ both families
S, PREFIX = 96, [5, 17, 30]


@pytest.fixture(scope="module", params=["llama", "gptneo"])
def family(request):
    torch.manual_seed(0)
    kw = dict(num_layers=2, vocab_size=97, max_position_embeddings=128)
    if request.param == "llama":
        model = LlamaForCausalLM(LlamaConfig(
            hidden_size=64, num_heads=4, num_kv_heads=2, intermediate_size=128,
            tie_word_embeddings=False, **kw))
    else:       # one global, one local layer
        model = GPTNeoForCausalLM(GPTNeoConfig(
            hidden_size=32, num_heads=2, window_size=8, **kw))
    model = model.double().eval()
    ids = torch.randint(0, 97, (3, S),
                        generator=torch.Generator().manual_seed(11))
    with torch.no_grad():
        full = model(ids)[0]
    cfg = model.cfg
    inter = getattr(cfg, "intermediate_size", None) or 4 * cfg.hidden_size
    K = cfg.num_layers * (4 * cfg.hidden_size + inter + S) + cfg.hidden_size
    return dict(model=model, ids=ids, full=full,
                bound=K * 2.0 ** -53 * float(full.abs().max()))


@pytest.mark.parametrize("width", [7, 64])
def test_extend_teacher_forced_fp64(family, width):
    model, ids, full = family["model"], family["ids"], family["full"]
    got, b, pos, cache = teacher_forced_extend(model, ids, PREFIX, width, 128)
    assert got.shape[0] == 3 + sum(S - p for p in PREFIX)
    err = float((got - full[b, pos]).abs().max())
    print("EXTEND fp64 width %d err %.3e bound %.3e"
          % (width, err, family["bound"]))
    assert err <= family["bound"]
    with pytest.raises(ValueError):
        model.extend(ids[:, :128 - cache.steps + 1], cache)


def test_extend_ragged_n_new_equals_unpadded(family):
    model, ids, bound = family["model"], family["ids"], family["bound"]
    n_new = torch.tensor([3, 7, 0], dtype=torch.int32)
    cache = KVCache.allocate(model, 3, 64)
    model.prefill(ids[:, :20], None, cache)
    last = model.extend(ids[:, 20:27], cache, n_new=n_new, last_only=True)
    assert torch.equal(cache.lens, 20 + n_new)
    step = model.decode_step(ids[:, 40], cache)
    for b, n in enumerate(n_new.tolist()):
        one = KVCache.allocate(model, 1, 64)
        want = model.prefill(ids[b:b + 1, :20], None, one)
        if n:       # n = 0: `last` is the pad's row 0, nothing to compare
            want = model.extend(ids[b:b + 1, 20:20 + n], one)[:, -1]
            assert float((last[b] - want[0]).abs().max()) <= bound
        want = model.decode_step(ids[b:b + 1, 40], one)
        assert float((step[b] - want[0]).abs().max()) <= bound


def test_greedy_generate_with_chunked_prefill(family):
    model, ids = family["model"], family["ids"]
    lens = torch.tensor([40, 9, 33])
    kw = dict(max_new=8, temperature=0.0, eos_token_id=None)
    want, _ = generate(model, ids[:, :40], lens, **kw)
    got, _ = generate(model, ids[:, :40], lens, prefill_chunk=16, **kw)
    assert torch.equal(got, want)
