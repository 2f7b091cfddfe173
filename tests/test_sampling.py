"""On-device sampling on the CPU: the reference semantics of
ops.sample_logits (its generator against the published Philox4x32-10
known-answer vectors, its filters against a brute-force fp64 sort, its draws
against the filtered distribution), models.generate on both model families,
and the tool's --device-sampling paths.

The brute force sums probabilities in another order than the reference, so a
filter case is only meaningful where no cumulative mass lies within 1e-12 of
top_p; that is asserted on the reference's own margin, never skipped."""

import contextlib
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

from acco_amd import ops
from acco_amd.models import (GPTNeoConfig, GPTNeoForCausalLM, LlamaConfig,
                             LlamaForCausalLM, generate)
from acco_amd.ops import torch_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOK_DIR = os.path.join(REPO, "corpus", "tokenizer")
TOOL_OVERRIDES = ["model=gptneo", "model.hidden_size=32",
                  "model.num_layers=1", "model.num_heads=2",
                  "model.max_position_embeddings=64", "model.window_size=16",
                  "model.config_path=null"]


def _load_tool():
    spec = importlib.util.spec_from_file_location(
        "generate_tool", os.path.join(REPO, "tools", "generate.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---------------------------------------------------------------- generator
# Random123 (Salmon, Moraes, Dror, Shaw, SC'11), kat_vectors, philox4x32 10
PHILOX_KAT = [
    ((0, 0, 0, 0), (0, 0),
     (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2,
     (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344),
     (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("ctr,key,want", PHILOX_KAT)
def test_philox_known_answer(ctr, key, want):
    got = torch_ref.philox4x32_10(ctr, key)
    assert tuple(int(w) for w in got) == want


def test_philox_is_elementwise_over_arrays():
    ctrs = np.array([c for c, _, _ in PHILOX_KAT], dtype=np.uint64).T
    keys = np.array([k for _, k, _ in PHILOX_KAT], dtype=np.uint64).T
    got = torch_ref.philox4x32_10(tuple(ctrs), tuple(keys))
    for j, (_, _, want) in enumerate(PHILOX_KAT):
        assert tuple(int(w[j]) for w in got) == want


def test_uniform_is_exact_in_fp32_and_inside_unit_interval():
    u = torch_ref.sample_uniform(np.arange(100000), 3, 2 ** 40 + 5, 2 ** 63 + 9)
    assert u.min() >= 2.0 ** -24 and u.max() <= 1 - 2.0 ** -24
    assert np.array_equal(u.astype(np.float32).astype(np.float64), u)
    # word 0 of the first vector: r = 0x6627e8d5 >> 9
    u0 = torch_ref.sample_uniform(np.array([0]), 0, 0, 0)[0]
    assert u0 == ((0x6627e8d5 >> 9) + 0.5) * 2.0 ** -23
    # another row, step or seed is another stream
    base = torch_ref.sample_uniform(np.arange(64), 0, 0, 0)
    for args in [(1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 2 ** 32, 0),
                 (0, 0, 2 ** 32)]:
        assert not np.array_equal(
            base, torch_ref.sample_uniform(np.arange(64), *args))


# ------------------------------------------------------------------ filters
def _rows(kind, V, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "ties":
        x = torch.randint(-3, 4, (3, V), generator=g).float()
    else:
        x = torch.randn(3, V, generator=g) * 3
    return x.bfloat16()


def _brute_force(x64, T, top_k, top_p):
    """(thr, n_kept) of one fp64 row by sorting: top-k's k-th value with its
    ties, then the largest value whose upper mass among the survivors reaches
    top_p."""
    V = x64.numel()
    thr = -math.inf
    if 1 <= top_k < V:
        thr = float(torch.topk(x64, top_k).values[-1])
    if top_p < 1.0:
        keep = x64 >= thr
        p = torch.softmax(x64[keep] / T, dim=0)
        vals, order = torch.sort(x64[keep], descending=True)
        cum = torch.cumsum(p[order], 0)
        for v in torch.unique(vals).flip(0):          # descending
            if float(cum[int((vals >= v).sum()) - 1]) >= top_p:
                thr = max(thr, float(v))
                break
    if thr == -math.inf:                   # no filter: the lowest finite bf16
        thr = -float(torch.finfo(torch.bfloat16).max)
    return thr, int((x64 >= thr).sum())


FILTER_CASES = [(k, p) for k in (0, 1, 2, 5, 50, 10 ** 6)
                for p in (1.0, 0.1, 0.9, 1 - 2.0 ** -30)]


@pytest.mark.parametrize("kind", ["randn", "ties"])
@pytest.mark.parametrize("V", [1, 2, 7, 50, 257])
def test_filters_match_brute_force(kind, V):
    T = 0.7
    x = _rows(kind, V, 100 + V)
    for top_k, top_p in FILTER_CASES:
        det = []
        tok, lp, thr, n = torch_ref.sample_logits(
            x, temperature=T, top_k=top_k, top_p=top_p, seed=1, step=2,
            details=det)
        assert tok.dtype == torch.int64 and lp.dtype == torch.float32
        assert thr.dtype == torch.bfloat16 and n.dtype == torch.int32
        for b in range(x.shape[0]):
            assert det[b]["p_margin"] > 1e-12, (V, top_k, top_p, b)
            x64 = x[b].double()
            # the kernel's temperature is fp32
            want_thr, want_n = _brute_force(x64, float(np.float32(T)),
                                            top_k, top_p)
            assert float(thr[b]) == want_thr, (V, top_k, top_p, b)
            assert int(n[b]) == want_n, (V, top_k, top_p, b)
            assert x64[tok[b]] >= want_thr and 0 <= int(tok[b]) < V
            kept = x64 >= want_thr
            logp = torch.log_softmax(x64[kept] / float(np.float32(T)), 0)
            want_lp = float(logp[int(kept[:int(tok[b])].sum())])
            assert abs(float(lp[b]) - want_lp) <= 2.0 ** -23 * (
                1 + abs(want_lp)), (V, top_k, top_p, b)


def test_topk_is_torch_topk_and_keeps_ties():
    x = _rows("ties", 257, 7)
    for k in (1, 2, 5, 50):
        _, _, thr, n = ops.sample_logits(x, temperature=1.0, top_k=k,
                                         seed=0, step=0)
        for b in range(3):
            kth = torch.topk(x[b].float(), k).values[-1]
            assert float(thr[b]) == float(kth)
            assert int(n[b]) == int((x[b].float() >= kth).sum())
            assert int(n[b]) > k          # 7 values over 257 slots: ties
    # k >= V and k = 0 keep everything
    for k in (0, 257, 258):
        _, _, thr, n = ops.sample_logits(x, temperature=1.0, top_k=k,
                                         seed=0, step=0)
        assert n.tolist() == [257] * 3
        assert thr.float().tolist() == [
            -float(torch.finfo(torch.bfloat16).max)] * 3


def test_special_values():
    nan, inf = float("nan"), float("inf")
    big = float(torch.finfo(torch.bfloat16).max)
    x = torch.tensor([[nan, nan, nan, nan],
                      [-inf, -inf, -inf, -inf],
                      [0.0, inf, 1.0, nan],
                      [-0.0, 0.0, -0.0, -1.0],
                      [nan, -1.0, nan, -2.0]]).bfloat16()
    tok, lp, thr, n = ops.sample_logits(x, temperature=1.0, seed=3, step=1)
    assert n.tolist() == [0, 4, 3, 4, 2]
    assert int(tok[0]) == 0 and float(lp[0]) == 0.0
    assert int(tok[2]) == 1                 # exp(1 - big) underflows
    assert int(tok[4]) in (1, 3)
    assert thr.float().tolist() == [-big] * 5      # no filter: lowest finite
    _, _, thr, n = ops.sample_logits(x, temperature=1.0, top_k=3, seed=3,
                                     step=1)
    # NaN counts as the lowest value but is never kept
    assert thr.float().tolist() == [-big, -big, 0.0, 0.0, -big]
    assert n.tolist() == [0, 4, 3, 3, 2]
    assert abs(float(lp[1]) - math.log(0.25)) < 1e-6
    # -0 and +0 are one value: top-1 keeps all three zeros
    _, _, thr, n = ops.sample_logits(x[3:4], temperature=1.0, top_k=1,
                                     seed=0, step=0)
    assert int(n[0]) == 3 and float(thr[0]) == 0.0
    assert math.copysign(1.0, float(thr[0])) == 1.0
    # greedy: lowest index of the largest value, unfiltered T = 1 softmax
    tok, lp, thr, n = ops.sample_logits(x, temperature=0.0, top_k=1,
                                        top_p=0.1, seed=0, step=0)
    assert tok.tolist() == [0, 0, 1, 0, 1]
    assert n.tolist() == [0, 4, 3, 4, 2]
    want = torch.log_softmax(torch.tensor([-1.0, -2.0]).double(), 0)[0]
    assert abs(float(lp[4]) - float(want)) < 1e-6


def test_fp32_logits_are_taken_as_bf16():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 300, generator=g) * 3
    a = ops.sample_logits(x, temperature=0.8, top_k=40, top_p=0.95, seed=1,
                          step=9)
    b = ops.sample_logits(x.bfloat16(), temperature=0.8, top_k=40,
                          top_p=0.95, seed=1, step=9)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


def test_done_and_eos():
    x = _rows("randn", 50, 11)
    tok0, _, _, _ = ops.sample_logits(x, temperature=1.0, seed=4, step=0)
    eos = int(tok0[1])
    done = torch.tensor([1, 0, 0], dtype=torch.uint8)
    tok, lp, thr, n = ops.sample_logits(x, temperature=1.0, seed=4, step=0,
                                        done=done, eos_id=eos)
    assert int(tok[0]) == eos and int(n[0]) == 0 and float(lp[0]) == 0.0
    assert tok[1:].tolist() == tok0[1:].tolist()
    assert done.tolist() == [1, 1, int(int(tok0[2]) == eos)]
    with pytest.raises(ValueError):
        ops.sample_logits(x, temperature=1.0, seed=4, step=0, done=done,
                          eos_id=50)
    with pytest.raises(ValueError):
        ops.sample_logits(x, temperature=-1.0, seed=4, step=0)
    with pytest.raises(ValueError):
        ops.sample_logits(x, temperature=1.0, top_p=0.0, seed=4, step=0)


# ------------------------------------------------------------- distribution
def test_draws_follow_the_filtered_distribution():
    """8192 draws of one row of V = 50 under top-k 20 and top-p 0.9, one per
    step: every kept token's count within 6 standard deviations of N·p, no
    draw outside the kept set. Fixed seed: deterministic."""
    N, V, T, top_k, top_p = 8192, 50, 0.7, 20, 0.9
    x = (torch.randn(1, V, generator=torch.Generator().manual_seed(50)) * 3
         ).bfloat16()
    x64 = x[0].double()
    thr, n_kept = _brute_force(x64, float(np.float32(T)), top_k, top_p)
    kept = x64 >= thr
    assert 1 < n_kept < top_k
    p = torch.zeros(V, dtype=torch.float64)
    p[kept] = torch.softmax(x64[kept] / float(np.float32(T)), 0)
    bits = x.view(torch.int16).numpy().view(np.uint16)[0]
    counts = np.zeros(V, dtype=np.int64)
    for step in range(N):
        r = torch_ref.sample_row(bits, 0, T, top_k, top_p, 2024, step)
        assert r["n_kept"] == n_kept
        counts[r["token"]] += 1
    assert counts[~kept.numpy()].sum() == 0
    for i in np.nonzero(kept.numpy())[0]:
        pi = float(p[i])
        dev = abs(counts[i] - N * pi)
        lim = 6 * math.sqrt(N * pi * (1 - pi))
        print("DIST token %d p %.4f count %d dev/lim %.3f"
              % (i, pi, counts[i], dev / lim))
        assert dev <= lim, (i, pi, counts[i])


# ----------------------------------------------------------------- generate
def _tiny(family):
    torch.manual_seed(0)
    if family == "llama":
        cfg = LlamaConfig(hidden_size=32, num_layers=2, num_heads=4,
                          num_kv_heads=2, intermediate_size=64, vocab_size=61,
                          max_position_embeddings=48)
        return LlamaForCausalLM(cfg).double().eval()
    cfg = GPTNeoConfig(hidden_size=32, num_layers=2, num_heads=4,
                       vocab_size=61, max_position_embeddings=48,
                       window_size=8)
    return GPTNeoForCausalLM(cfg).double().eval()


def _prompts():
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(0, 61, (3, 9), generator=g)
    return ids, torch.tensor([9, 4, 6])


def _argmax_reforward(model, ids, lens, max_new):
    """Uncached greedy: one full forward per token and sequence; the argmax
    is taken on the bf16 value, lowest index on ties, as the sampler does."""
    rows = []
    for b in range(ids.shape[0]):
        seq = ids[b:b + 1, :int(lens[b])]
        for _ in range(max_new):
            out = model(seq)
            logits = out[0] if isinstance(out, tuple) else out
            last = logits[0, -1].bfloat16().double()
            nxt = int((last == last.max()).nonzero()[0])
            seq = torch.cat([seq, torch.tensor([[nxt]])], dim=1)
        rows.append(seq[0])
    return rows


@contextlib.contextmanager
def _no_host_reads():
    def boom(*a, **k):
        raise AssertionError("host read inside the generation loop")
    saved = {n: getattr(torch.Tensor, n)
             for n in ("item", "cpu", "tolist", "__bool__")}
    for n in saved:
        setattr(torch.Tensor, n, boom)
    try:
        yield
    finally:
        for n, f in saved.items():
            setattr(torch.Tensor, n, f)


@pytest.fixture(scope="module", params=["llama", "gptneo"])
def greedy_run(request):
    model = _tiny(request.param)
    ids, lens = _prompts()
    max_new = 12
    with _no_host_reads():
        tokens, n_gen = generate(model, ids, lens, max_new=max_new,
                                 temperature=0.0)
    return model, ids, lens, max_new, tokens, n_gen


def test_generate_greedy_equals_uncached_argmax(greedy_run):
    model, ids, lens, max_new, tokens, n_gen = greedy_run
    assert tokens.shape == (3, 9 + max_new) and tokens.dtype == torch.int64
    assert n_gen.tolist() == [max_new] * 3
    want = _argmax_reforward(model, ids, lens, max_new)
    for b in range(3):
        L = int(lens[b])
        assert torch.equal(tokens[b, :L + max_new], want[b]), b
        assert (tokens[b, L + max_new:] == 0).all()       # no eos: fill 0


def test_generate_full_prompts_default_lens(greedy_run):
    model, ids, _, max_new, _, _ = greedy_run
    tokens, _ = generate(model, ids, max_new=4, temperature=0.0)
    want = _argmax_reforward(model, ids, torch.tensor([9, 9, 9]), 4)
    assert torch.equal(tokens, torch.stack(want))
    empty, n = generate(model, ids, max_new=0)
    assert torch.equal(empty, ids) and n.tolist() == [0, 0, 0]
    with pytest.raises(ValueError):
        generate(model, ids, max_new=40)                  # 9 + 40 > 48


def test_generate_eos_pins_a_finished_sequence(greedy_run):
    model, ids, lens, max_new, free, _ = greedy_run
    eos = int(free[0, int(lens[0]) + 2])          # sequence 0's third token
    with _no_host_reads():
        tokens, n_gen = generate(model, ids, lens, max_new=max_new,
                                 temperature=0.0, eos_token_id=eos)
    for b in range(3):
        L = int(lens[b])
        new_free = free[b, L:L + max_new].tolist()
        first = new_free.index(eos) if eos in new_free else max_new - 1
        assert int(n_gen[b]) == first + 1, b
        assert tokens[b, L:L + first + 1].tolist() == new_free[:first + 1]
        assert (tokens[b, L + first + 1:] == eos).all(), b
    assert int(n_gen[0]) <= 3
    # the config's eos is the default
    model.cfg.eos_token_id = eos
    try:
        again, n_again = generate(model, ids, lens, max_new=max_new,
                                  temperature=0.0)
    finally:
        model.cfg.eos_token_id = None
    assert torch.equal(again, tokens) and torch.equal(n_again, n_gen)
    with pytest.raises(ValueError):
        generate(model, ids, lens, max_new=2, eos_token_id=61)


def test_generate_sampled_is_a_function_of_the_seed(greedy_run):
    model, ids, lens, max_new, free, _ = greedy_run
    kw = dict(max_new=max_new, temperature=1.0, top_k=30, top_p=0.95)
    with _no_host_reads():
        a, _ = generate(model, ids, lens, seed=5, **kw)
        b, _ = generate(model, ids, lens, seed=5, **kw)
        c, _ = generate(model, ids, lens, seed=6, **kw)
    assert torch.equal(a, b)
    assert not torch.equal(a, c)
    assert not torch.equal(a, free)
    assert int(a.min()) >= 0 and int(a.max()) < 61


# --------------------------------------------------------------------- tool
def test_tool_filters_need_device_sampling(capsys):
    mod = _load_tool()
    for extra in (["--top-k", "5"], ["--top-p", "0.9"]):
        with pytest.raises(SystemExit) as e:
            mod.main(["--ckpt", "none.pt", "--tokenizer", TOK_DIR] + extra)
        assert e.value.code == 2
        assert "--device-sampling" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        mod.main(["--ckpt", "none.pt", "--tokenizer", TOK_DIR,
                  "--device-sampling", "--top-p", "0"])


def test_tool_device_sampling(tmp_path):
    from tokenizers import Tokenizer
    from acco_amd.config import load_config
    from acco_amd.models import build_model
    tok = Tokenizer.from_file(os.path.join(TOK_DIR, "tokenizer.json"))
    cfg = load_config(TOOL_OVERRIDES)
    torch.manual_seed(0)
    model = build_model(cfg.model, vocab_size_override=tok.get_vocab_size())
    ckpt = tmp_path / "m.pt"
    torch.save(model.state_dict(), str(ckpt))
    mod = _load_tool()
    base = ["--ckpt", str(ckpt), "--tokenizer", TOK_DIR, "--prompt", "the",
            "--max-new", "8", "--device-sampling"]
    greedy = mod.main(base + ["--temperature", "0.0"] + TOOL_OVERRIDES)
    assert isinstance(greedy, str) and greedy.startswith("the")
    sampled = [mod.main(base + ["--temperature", "0.9", "--top-k", "50",
                                "--top-p", "0.9", "--seed", s]
                        + TOOL_OVERRIDES) for s in ("7", "7", "8")]
    assert sampled[0] == sampled[1] and sampled[0].startswith("the")
    assert sampled[0] != sampled[2]
    # prompt + max-new must fit the cache, as with --kv-cache
    with pytest.raises(ValueError):
        mod.main(base + ["--max-new", "100"] + TOOL_OVERRIDES)
