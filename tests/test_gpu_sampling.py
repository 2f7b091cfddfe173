"""acco_sample_logits (sample.hip) on the GPU against the fp64 reference
(torch_ref.sample_logits), and models.generate in bf16.

thr and n_kept are integers of the bf16 keys: bit-exact. token is exact too.
Both hold only where the reference itself is not within the kernel's fp32
error of a decision boundary; those preconditions are asserted on the
reference alone, for every row of every case (the seeds below satisfy them;
no row is skipped).

top-p precondition. The kernel's mass of element i is
    trunc(2^s · fl(exp2(fl(fl(x_i - max) · c2)))),  c2 = fl(log2(e) / T),
s = min(40, 62 - ceil(log2 V)), summed as integers (exactly, in any order).
x_i - max is a difference of two bf16: exact, or rounded (2^-24) when the
exponents lie more than 16 apart; c2 and the product add 2^-24 each, so the
exponent a_i = (x_i - max) / T carries 3·2^-24·|a_i|, which exp turns into
the same relative error of the mass; v_exp_f32 is a 1-ulp instruction
(2^-23); truncation loses at most 2^-s of the largest mass (= 1) per element.
With p the distribution over the top-k survivors, a cumulative share
mass(x >= v) / Z is a ratio of two such sums, so it is off by at most
    E = 2 · (2^-23 + 3·2^-24 · sum_i p_i |a_i| + (V + 1) · 2^-s)
(the + 1: the integer target ceil(Z · top_p)). The cases need every distinct
value's share to differ from top_p by more than 2·E (first order doubled).

token precondition. score_i = x_i / T + g_i, g_i = -log(-log(u_i)), u_i exact.
Division is correctly rounded (2^-24·|x/T|); logf is a 1-ulp function: the
inner one shifts g by 2^-23 absolutely, the outer adds 2^-23·|g|; the sum
rounds once (2^-24·(|x/T| + |g|)). Together at most
    2^-24 · (2|x/T| + 3|g| + 2)  <=  4 · 2^-24 · (|x/T| + |g| + 1)
per score, so two scores cannot change order while their gap exceeds
c · 2^-24 · scale with c = 8 and scale the larger |x/T| + |g| + 1 of the two.
Asserted for the runner-up in that form, and pairwise against every other
kept element with the sum of both scales (4 · 2^-24 · (scale_i + scale_j)).

logprob = a_tok - log(Z_kept): fl(fl(x_tok - max) / T) carries 2^-23·|a_tok|,
Z_kept the mass error above (without the ratio's factor 2) plus its
conversion to fp32 (2^-24), logf 2^-23·|log Z|, the difference 2^-24·|logprob|:
    L = 2^-23·(|a_tok| + |log Z| + 1) + 3·2^-24·sum_i p_i|a_i| + V·2^-s
        + 2^-24·(1 + |logprob|);
the limit is 2·L (first order doubled).

MEASURED (MI355X, one run): smallest gap / limit of any row 5.35e+03
(V = 128256, no filter), worst logprob err / limit 0.151 (V = 50257, top-k 50
with top-p 0.9); RESULTS.md, "On-device sampling".
"""

import functools
import math

import pytest
import torch

from acco_amd import ops
from acco_amd.models import (GPTNeoConfig, GPTNeoForCausalLM, LlamaConfig,
                             LlamaForCausalLM, generate)
from acco_amd.models.kv_cache import KVCache
from acco_amd.ops import torch_ref
from tests import streaming_ref as sr

pytestmark = pytest.mark.gpu
DEV = "cuda"

B = 3
VOCABS = [1, 7, 8, 9, 255, 256, 257, 2049, 50257, 128256]
T = 0.8
SEED, STEP = 0x5EEDC0DE12345678, 2 ** 33 + 7
C_GAP = 8.0


def _configs(V):
    """(top_k, top_p) of every filter case at vocabulary V."""
    ks = [(k, 1.0) for k in (1, 2, 50, V, V + 1)]
    ps = [(0, p) for p in (0.1, 0.9, 0.999)]
    return ks + ps + [(50, 0.9), (0, 1.0)]


# The first generator tag per V whose rows meet every precondition of every
# case below, found by running the reference alone (0 where not listed).
SEED_TAGS = {2049: 7, 50257: 37, 128256: 6}


@functools.lru_cache(maxsize=None)
def _logits(V, tag=None):
    """randn · 3 in bf16, [B, V] with row stride V: odd V walks every 16-byte
    alignment."""
    tag = SEED_TAGS.get(V, 0) if tag is None else tag
    g = sr.case_generator("sample_logits_%d_%d" % (V, tag))
    return (torch.randn(B, V, generator=g) * 3).bfloat16()


@functools.lru_cache(maxsize=None)
def _reference(V, top_k, top_p, temperature=T):
    det = []
    out = torch_ref.sample_logits(_logits(V), temperature=temperature,
                                  top_k=top_k, top_p=top_p, seed=SEED,
                                  step=STEP, details=det)
    return out, det


def _shift(V):
    return min(40, 62 - max(V - 1, 0).bit_length())


def _mass_error(V, d):
    return (2.0 ** -23 + 3 * 2.0 ** -24 * d["mean_abs_a"]
            + (V + 1) * 2.0 ** -_shift(V))


def _check_preconditions(V, top_p, det):
    """On the reference alone. Returns the smallest gap / limit."""
    worst = math.inf
    for b, d in enumerate(det):
        if top_p < 1.0:
            need = 2 * 2 * _mass_error(V, d)
            assert d["p_margin"] > need, (V, top_p, b, d["p_margin"], need)
        limit = C_GAP * 2.0 ** -24 * d["gap_scale"]
        assert d["gap"] > limit, (V, b, d["gap"], limit)
        assert d["gap_pairwise"] > 4 * 2.0 ** -24, (V, b, d["gap_pairwise"])
        worst = min(worst, d["gap"] / limit)
    return worst


def _logprob_limit(V, d):
    lp = d["a_tok"] - d["log_z"]
    L = (2.0 ** -23 * (abs(d["a_tok"]) + abs(d["log_z"]) + 1)
         + 3 * 2.0 ** -24 * d["mean_abs_a"] + V * 2.0 ** -_shift(V)
         + 2.0 ** -24 * (1 + abs(lp)))
    return 2 * L


def _bits(t):
    return t.cpu().contiguous().view(torch.int16)


def _compare(V, top_k, top_p, got, temperature=T):
    (tok, lp, thr, n), det = _reference(V, top_k, top_p, temperature)
    ratio = _check_preconditions(V, top_p, det)
    g_tok, g_lp, g_thr, g_n = got
    assert g_tok.dtype == torch.int64 and g_lp.dtype == torch.float32
    assert g_thr.dtype == torch.bfloat16 and g_n.dtype == torch.int32
    assert torch.equal(_bits(g_thr), _bits(thr)), (V, top_k, top_p)
    assert torch.equal(g_n.cpu(), n), (V, top_k, top_p)
    assert torch.equal(g_tok.cpu(), tok), (V, top_k, top_p)
    worst = 0.0
    for b, d in enumerate(det):
        err = abs(float(g_lp[b]) - (d["a_tok"] - d["log_z"]))
        worst = max(worst, err / _logprob_limit(V, d))
    print("SAMPLE V=%d k=%d p=%g gap/limit %.3g logprob err/limit %.3g"
          % (V, top_k, top_p, ratio, worst))
    assert worst <= 1.0, (V, top_k, top_p, worst)
    return ratio, worst


@pytest.mark.parametrize("V", VOCABS)
def test_filters_token_and_logprob(V):
    x = _logits(V).to(DEV)
    assert x.stride(0) == V or V == 1
    for top_k, top_p in _configs(V):
        got = ops.sample_logits(x, temperature=T, top_k=top_k, top_p=top_p,
                                seed=SEED, step=STEP)
        _compare(V, top_k, top_p, got)


@pytest.mark.parametrize("V", [257, 2049])
def test_padded_stride_and_unaligned_base(V):
    """Rows V + 5 elements apart inside a buffer that starts 2 bytes past a
    16-byte boundary; the padding holds NaN and +inf, which must not be
    read as logits."""
    x = _logits(V)
    buf = torch.full((1 + B * (V + 5),), float("nan"), dtype=torch.bfloat16)
    buf[1::2] = float("inf")
    view = buf[1:].view(B, V + 5)[:, :V]
    view.copy_(x)
    dbuf = buf.to(DEV)
    dview = dbuf[1:].view(B, V + 5)[:, :V]
    assert dview.data_ptr() % 16 == 2 and dview.stride(0) == V + 5
    for top_k, top_p in [(50, 0.9), (0, 1.0)]:
        got = ops.sample_logits(dview, temperature=T, top_k=top_k,
                                top_p=top_p, seed=SEED, step=STEP)
        _compare(V, top_k, top_p, got)


@pytest.mark.parametrize("V", [9, 257, 50257])
def test_greedy_is_lowest_index_argmax(V):
    x = _logits(V).clone()
    x[1] = x[1].clamp(max=2.0)            # a tie row: many elements at 2.0
    x[2, V // 2:] = x[2].max()            # and one tied over half the row
    want = torch.stack([(r == r.max()).nonzero()[0, 0] for r in x.float()])
    assert int((x[1] == 2.0).sum()) > 1 or V < 50
    tok, lp, thr, n = ops.sample_logits(x.to(DEV), temperature=0.0, top_k=1,
                                        top_p=0.5, seed=SEED, step=STEP)
    det = []
    r_tok, r_lp, r_thr, r_n = torch_ref.sample_logits(
        x, temperature=0.0, top_k=1, top_p=0.5, seed=SEED, step=STEP,
        details=det)
    assert torch.equal(tok.cpu(), want) and torch.equal(r_tok, want)
    assert torch.equal(n.cpu(), r_n) and n.tolist() == [V] * B
    assert torch.equal(_bits(thr), _bits(r_thr))
    # the unfiltered T = 1 softmax, within the logprob limit above
    want_lp = torch.log_softmax(x.double(), -1)[torch.arange(B), want]
    for b, d in enumerate(det):
        assert abs(d["a_tok"] - d["log_z"] - float(want_lp[b])) < 1e-12
        err = abs(float(lp[b]) - float(want_lp[b]))
        assert err <= _logprob_limit(V, d), (V, b, err)


def test_special_values():
    nan, inf = float("nan"), float("inf")
    rows = [[nan] * 9, [-inf] * 9,
            [-inf, -1.0, nan, inf, -inf, 0.5, nan, -2.0, 1.0],
            [-0.0, 0.0, -0.0, -1.0, 0.0, -0.0, -3.0, 0.0, -0.0],
            [nan, -1.0, nan, -2.0, nan, nan, nan, nan, nan]]
    x = torch.tensor(rows).bfloat16()
    for temperature, top_k, top_p in [(1.0, 0, 1.0), (1.0, 3, 1.0),
                                      (1.0, 1, 1.0), (0.7, 0, 0.6),
                                      (0.7, 8, 0.9), (0.0, 0, 1.0)]:
        got = ops.sample_logits(x.to(DEV), temperature=temperature,
                                top_k=top_k, top_p=top_p, seed=3, step=1)
        det = []
        want = torch_ref.sample_logits(x, temperature=temperature,
                                       top_k=top_k, top_p=top_p, seed=3,
                                       step=1, details=det)
        case = (temperature, top_k, top_p)
        if temperature > 0 and top_p < 1.0:
            for d in det:
                assert d["p_margin"] > 4 * _mass_error(9, d), case
        assert ((got[0] >= 0) & (got[0] < 9)).all(), case
        assert torch.equal(got[3].cpu(), want[3]), case
        assert torch.equal(_bits(got[2]), _bits(want[2])), case
        assert torch.isfinite(got[1]).all(), case
        for b, d in enumerate(det):       # where the draw is decided, equal
            if d["gap"] > C_GAP * 2.0 ** -24 * d["gap_scale"]:
                assert int(got[0][b]) == d["token"], (case, b)
    assert int(got[0][0]) == 0 and int(got[3][0]) == 0      # all NaN


def test_done_and_eos():
    V = 2049
    x = _logits(V).to(DEV)
    (tok0, _, _, _), _ = _reference(V, 50, 0.9)
    eos = int(tok0[1])
    done = torch.tensor([1, 0, 0], dtype=torch.uint8, device=DEV)
    tok, lp, thr, n = ops.sample_logits(x, temperature=T, top_k=50,
                                        top_p=0.9, seed=SEED, step=STEP,
                                        done=done, eos_id=eos)
    assert int(tok[0]) == eos and int(n[0]) == 0 and float(lp[0]) == 0.0
    assert tok[1:].tolist() == tok0[1:].tolist()
    assert done.tolist() == [1, 1, int(int(tok0[2]) == eos)]
    with pytest.raises(RuntimeError):
        ops.sample_logits(x, temperature=T, seed=0, step=0, done=done,
                          eos_id=V)
    with pytest.raises(RuntimeError):
        ops.sample_logits(x, temperature=T, seed=0, step=0,
                          done=done.cpu(), eos_id=0)
    with pytest.raises(RuntimeError):
        ops.sample_logits(x[:, ::2], temperature=T, seed=0, step=0)
    with pytest.raises(RuntimeError):
        ops.sample_logits(x, temperature=-1.0, seed=0, step=0)
    with pytest.raises(RuntimeError):
        ops.sample_logits(x, temperature=T, top_p=0.0, seed=0, step=0)


def test_reproducible_and_step_dependent():
    V = 128256
    x = _logits(V).to(DEV)
    kw = dict(temperature=T, top_k=0, top_p=0.999, seed=SEED)
    a = ops.sample_logits(x, step=STEP, **kw)
    b = ops.sample_logits(x, step=STEP, **kw)
    assert torch.equal(a[0], b[0]) and torch.equal(a[3], b[3])
    assert torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    assert torch.equal(_bits(a[2]), _bits(b[2]))
    c = ops.sample_logits(x, step=STEP + 1, **kw)
    assert not torch.equal(a[0], c[0])
    assert torch.equal(a[3], c[3]) and torch.equal(_bits(a[2]), _bits(c[2]))


def test_dispatch_reaches_the_kernel(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("torch reference used for CUDA bf16 logits")
    monkeypatch.setattr(torch_ref, "sample_logits", boom)
    x = _logits(257).to(DEV)
    ops.sample_logits(x, temperature=T, seed=0, step=0)
    with pytest.raises(AssertionError):
        ops.sample_logits(x.float(), temperature=T, seed=0, step=0)


# ----------------------------------------------------------------- generate
def _model(family):
    torch.manual_seed(0)
    if family == "llama":
        cfg = LlamaConfig(hidden_size=256, num_layers=2, num_heads=4,
                          num_kv_heads=2, intermediate_size=512,
                          vocab_size=515, max_position_embeddings=512)
        model = LlamaForCausalLM(cfg)
    else:
        cfg = GPTNeoConfig(hidden_size=128, num_layers=2, num_heads=2,
                           vocab_size=515, max_position_embeddings=256,
                           window_size=16)
        model = GPTNeoForCausalLM(cfg)
    return model.to(DEV, dtype=torch.bfloat16).eval()


@pytest.mark.parametrize("family", ["llama", "gptneo"])
def test_generate_bf16(family):
    model = _model(family)
    g = sr.case_generator("generate_%s" % family)
    ids = torch.randint(0, 515, (3, 21), generator=g).to(DEV)
    lens = torch.tensor([21, 5, 13], device=DEV)
    max_new = 10
    tokens, n_gen = generate(model, ids, lens, max_new=max_new,
                             temperature=0.0)
    assert n_gen.tolist() == [max_new] * 3
    # the same loop with the argmax on the host
    cache = KVCache.allocate(model, 3, 21 + max_new)
    logits = model.prefill(ids, lens, cache)
    for i in range(max_new):
        host = logits.float().cpu()
        nxt = torch.stack([(r == r.max()).nonzero()[0, 0] for r in host])
        for b in range(3):
            assert int(tokens[b, int(lens[b]) + i]) == int(nxt[b]), (b, i)
        if i + 1 < max_new:
            logits = model.decode_step(nxt.to(DEV), cache)
    for b in range(3):
        assert torch.equal(tokens[b, :int(lens[b])], ids[b, :int(lens[b])])
    kw = dict(max_new=max_new, temperature=0.9, top_k=40, top_p=0.95)
    a, _ = generate(model, ids, lens, seed=11, **kw)
    b2, _ = generate(model, ids, lens, seed=11, **kw)
    c, _ = generate(model, ids, lens, seed=12, **kw)
    assert torch.equal(a, b2) and not torch.equal(a, c)
    assert int(a.min()) >= 0 and int(a.max()) < 515
    # eos: sequence 0's third greedy token ends it
    eos = int(tokens[0, 21 + 2])
    stopped, n_stop = generate(model, ids, lens, max_new=max_new,
                               temperature=0.0, eos_token_id=eos)
    first = tokens[0, 21:].tolist().index(eos)
    assert int(n_stop[0]) == first + 1 <= 3
    assert (stopped[0, 21 + first:] == eos).all()
    assert torch.equal(stopped[0, :21 + first + 1], tokens[0, :21 + first + 1])
