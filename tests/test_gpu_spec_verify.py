"""acco_spec_verify (spec_verify.hip) on the GPU against the fp64 reference
(torch_ref.spec_verify), and models.generate(draft=...) in bf16.

n_accept and next_token are compared bit for bit. That holds only where the
reference is not within the kernel's fp32 error of a decision, so the
preconditions below are asserted on the reference alone, for every decision
that reaches an output (the seeds satisfy them; nothing is skipped).

Error of a probability. The kernel's p_i = fl(e_i · r), e_i =
exp2(fl(fl(x_i - max) · c2)), c2 = fl(log2(e) / T), r = fl(1 / fl(Z)),
Z = sum_i trunc(2^s · e_i) · 2^-s summed as integers (exactly),
s = min(40, 62 - ceil(log2 V)). As for the sampler (test_gpu_sampling.py): the
exponent a_i = (x_i - max) / T carries 3·2^-24·|a_i|, which exp2 turns into
that relative error of e_i, plus 2^-23 for v_exp_f32; Z carries 2^-23 +
3·2^-24·sum_j p_j |a_j| from its terms and V·2^-s from the truncation (Z >= 1);
its conversion to fp32, the division and the product round once each
(3·2^-24). Relative error of p_i at most
    E_i = 2^-24 · (7 + 3 |a_i| + 3 sum_j p_j |a_j|) + V · 2^-s.
accept test: fl(u · q(x)) < p(x) adds one rounding (2^-24) to the left side,
so the decision is the reference's while
    |u q(x) - p(x)| > 2 · (u q(x) (E_q + 2^-24) + p(x) E_p)     (first order
doubled). accept_prob = min(1, fl(p / q)) is off by at most
2 · (E_p + E_q + 2^-24) relative.
residual: r_i = p_i - q_i is off by at most err_i = 2 (E_p,i p_i + E_q,i q_i):
the cancellation keeps the absolute error of its operands. The kernel's score
logf(r) + g, both 1-ulp logs and one rounded sum, is off by
4 · 2^-24 · (|log r| + |g| + 1) as the sampler's, so the reference's winner w
is the kernel's while, for every other i with p_i > 0,
    log(r_w - err_w) + g_w - (log(max(r_i, 0) + err_i) + g_i)
        > 4 · 2^-24 · (scale_w + scale_i),
scale = |log(.)| + |g| + 1 of those perturbed residuals: this also covers an
i whose residual changes sign. The draw from p_k is the sampler's, with its
pairwise rule on x / T + g.

MEASURED (MI355X, one run): smallest margin / limit of any case 6.4e3
(V = 1001, k = 4, B = 3, T = 1.5), worst accept_prob err / bound 0.104
(V = 1001, k = 1, B = 3, T = 0.7); RESULTS.md, "Speculative decoding".
"""

import copy
import functools
import math

import numpy as np
import pytest
import torch

from acco_amd import ops
from acco_amd.models import (LlamaConfig, LlamaForCausalLM, generate,
                             quantize_weights)
from acco_amd.ops import torch_ref
from tests import streaming_ref as sr

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED, STEP = 0x5EEDC0DE12345678, 2 ** 33 + 7
U = 2.0 ** -24


def _shift(V):
    return min(40, 62 - max(V - 1, 0).bit_length())


@functools.lru_cache(maxsize=None)
def _case(V, k, B, temperature):
    """(p, q, x, reference outputs, details). q is p plus unit noise; the
    drafted tokens make sequence 0 all-accepted (tokens with p >= q),
    sequence 1 rejected at 0 and sequence 2 mid-way, at k // 2 (there token
    1, or 0 at V = 1, gets p(x) / q(x) far below 2^-24, the smallest u);
    B = 1 takes the mid-way pattern."""
    g = sr.case_generator("spec_verify_%d_%d_%d" % (V, k, B))
    p = (torch.randn(B, k + 1, V, generator=g) * 3).bfloat16()
    q = (p[:, :k].float() + torch.randn(B, k, V, generator=g)).bfloat16()
    T = temperature if temperature > 0 else 1.0
    reject = [(b, 0 if (2 if B == 1 else b) == 1 else k // 2)
              for b in range(B) if B == 1 or b]
    for b, t in reject:
        p[b, t, min(1, V - 1)] = p[b, t].min() - 2
        q[b, t, min(1, V - 1)] = q[b, t].max() + 2
    ratio = (torch.log_softmax(p[:, :k].double() / T, -1)
             - torch.log_softmax(q.double() / T, -1))
    x = p[:, :k].double().argmax(-1) if temperature == 0 \
        else ratio.argmax(-1)
    for b, t in reject:
        x[b, t] = min(1, V - 1)
    det = []
    want = torch_ref.spec_verify(p, q, x, temperature=temperature, seed=SEED,
                                 step=STEP, details=det)
    return p, q, x, want, det


def _rel_err(prob, a, V):
    mean_abs_a = (prob * np.abs(a)).sum(axis=-1, keepdims=True)
    return U * (7 + 3 * np.abs(a) + 3 * mean_abs_a) + V * 2.0 ** -_shift(V)


def _check_preconditions(V, k, x, n_accept, det):
    """On the reference alone, for the decisions that reach an output.
    Returns the smallest margin / limit."""
    worst = math.inf
    for b, n in enumerate(n_accept.tolist()):
        for t in range(min(n + 1, k)):                   # every accept test
            d = det[t]
            e_p = _rel_err(d["p"][b], d["a_p"][b], V)[x[b, t]]
            e_q = _rel_err(d["q"][b], d["a_q"][b], V)[x[b, t]]
            lhs, px = d["u"][b] * d["qx"][b], d["px"][b]
            if lhs == 0 and px == 0:      # two exact zeros in the kernel too
                continue
            limit = 2 * (lhs * (e_q + U) + px * e_p)
            assert abs(lhs - px) > limit, (V, b, t, lhs, px, limit)
            worst = min(worst, abs(lhs - px) / limit)
        d = det[n]
        p, g, w = d["p"][b], d["g"][b], int(d["cand"][b])
        live = p > 0
        if not live.any():                # no finite logit: token 0, no draw
            continue
        if n < k and (p > d["q"][b]).any():              # the residual draw
            r = p - d["q"][b]
            err = 2 * (_rel_err(p, d["a_p"][b], V) * p
                       + _rel_err(d["q"][b], d["a_q"][b], V) * d["q"][b])
            assert r[w] > err[w], (V, b, n)
            hi = np.log(np.maximum(r, 0) + err + 1e-300)
            hi[w] = math.log(r[w] - err[w])
        else:                                            # the draw from p_n
            hi = np.where(live, d["x"][b], 0.0) / d["T"]
        scale = np.abs(hi) + np.abs(g) + 1
        margin = (hi[w] + g[w] - (hi + g)) / (4 * U * (scale[w] + scale))
        margin[w] = math.inf
        margin = margin[live]
        assert margin.min() > 1.0, (V, b, n, margin.min())
        worst = min(worst, float(margin.min()))
    return worst


def _compare(V, k, B, temperature, run):
    p, q, x, (n_want, tok_want, ap_want), det = _case(V, k, B, temperature)
    margin = math.inf
    if temperature > 0:
        margin = _check_preconditions(V, k, x.numpy(), n_want, det)
    n, tok, ap = run(p.to(DEV), q.to(DEV), x.to(DEV))
    assert (n.dtype, tok.dtype, ap.dtype, ap.shape) == (
        torch.int32, torch.int64, torch.float32, (B, k))
    assert torch.equal(n.cpu(), n_want), (V, k, B, temperature)
    assert torch.equal(tok.cpu(), tok_want), (V, k, B, temperature)
    worst = 0.0
    for t in range(k if temperature > 0 else 0):
        d = det[t]
        for b in range(B):
            want = min(1.0, d["px"][b] / d["qx"][b])
            bound = 2 * want * (U + sum(
                _rel_err(d[s][b], d["a_" + s][b], V)[x[b, t]] for s in "pq"))
            worst = max(worst, abs(float(ap[b, t]) - want) / bound)
    if temperature == 0:
        assert torch.equal(ap.cpu(), ap_want)
    print("SPEC V=%d k=%d B=%d T=%g margin/limit %.3g accept_prob err/bound "
          "%.3g n_accept %s" % (V, k, B, temperature, margin, worst,
                                n_want.tolist()))
    assert worst <= 1.0, (V, k, B, temperature, worst)
    return n, tok, ap


@pytest.mark.parametrize("temperature", [0.0, 0.7, 1.5])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("k", [1, 4])
@pytest.mark.parametrize("V", [1, 7, 1001, 8192 + 3, 50257])
def test_kernel_matches_reference(V, k, B, temperature):
    def run(p, q, x):
        return ops.spec_verify(p, q, x, temperature=temperature, seed=SEED,
                               step=STEP)
    a = _compare(V, k, B, temperature, run)
    n_want = _case(V, k, B, temperature)[3][0].tolist()
    if B == 3 and V > 1:          # all accepted, rejected at 0 and mid-way
        assert n_want == [k, 0, k // 2], n_want
    p, q, x = (t.to(DEV) for t in _case(V, k, B, temperature)[:3])
    b = run(p, q, x)                                        # the same bits
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(a[2].view(torch.int32), b[2].view(torch.int32))


@pytest.mark.parametrize("temperature", [0.0, 0.7])
def test_special_values_and_done(temperature):
    nan, inf = float("nan"), float("inf")
    p = torch.tensor([
        [[-inf, 1.0, nan, inf, 0.5, nan, -2.0, inf, -0.0],
         [nan] * 9, [0.0, 1.0, 2.0, 3.0, 2.0, 1.0, 0.0, nan, -inf]],
        [[-0.0, 0.0, -1.0, 2.0, nan, 2.0, -3.0, 0.5, 1.0],
         [1.0, nan, 0.25, -inf, 3.0, 0.0, 0.5, -0.5, 2.5],
         [-inf, 2.0, -inf, 1.0, nan, 0.0, 1.5, -inf, 0.5]]]).bfloat16()
    q = torch.tensor([
        [[0.0, 1.0, 2.0, nan, 0.5, inf, -2.0, 1.5, -0.0], [nan] * 9],
        [[nan] * 9, [1.0, nan, 0.25, -inf, 3.0, 0.0, 0.5, -0.5, 2.5]],
    ]).bfloat16()
    for x in ([[3, 0], [3, 4]], [[5, 1], [4, 1]], [[9, -1], [5, 6]]):
        x = torch.tensor(x)
        det = []
        want = torch_ref.spec_verify(p, q, x, temperature=temperature,
                                     seed=3, step=1, details=det)
        if temperature > 0:
            _check_preconditions(9, 2, x.numpy().clip(0, 8), want[0], det)
        got = ops.spec_verify(p.to(DEV), q.to(DEV), x.to(DEV),
                              temperature=temperature, seed=3, step=1)
        assert torch.equal(got[0].cpu(), want[0]), (x, got, want)
        assert torch.equal(got[1].cpu(), want[1]), (x, got, want)
        assert torch.allclose(got[2].cpu(), want[2], rtol=1e-5, atol=0)
    eos = int(want[1][1])
    done = torch.tensor([1, 0], dtype=torch.uint8, device=DEV)
    n, tok, ap = ops.spec_verify(p.to(DEV), q.to(DEV), x.to(DEV),
                                 temperature=temperature, seed=3, step=1,
                                 done=done, eos_id=eos)
    assert n.tolist() == [0, int(want[0][1])] and tok.tolist() == [eos, eos]
    assert ap[0].tolist() == [0.0, 0.0] and done.tolist() == [1, 1]
    with pytest.raises(RuntimeError):
        ops.spec_verify(p.to(DEV), q.to(DEV), x.to(DEV), temperature=1.0,
                        seed=0, step=0, done=done, eos_id=9)
    with pytest.raises(RuntimeError):
        ops.spec_verify(p.to(DEV), q.to(DEV)[:, :1], x.to(DEV),
                        temperature=1.0, seed=0, step=0)


def test_dispatch_reaches_the_kernel(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("torch reference used for CUDA bf16 logits")
    monkeypatch.setattr(torch_ref, "spec_verify", boom)
    p, q, x, _, _ = _case(1001, 4, 3, 0.7)
    ops.spec_verify(p.to(DEV), q.to(DEV), x.to(DEV), temperature=0.7, seed=0,
                    step=0)
    with pytest.raises(AssertionError):
        ops.spec_verify(p.to(DEV).float(), q.to(DEV).float(), x.to(DEV),
                        temperature=0.7, seed=0, step=0)


def test_generate_with_fp4_draft_bf16():
    """Greedy, k = 3, draft = the MXFP4 copy of the target. Every generated
    token is the argmax of a target row computed by `extend`; rescored by one
    teacher-forced bf16 forward, its logit may trail that row's maximum only
    by what the two paths differ. test_e2e_extend_bf16 bounds the extend
    path at rms(extend - fp64) <= 2 e_full, e_full = rms(bf16 forward - fp64
    forward of the same weights), hence extend versus forward at 3 e_full;
    doubled, because the token and the maximum are two logits that both
    moved: tol = 6 e_full, e_full measured here on the generated rows."""
    torch.manual_seed(0)
    cfg = LlamaConfig(hidden_size=256, num_layers=2, num_heads=4,
                      num_kv_heads=2, intermediate_size=512, vocab_size=515,
                      max_position_embeddings=512)
    model = LlamaForCausalLM(cfg).to(torch.bfloat16).eval()
    ref_model = copy.deepcopy(model).double()
    model = model.to(DEV)
    draft = quantize_weights(model, torch.float4_e2m1fn_x2)
    ids = torch.randint(0, 515, (3, 21), generator=sr.case_generator(
        "generate_spec")).to(DEV)
    lens = torch.tensor([21, 5, 13], device=DEV)
    max_new, k = 10, 3
    rounds = []
    extend = model.extend
    model.extend = lambda *a, **kw: (rounds.append(1), extend(*a, **kw))[1]
    tokens, n_gen = generate(model, ids, lens, max_new=max_new,
                             temperature=0.0, draft=draft, spec_k=k)
    del model.extend
    assert n_gen.tolist() == [max_new] * 3
    with torch.no_grad():
        full = model(tokens)[0].double().cpu()
        ref = ref_model(tokens.cpu())[0]
    worst, errs = 0.0, []
    for b, n in enumerate(lens.tolist()):
        assert torch.equal(tokens[b, :n], ids[b, :n])
        rows = full[b, n - 1:n - 1 + max_new]
        errs.append(rows - ref[b, n - 1:n - 1 + max_new])
        tok = tokens[b, n:n + max_new].cpu()
        assert int(tok.min()) >= 0 and int(tok.max()) < 515
        deficit = rows.max(-1).values - rows.gather(1, tok[:, None])[:, 0]
        worst = max(worst, float(deficit.max()))
    tol = 6 * float(torch.cat(errs).pow(2).mean().sqrt())
    print("E2E spec fp4 draft: worst deficit %.4e tol %.4e, %d rounds, "
          "accepted per round %.2f of %d"
          % (worst, tol, len(rounds),
             max_new / len(rounds) - 1, k))
    assert tol > 0 and worst <= tol, (worst, tol)
