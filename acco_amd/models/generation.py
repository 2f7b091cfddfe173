"""Generation loop on a KV cache with on-device sampling: one `prefill`, then
per token one `ops.sample_logits` and one `decode_step`. Between the prompt
and the result nothing is read on the host: the sampler draws on the device
from a counter-based generator keyed by (seed, step), `done` flags live on
the device, and the output buffer is preallocated. Stopping early once every
sequence is done would need a host read per token, so all `max_new` steps
run and finished sequences emit `eos_token_id`."""

from __future__ import annotations

from typing import Optional, Tuple

import torch

from acco_amd import ops
from acco_amd.models.kv_cache import KVCache, prefill_chunked


@torch.no_grad()
def generate(model, input_ids: torch.Tensor,
             lens: Optional[torch.Tensor] = None, *, max_new: int,
             temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0,
             seed: int = 0, eos_token_id: Optional[int] = None,
             prefill_chunk: int = 0,
             kv_dtype: Optional[torch.dtype] = None,
             weight_dtype: Optional[torch.dtype] = None,
             draft=None, spec_k: int = 4,
             act_dtype: Optional[torch.dtype] = None
             ) ->Tuple[torch.Tensor, torch.Tensor]:
    """(tokens int64 [B, S + max_new], n_generated int64 [B]) for prompts
    `input_ids` [B, S] of `model` (LlamaForCausalLM or GPTNeoForCausalLM, in
    eval mode). Sequence b holds lens[b] <= S prompt tokens (None = all S),
    the rest of its row is right-padding; its new tokens start at column
    lens[b], and columns past lens[b] + max_new hold `eos_token_id` (0
    without one). Needs S + max_new <= max_position_embeddings.

    temperature / top_k / top_p / seed: ops.sample_logits, with the step index
    as the generator's counter, so the same arguments give the same tokens;
    temperature 0 is greedy. eos_token_id (default: model.cfg.eos_token_id;
    None = never stop): once sequence b draws it, b emits it from then on;
    n_generated[b] counts b's tokens up to and including its first eos.
    prefill_chunk (0 < prefill_chunk < S): the prompt goes through the cache
    in slices of that many columns (kv_cache.prefill_chunked), which bounds
    the prefill's activation memory; 0 = one prefill of the whole prompt.
    kv_dtype: the dtype of the KV cache (KVCache.allocate; None = the
    model's); torch.float8_e4m3fn stores it quantised, about half the bytes
    per cached token.
    weight_dtype: None = the model's own linears; torch.float8_e4m3fn
    generates from quant.quantize_weights(model) (e4m3 weight codes with one
    scale per output row, ops.linear_w8), about half the weight bytes per
    token; the copy is made per call, so quantise once and pass the result
    when generating more than once (a model that already holds W8Linears is
    used as it is). torch.float4_e2m1fn_x2 does the same in OCP MXFP4
    (quantize_weights(model, dtype), ops.linear_w4): e2m1 codes with one
    power-of-two scale per 32 weights, about 0.53 bytes per weight; a model
    that already holds quantised linears of either kind is used as it is.
    Calls of more than 64 rows (the prefill, prefill_chunk slices, a
    speculative round of a large batch) run ops.gemm_w8 / ops.gemm_w4, HIP
    kernels that read the codes as codes, up to ops.W8_GEMM_MAX_ROWS /
    ops.W4_GEMM_MAX_ROWS rows.
    act_dtype: passed to quantize_weights when this call quantises the model
    itself (weight_dtype torch.float4_e2m1fn_x2 only; None = off; a model
    that is already quantised keeps its own setting). With
    torch.float8_e4m3fn the prompt-width calls (65 rows and more: the
    prefill, prefill_chunk slices) see activations rounded to OCP MXFP8 and
    run ops.gemm_w4a8 on the block-scaled MFMA; decode-width calls do not:
    they stay weight-only.
    draft: a model of the same interface and vocab_size (for one,
    quantize_weights(model, torch.float4_e2m1fn_x2) of `model` itself) turns
    on speculative decoding, spec_k >= 1 drafted tokens per round
    (_generate_speculative has the loop): the tokens are distributed as
    without a draft, and greedy ones are the target's own argmax of the logits
    it computes; the draws differ from the plain loop's for the same seed.
    top_k / top_p are not supported with a draft (ValueError); weight_dtype
    applies to `model` only; needs S + max_new + spec_k + 1 <=
    max_position_embeddings of both models. None: the loop above, unchanged."""
    if input_ids.dim() != 2:
        raise ValueError(f"input_ids must be [B, S], got {input_ids.shape}")
    if weight_dtype is not None:
        from acco_amd.models.quant import (has_quantized_linears,
                                           quantize_weights)
        if weight_dtype not in (torch.float8_e4m3fn,
                                torch.float4_e2m1fn_x2):
            raise ValueError("weight_dtype must be None, torch.float8_e4m3fn "
                             f"or torch.float4_e2m1fn_x2, got {weight_dtype}")
        if not has_quantized_linears(model):
            model = quantize_weights(model, weight_dtype, act_dtype)
    elif act_dtype is not None:
        raise ValueError("act_dtype needs weight_dtype="
                         "torch.float4_e2m1fn_x2")
    B, S = input_ids.shape
    max_new = int(max_new)
    if max_new < 0:
        raise ValueError(f"max_new must be >= 0, got {max_new}")
    cfg = model.cfg
    if eos_token_id is None:
        # a config's eos of another vocabulary (vocab_size overridden) is
        # not a token of this model: never stop
        eos_token_id = getattr(cfg, "eos_token_id", None)
        if (eos_token_id is not None
                and not 0 <= int(eos_token_id) < cfg.vocab_size):
            eos_token_id = None
    elif not 0 <= int(eos_token_id) < cfg.vocab_size:
        raise ValueError(f"eos_token_id must be in [0, {cfg.vocab_size}), "
                         f"got {eos_token_id}")
    if draft is not None:
        _check_draft(model, draft, spec_k, top_k, top_p, S + max_new)
    dev = input_ids.device
    total = S + max_new
    if lens is None:
        start = torch.full((B,), S, device=dev, dtype=torch.long)
    else:
        start = lens.to(device=dev, dtype=torch.long).clamp(1, S)  # as prefill
    fill = 0 if eos_token_id is None else int(eos_token_id)
    tokens = torch.full((B, total), fill, device=dev, dtype=torch.long)
    prompt = torch.arange(S, device=dev)[None, :] < start[:, None]
    tokens[:, :S] = torch.where(prompt, input_ids, tokens[:, :S])
    n_generated = torch.zeros(B, device=dev, dtype=torch.long)
    if max_new == 0:
        return tokens, n_generated
    done = None
    if eos_token_id is not None:
        done = torch.zeros(B, device=dev, dtype=torch.uint8)
    if draft is not None:
        return _generate_speculative(
            model, draft, int(spec_k), input_ids, lens, start, tokens, done,
            max_new, float(temperature), seed, eos_token_id,
            int(prefill_chunk), kv_dtype)
    cache = KVCache.allocate(model, B, total, dtype=kv_dtype)
    if 0 < int(prefill_chunk) < S:
        logits = prefill_chunked(model, input_ids, lens, cache, prefill_chunk)
    else:
        logits = model.prefill(input_ids, lens, cache)
    for i in range(max_new):
        if done is None:
            n_generated += 1
        else:
            n_generated += done == 0
        tok, _, _, _ = ops.sample_logits(
            logits, temperature=temperature, top_k=top_k, top_p=top_p,
            seed=seed, step=i, done=done,
            eos_id=-1 if eos_token_id is None else int(eos_token_id))
        tokens.scatter_(1, (start + i)[:, None], tok[:, None])
        if i + 1 < max_new:
            logits = model.decode_step(tok, cache)
    return tokens, n_generated


def _check_draft(model, draft, spec_k, top_k, top_p, total: int) -> None:
    if int(top_k) != 0 or float(top_p) < 1.0:
        raise ValueError("generate(draft=...) supports neither top_k nor "
                         "top_p: the verification compares unfiltered "
                         "distributions")
    if int(spec_k) < 1:
        raise ValueError(f"spec_k must be >= 1, got {spec_k}")
    for name in ("prefill", "decode_step", "extend"):
        if not callable(getattr(draft, name, None)):
            raise ValueError(f"draft has no {name}(): it must be a model of "
                             "the same interface as the target")
    v_d = getattr(getattr(draft, "cfg", None), "vocab_size", None)
    if v_d != model.cfg.vocab_size:
        raise ValueError(f"draft vocab_size {v_d} is not the target's "
                         f"{model.cfg.vocab_size}")
    need = total + int(spec_k) + 1
    for m in (model, draft):
        if need > int(m.cfg.max_position_embeddings):
            raise ValueError(
                f"speculative decoding needs S + max_new + spec_k + 1 = "
                f"{need} <= max_position_embeddings = "
                f"{m.cfg.max_position_embeddings}")


def _generate_speculative(model, draft, k, input_ids, lens, start, tokens,
                          done, max_new, temperature, seed, eos_token_id,
                          prefill_chunk, kv_dtype):
    """The loop of generate(draft=...). State per sequence b: n[b] tokens
    produced, both caches valid below L[b] = start[b] - 1 + n[b], last[b] the
    token at position L[b] (at first the prompt's last token: its cache row is
    written again by round 0). A round:
      1  the draft takes k decode_step + sample_logits from last, keeping its
         k logits rows, and one more decode_step on x_{k-1}, so that its
         cache covers positions L .. L + k like the target's;
      2  the target scores [last, x_0 .. x_{k-1}] in one extend with
         n_new = 0 (its lens stay): p_0 .. p_k;
      3  ops.spec_verify: n_accept drafted tokens and the token after them;
      4  those n_accept + 1 tokens go to columns start + n .., on the device;
         writes stop at the sequence's first eos and at column
         start + max_new, and a sequence that is done or full does not move;
      5  both caches are set to the new L; their rows beyond it are stale and
         are overwritten by the next round (the argument of right-padding).
    The host cannot know n, so it reads one int64 [2] per round: min n (done
    sequences count as full) ends the loop at max_new, max n bounds the
    caches' host-side step count. Draft draws use generator steps r k + j,
    the verification step r, in its own counter range."""
    B, S = input_ids.shape
    dev = input_ids.device
    eos = -1 if eos_token_id is None else int(eos_token_id)
    rows = S + max_new + k + 1
    caches = [KVCache.allocate(m, B, rows, dtype=kv_dtype)
              for m in (model, draft)]
    for m, c in zip((model, draft), caches):
        if 0 < prefill_chunk < S:
            prefill_chunked(m, input_ids, lens, c, prefill_chunk)
        else:
            m.prefill(input_ids, lens, c)
    # one spare column takes the masked writes
    out = torch.cat([tokens, tokens[:, :1]], dim=1)
    spare = out.shape[1] - 1
    n = torch.zeros(B, device=dev, dtype=torch.long)
    last = input_ids.gather(1, (start - 1)[:, None])[:, 0]
    j = torch.arange(k + 1, device=dev)[None, :]
    zero = torch.zeros(B, device=dev, dtype=torch.int32)
    n_max, r = 0, 0
    while True:
        for c in caches:
            c.begin(S - 1 + n_max, start - 1 + n)
        tok, xs, q_rows = last, [], []
        for i in range(k):
            q_rows.append(draft.decode_step(tok, caches[1]))
            tok = ops.sample_logits(q_rows[-1], temperature=temperature,
                                    seed=seed, step=r * k + i)[0]
            xs.append(tok)
        draft.decode_step(tok, caches[1])
        xs = torch.stack(xs, dim=1)                               # [B, k]
        p_logits = model.extend(torch.cat([last[:, None], xs], dim=1),
                                caches[0], n_new=zero)
        was_done = None if done is None else done != 0
        n_accept, nxt, _ = ops.spec_verify(
            p_logits, torch.stack(q_rows, dim=1), xs,
            temperature=temperature, seed=seed, step=r, done=done, eos_id=eos)
        new = torch.cat([xs, nxt[:, None]], dim=1)
        new = torch.where(j == n_accept[:, None], nxt[:, None], new)
        write = (j <= n_accept[:, None]) & (j < (max_new - n)[:, None])
        if done is not None:
            write &= ~was_done[:, None]
            hit = (new == eos) & write
            write &= (hit.cumsum(1) - hit.long()) == 0     # up to the first eos
            done.copy_(was_done | (hit & write).any(1))
        cols = torch.where(write, (start + n)[:, None] + j, spare)
        out.scatter_(1, cols, new)
        adv = write.sum(1)
        last = torch.where(adv > 0,
                           new.gather(1, (adv - 1).clamp(min=0)[:, None])[:, 0],
                           last)
        n = n + adv
        full = n if done is None else torch.where(done != 0, max_new, n)
        n_min, n_max = torch.stack([full.min(), n.max()]).tolist()
        r += 1
        if n_min >= max_new:
            return out[:, :spare].contiguous(), n
