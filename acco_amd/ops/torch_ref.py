"""Pure-PyTorch reference implementations of every hot op.

These are (a) the CPU execution path for tests (this container has no GPU),
and (b) the numerics oracle the gfx950 HIP kernels are validated against
(tests compare HIP output to these run in fp32).

Each docstring cites the reference call-site whose computation the op
replaces (SURVEY.md §2.5 kernel inventory).
"""

from __future__ import annotations

import math
from typing import Optional, Tuple

import torch
import torch.nn.functional as F


def rms_norm(x: torch.Tensor, weight: torch.Tensor, eps: float) -> torch.Tensor:
    """RMSNorm (Llama-family; replaces HF modeling_llama RMSNorm inside K1,
    reference trainer_decoupled.py:26-34 forward)."""
    dt = x.dtype
    # fp32 math for bf16 / fp32 inputs; a double model stays in double
    xf = x.to(torch.promote_types(dt, torch.float32))
    var = xf.pow(2).mean(-1, keepdim=True)
    return (xf * torch.rsqrt(var + eps)).to(dt) * weight


def layer_norm(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor,
               eps: float) -> torch.Tensor:
    """LayerNorm (GPT-Neo family, K1)."""
    return F.layer_norm(x, (x.shape[-1],), weight, bias, eps)


def gelu_new(x: torch.Tensor) -> torch.Tensor:
    """gelu_new / tanh-approximated GELU (GPT-Neo MLP activation,
    reference config/model/gpt-neo-125M.json:2)."""
    return 0.5 * x * (1.0 + torch.tanh(
        math.sqrt(2.0 / math.pi) * (x + 0.044715 * torch.pow(x, 3.0))))


def swiglu(gate: torch.Tensor, up: torch.Tensor) -> torch.Tensor:
    """SwiGLU: silu(gate) * up (Llama MLP, K1)."""
    return F.silu(gate) * up


def rope_cos_sin(seq_len: int, head_dim: int, theta: float,
                 device, dtype=torch.float32) -> Tuple[torch.Tensor, torch.Tensor]:
    """Precomputed RoPE tables, HF-Llama layout: [S, D] with the two halves
    duplicated (cos = cat(c, c), sin = cat(s, s))."""
    inv_freq = 1.0 / (theta ** (torch.arange(0, head_dim, 2, device=device,
                                             dtype=torch.float32) / head_dim))
    t = torch.arange(seq_len, device=device, dtype=torch.float32)
    freqs = torch.outer(t, inv_freq)          # [S, D/2]
    emb = torch.cat((freqs, freqs), dim=-1)   # [S, D]
    return emb.cos().to(dtype), emb.sin().to(dtype)


def _rotate_half(x: torch.Tensor) -> torch.Tensor:
    half = x.shape[-1] // 2
    return torch.cat((-x[..., half:], x[..., :half]), dim=-1)


def rope_apply(q: torch.Tensor, k: torch.Tensor, cos: torch.Tensor,
               sin: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Apply rotary embedding, HF-Llama rotate_half convention.

    q: [B, S, H, D]; k: [B, S, Hkv, D] (the projection's natural contiguous
    layout — the MI355X kernel walks D coalesced with no transpose copies);
    cos/sin: [S, D]."""
    cos = cos.to(q.dtype)[None, :, None, :]
    sin = sin.to(q.dtype)[None, :, None, :]
    q2 = q * cos + _rotate_half(q) * sin
    k2 = k * cos + _rotate_half(k) * sin
    return q2, k2


def doc_start_from_eos(input_ids: torch.Tensor,
                       eos_token_id: int) -> torch.Tensor:
    """Document boundaries of packed rows: int32 [B, S], entry (b, s) is the
    index of the first token of the document that holds token s. A document
    ends with its EOS (the EOS belongs to it); the next token starts a new
    one. Non-decreasing along s, 0 <= out[b, s] <= s, and
    out[b, out[b, s]] == out[b, s]. Plain torch ops, no host sync."""
    B, S = input_ids.shape
    pos = torch.arange(S, device=input_ids.device)
    starts = torch.zeros(B, S, dtype=torch.long, device=input_ids.device)
    # position s starts a document iff token s-1 is an EOS
    starts[:, 1:] = (input_ids[:, :-1] == eos_token_id) * pos[1:]
    return torch.cummax(starts, dim=1).values.to(torch.int32)


def doc_end_from_start(doc_start: torch.Tensor) -> torch.Tensor:
    """The key-side twin of doc_start: int32 [B, S], entry (b, s) is the
    EXCLUSIVE end of the document that holds token s (the next document's
    start, or S). The dkv attention kernel masks with it."""
    B, S = doc_start.shape
    ds = doc_start.long()
    pos = torch.arange(S, device=doc_start.device)
    # a document's last token is followed by a token with another start (or
    # by the row's end); its end is the running minimum from the right
    nxt = torch.full((B, S), S, dtype=torch.long, device=doc_start.device)
    is_last = ds[:, 1:] != ds[:, :-1]
    nxt[:, :-1] = torch.where(is_last, pos[1:], nxt[:, :-1])
    end = torch.flip(torch.cummin(torch.flip(nxt, [1]), dim=1).values, [1])
    return end.to(torch.int32)


def causal_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                     scale: Optional[float] = None,
                     window: Optional[int] = None,
                     doc_start: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Causal (optionally banded/local) attention.

    q: [B, S, H, D]; k, v: [B, S, Hkv, D] (GQA: H a multiple of Hkv) —
    the projections' natural contiguous layout. Returns [B, S, H, D].
    `scale=None` → 1/sqrt(D); GPT-Neo passes scale=1.0 (it does not scale).
    `window` (GPT-Neo local layers, window_size=256): query i attends to
    keys j with i-window < j <= i.
    `doc_start` (int [B, S], see doc_start_from_eos): query i attends only
    to keys j >= doc_start[b, i], i.e. never across a document boundary of
    a packed row; it combines with `window`.
    """
    B, S, H, D = q.shape
    Hkv = k.shape[2]
    q = q.transpose(1, 2)
    k = k.transpose(1, 2)
    v = v.transpose(1, 2)
    if Hkv != H:
        rep = H // Hkv
        k = k.repeat_interleave(rep, dim=1)
        v = v.repeat_interleave(rep, dim=1)
    if scale is None:
        scale = 1.0 / math.sqrt(D)
    # fp32 math for bf16 / fp32 inputs; a double model stays in double
    wide = torch.promote_types(q.dtype, torch.float32)
    scores = torch.matmul(q.to(wide), k.to(wide).transpose(-1, -2)) * scale
    idx = torch.arange(S, device=q.device)
    mask = idx[None, :] > idx[:, None]           # future → masked
    if window is not None:
        mask = mask | (idx[None, :] <= idx[:, None] - window)
    if doc_start is not None:
        lo = doc_start.to(device=q.device, dtype=idx.dtype)   # [B, S] by query
        mask = mask[None, None] | (idx[None, None, None, :] < lo[:, None, :, None])
    scores = scores.masked_fill(mask, float("-inf"))
    probs = torch.softmax(scores, dim=-1)
    out = torch.matmul(probs, v.to(wide)).to(q.dtype)
    return out.transpose(1, 2)


# ------------------------------------------------- KV cache (generation)
# k_cache / v_cache [B, Hkv, Smax, D] per layer, K stored after RoPE;
# cache_len int [B] = tokens already cached per sequence (ragged batches).
# cache_len is data: it is clamped into [0, Smax] and otherwise only
# compared, the convention of the document-mask arrays. No host sync.

@torch.no_grad()
def kv_append(k_cache: torch.Tensor, v_cache: torch.Tensor,
              cache_len: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
              q: Optional[torch.Tensor] = None,
              cos: Optional[torch.Tensor] = None,
              sin: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
    """Write k, v [B, T, Hkv, D] of T new tokens per sequence into the caches,
    in place: token t of sequence b goes to row p = clamp(cache_len[b]) + t,
    and a row at or beyond Smax is dropped. With `cos` / `sin` ([>= Smax, D])
    K is rotated by row p, its absolute position, exactly as rope_apply
    rotates it in a full forward, and the rotated q [B, T, H, D] is returned
    (a dropped token's q takes the table's last row); without them K is copied
    and None is returned. `cache_len` is not modified."""
    B, T, Hkv, D = k.shape
    Smax = k_cache.shape[2]
    base = cache_len.long().clamp(0, Smax)                      # [B]
    q_rot = None
    if cos is not None:
        pos = base[:, None] + torch.arange(T, device=k.device)  # [B, T]
        rows = pos.clamp(max=cos.shape[0] - 1)
        c = cos[rows].to(k.dtype)[:, :, None, :]
        s = sin[rows].to(k.dtype)[:, :, None, :]
        k = k * c + _rotate_half(k) * s
        q_rot = q * c + _rotate_half(q) * s
    if T == 0:
        return q_rot
    # gather form (row r of the cache takes token r - base when there is
    # one): deterministic, nothing indexes past either tensor
    t = torch.arange(Smax, device=k.device)[None, :] - base[:, None]
    take = ((t >= 0) & (t < T))[:, None, :, None]               # [B,1,Smax,1]
    idx = t.clamp(0, T - 1)[:, None, :, None].expand(B, Hkv, Smax, D)
    for cache, new in ((k_cache, k), (v_cache, v)):
        rows = new.permute(0, 2, 1, 3).gather(2, idx).to(cache.dtype)
        cache.copy_(torch.where(take, rows, cache))
    return q_rot


def decode_attention(q: torch.Tensor, k_cache: torch.Tensor,
                     v_cache: torch.Tensor, cache_len: torch.Tensor,
                     scale: Optional[float] = None,
                     window: Optional[int] = None) -> torch.Tensor:
    """Attention of one query token per sequence against the cache.

    q [B, H, D] is the query of the LAST cached token, position L - 1 with
    L = clamp(cache_len[b], 0, Smax); it attends keys [max(0, L - window), L)
    (`window` None or 0 = no window; the convention of causal_attention:
    j > L - 1 - window). Rows at or beyond L are never used, whatever they
    hold. L = 0 gives zeros. Math in the wider of q's dtype and fp32; returns
    [B, H, D] in q's dtype."""
    B, H, D = q.shape
    Hkv, Smax = k_cache.shape[1], k_cache.shape[2]
    wide = torch.promote_types(q.dtype, torch.float32)
    if scale is None:
        scale = 1.0 / math.sqrt(D)
    L = cache_len.long().clamp(0, Smax)[:, None]                # [B, 1]
    j = torch.arange(Smax, device=q.device)[None, :]
    allow = j < L
    if window:
        allow = allow & (j >= L - int(window))
    a4 = allow[:, None, :, None]
    zero = torch.zeros((), dtype=wide, device=q.device)
    k = torch.where(a4, k_cache.to(wide), zero)
    v = torch.where(a4, v_cache.to(wide), zero)
    if Hkv != H:
        k = k.repeat_interleave(H // Hkv, dim=1)
        v = v.repeat_interleave(H // Hkv, dim=1)
    s = torch.einsum("bhd,bhjd->bhj", q.to(wide), k) * scale
    s = s.masked_fill(~allow[:, None, :], float("-inf"))
    m = s.amax(-1, keepdim=True).clamp(min=torch.finfo(wide).min)
    p = torch.exp(s - m)                                        # masked: 0
    l = p.sum(-1, keepdim=True)
    o = torch.einsum("bhj,bhjd->bhd", p, v)
    return (o / l.clamp(min=torch.finfo(wide).tiny)).to(q.dtype)


# ------------------------------------------------- sampling (generation)
# The executable definition of ops.sample_logits (kernel: csrc/sample.hip).
# Integer parts (keys, thresholds, the generator) are exact; every real
# quantity is fp64.

SAMPLE_KEY_MIN = 0x0080          # key of the lowest finite bf16
_PHILOX_M0, _PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
_PHILOX_W0, _PHILOX_W1 = 0x9E3779B9, 0xBB67AE85


def philox4x32_10(ctr, key):
    """Philox4x32-10 (Salmon et al., SC'11): ctr = four and key = two uint32
    values or equal-shaped arrays of them; returns the four output words as
    numpy uint64 arrays holding uint32 values."""
    import numpy as np
    m32 = np.uint64(0xFFFFFFFF)
    c = [np.asarray(x, dtype=np.uint64) & m32 for x in ctr]
    k = [np.asarray(x, dtype=np.uint64) & m32 for x in key]
    s32 = np.uint64(32)
    for r in range(10):
        if r:
            k = [(k[0] + np.uint64(_PHILOX_W0)) & m32,
                 (k[1] + np.uint64(_PHILOX_W1)) & m32]
        p0 = np.uint64(_PHILOX_M0) * c[0]      # < 2^64: no wrap
        p1 = np.uint64(_PHILOX_M1) * c[2]
        c = [(p1 >> s32) ^ c[1] ^ k[0], p1 & m32,
             (p0 >> s32) ^ c[3] ^ k[1], p0 & m32]
    return c


def sample_uniform(idx, row: int, step: int, seed: int):
    """u_i = (r_i + 0.5) · 2^-23 in fp64 (exact in fp32 too, inside (0, 1)):
    r_i = top 23 bits of word 0 of Philox4x32-10 at counter
    (i, row, step_lo, step_hi) under key (seed_lo, seed_hi)."""
    import numpy as np
    seed, step = int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1)
    idx = np.asarray(idx, dtype=np.uint64)
    full = lambda v: np.full(idx.shape, v, dtype=np.uint64)   # noqa: E731
    w0 = philox4x32_10(
        (idx, full(row), full(step & 0xFFFFFFFF), full(step >> 32)),
        (full(seed & 0xFFFFFFFF), full(seed >> 32)))[0]
    r = (w0 >> np.uint64(9)).astype(np.float64)
    return (r + 0.5) * 2.0 ** -23


def sample_keys(bits):
    """Order-preserving uint16 keys of bf16 bit patterns (numpy uint16 in,
    int64 out): -0 -> +0, +-inf -> the largest finite bf16 of that sign, NaN
    -> key 0, below every value."""
    import numpy as np
    b = bits.astype(np.int64) & 0xFFFF
    mag = b & 0x7FFF
    b = np.where(mag == 0x7F80, (b & 0x8000) | 0x7F7F, b)
    b = np.where(mag == 0, 0, b)
    key = np.where(b & 0x8000, ~b & 0xFFFF, b | 0x8000)
    return np.where(mag > 0x7F80, 0, key)


def sample_key_bits(key):
    """The bf16 bit pattern of a key (inverse of sample_keys on values)."""
    import numpy as np
    key = np.asarray(key, dtype=np.int64)
    return np.where(key & 0x8000, key ^ 0x8000, ~key & 0xFFFF)


def _bf16_bits_to_f64(bits):
    import numpy as np
    return (np.asarray(bits, dtype=np.int64).astype(np.uint32)
            << np.uint32(16)).view(np.float32).astype(np.float64)


def sample_row(bits, row: int, temperature: float, top_k: int, top_p: float,
               seed: int, step: int) -> dict:
    """One row (numpy uint16 bf16 bit patterns [V]) of sample_logits, with
    what the tests' preconditions need next to the four outputs:
      p_margin  min over distinct values v of |mass(x >= v) / Z_k - top_p|
                (inf with top-p off)
      gap, gap_scale  best minus second-best perturbed score, and the larger
                |x/T| + |g| + 1 of the two (gap inf with one candidate)
      gap_pairwise  min over the other kept j of (score_best - score_j) /
                (scale_best + scale_j), scale = |x/T| + |g| + 1
      mean_abs_a  sum_i p_i · |x_i - max| / T over the top-k survivors
      a_tok, log_z  logprob = a_tok - log_z
    The temperature is taken as fp32 (the kernel's argument type)."""
    import numpy as np
    V = bits.shape[0]
    key = sample_keys(bits)
    valid = key > 0
    out = dict(token=0, logprob=0.0, thr_bits=int(
        sample_key_bits(SAMPLE_KEY_MIN)), n_kept=0, p_margin=math.inf,
        gap=math.inf, gap_scale=1.0, gap_pairwise=math.inf, mean_abs_a=0.0,
        a_tok=0.0, log_z=0.0)
    if not valid.any():
        return out
    x = _bf16_bits_to_f64(sample_key_bits(key))        # sanitised values
    greedy = float(temperature) == 0.0
    T = 1.0 if greedy else float(np.float32(temperature))
    kmax = key.max()
    a = (x - x[key == kmax][0]) / T                    # <= 0 where valid
    thr = SAMPLE_KEY_MIN
    if not greedy and 1 <= top_k < V:
        thr = max(thr, int(np.sort(key)[V - top_k]))   # k-th largest
    w = np.where(key >= thr, np.exp(np.where(valid, a, 0.0)), 0.0)
    z_k = w.sum()
    out["mean_abs_a"] = float((w * np.abs(np.where(valid, a, 0.0))).sum()
                              / z_k)
    if not greedy and top_p < 1.0:
        order = np.argsort(-key, kind="stable")
        ks, cw = key[order], np.cumsum(w[order])
        last = np.ones(V, dtype=bool)
        last[:-1] = ks[:-1] != ks[1:]                  # end of a tie group
        cand = last & (ks >= thr)
        frac = cw[cand] / z_k                          # mass(x >= v) / Z_k
        out["p_margin"] = float(np.abs(frac - top_p).min())
        hit = np.nonzero(frac >= top_p)[0]
        # the first group that reaches top_p; rounding may leave none
        thr_p = int(ks[cand][hit[0]]) if hit.size else thr
        thr = max(thr, thr_p)
    kept = key >= thr
    idx = np.nonzero(kept)[0]
    if greedy:
        score = x[idx]
        g = np.zeros(idx.shape)
    else:
        u = sample_uniform(idx, row, step, seed)
        g = -np.log(-np.log(u))
        score = x[idx] / T + g
    j = int(np.argmax(score))                          # lowest index on ties
    tok = int(idx[j])
    if idx.size > 1:
        rest = np.delete(score, j)
        j2 = int(np.argmax(rest))
        j2 += j2 >= j
        out["gap"] = float(score[j] - score[j2])
        scale = np.abs(x[idx] / T) + np.abs(g) + 1.0
        out["gap_scale"] = float(max(scale[j], scale[j2]))
        pair = (score[j] - score) / (scale[j] + scale)
        pair[j] = np.inf
        out["gap_pairwise"] = float(pair.min())
    z = w[kept].sum()
    out.update(token=tok, a_tok=float(a[tok]), log_z=float(np.log(z)),
               logprob=float(a[tok] - np.log(z)),
               thr_bits=int(sample_key_bits(thr)), n_kept=int(idx.size))
    return out


def sample_logits(logits: torch.Tensor, *, temperature: float, top_k: int = 0,
                  top_p: float = 1.0, seed: int, step: int,
                  done: Optional[torch.Tensor] = None, eos_id: int = -1,
                  details: Optional[list] = None):
    """(token int64 [B], logprob fp32 [B], thr bf16 [B], n_kept int32 [B]) of
    one draw per row of logits [B, V], taken as bf16 (another dtype is
    rounded to it first: thresholds are keys of the bf16 value).

    temperature > 0: top-k (0 = off; x >= the k-th largest value, ties kept),
    then top-p (>= 1 = off) on softmax(x / T) renormalised over the top-k
    survivors (the largest value whose upper mass reaches top_p; ties kept,
    at least one token), then Gumbel-max token = argmax_i x_i / T + g_i over
    the kept i, lowest index on ties, g_i from sample_uniform(i, b, step,
    seed). temperature == 0: the argmax, filters ignored. logprob: log of the
    token's probability in the filtered, temperature-scaled distribution
    (greedy: the unfiltered T = 1 softmax). A row without a finite logit
    gives token 0, logprob 0, n_kept 0.

    done (uint8 [B], updated in place) with 0 <= eos_id < V: a set flag makes
    the row's token eos_id, nothing is drawn (logprob 0, thr 0, n_kept 0);
    otherwise done[b] |= token == eos_id. `details`, a list, receives
    sample_row's dict of every row that was drawn."""
    import numpy as np
    if logits.dim() != 2 or logits.shape[1] < 1:
        raise ValueError(f"logits must be [B, V >= 1], got {logits.shape}")
    if not (0.0 <= float(temperature) < 1e30):
        raise ValueError(f"temperature must be >= 0, got {temperature}")
    if int(top_k) < 0 or not float(top_p) > 0.0:
        raise ValueError(f"need top_k >= 0 and top_p > 0, got {top_k}, "
                         f"{top_p}")
    B, V = logits.shape
    if done is not None and not 0 <= int(eos_id) < V:
        raise ValueError(f"with done, eos_id must be in [0, {V}), got "
                         f"{eos_id}")
    dev = logits.device
    bits = logits.detach().to(device="cpu", dtype=torch.bfloat16) \
        .contiguous().view(torch.int16).numpy().view(np.uint16)
    done_np = None
    if done is not None:
        done_np = done.detach().to("cpu").numpy()      # shared when on CPU
    token = np.zeros(B, dtype=np.int64)
    logprob = np.zeros(B, dtype=np.float32)
    thr = np.zeros(B, dtype=np.int16)
    n_kept = np.zeros(B, dtype=np.int32)
    for b in range(B):
        if done_np is not None and done_np[b]:
            token[b] = int(eos_id)
            continue
        r = sample_row(bits[b], b, float(temperature), int(top_k),
                       float(top_p), seed, step)
        if details is not None:
            details.append(r)
        token[b], logprob[b], n_kept[b] = r["token"], r["logprob"], \
            r["n_kept"]
        thr[b] = np.uint16(r["thr_bits"]).view(np.int16)
        if done_np is not None:
            done_np[b] = r["token"] == int(eos_id)
    if done is not None and done.device.type != "cpu":
        done.copy_(torch.from_numpy(done_np))
    return (torch.from_numpy(token).to(dev),
            torch.from_numpy(logprob).to(dev),
            torch.from_numpy(thr).view(torch.bfloat16).to(dev),
            torch.from_numpy(n_kept).to(dev))


def causal_lm_loss(logits: torch.Tensor, labels: torch.Tensor,
                   ignore_index: int = -100) -> torch.Tensor:
    """Shifted causal-LM cross entropy (HF CausalLM loss inside K1/K9)."""
    shift_logits = logits[..., :-1, :].contiguous().float()
    shift_labels = labels[..., 1:].contiguous()
    return F.cross_entropy(shift_logits.view(-1, shift_logits.size(-1)),
                           shift_labels.view(-1), ignore_index=ignore_index)


def label_smoothed_causal_lm_loss(logits: torch.Tensor, labels: torch.Tensor,
                                  epsilon: float,
                                  ignore_index: int = -100) -> torch.Tensor:
    """HF LabelSmoother-equivalent shifted loss
    (reference utils/trainer_utils.py:862-902, used when
    label_smoothing_factor != 0 — trainer_base.py:63-68):
    (1-eps)·NLL + eps·(mean over vocab of -log p), masked mean."""
    shift_logits = logits[..., :-1, :].contiguous().float()
    shift_labels = labels[..., 1:].contiguous()
    logp = F.log_softmax(shift_logits, dim=-1)
    mask = shift_labels.eq(ignore_index)
    safe = shift_labels.clamp(min=0).unsqueeze(-1)
    nll = -logp.gather(-1, safe).squeeze(-1).masked_fill(mask, 0.0)
    smooth = -logp.sum(-1).masked_fill(mask, 0.0)
    n = (~mask).sum().clamp(min=1)
    nll = nll.sum() / n
    smooth = smooth.sum() / (n * shift_logits.size(-1))
    return (1.0 - epsilon) * nll + epsilon * smooth


# ------------------------------------------- chunked lm_head + shifted CE
# The [B, S, V] logits are never materialised: a chunk of `chunk_tokens` rows
# is projected into one reused [C, V] buffer, reduced to per-row lse and loss,
# and dropped; the backward recomputes the chunk, turns the buffer into
# dlogits in place and feeds the dh and dW GEMMs from it. The chunk loop below
# is shared by the torch-math path (here) and the HIP path (ops/autograd.py),
# which differ in the row kernels only.

def shifted_targets(labels: torch.Tensor, V: int):
    """(targets int64 [B·S], n_valid 0-dim int64): targets[b·S + s] =
    labels[b, s + 1], -100 at each row's last position; a target is valid iff
    0 <= target < V. Plain torch ops on the labels' device, no host sync."""
    labels = labels.long()
    targets = torch.full_like(labels, -100)
    targets[..., :-1] = labels[..., 1:]
    targets = targets.reshape(-1)
    n_valid = ((targets >= 0) & (targets < V)).sum()
    return targets, n_valid


class TorchRows:
    """Row kernels of the chunked loss in torch math, in the wider of the
    logits' dtype and fp32."""

    @staticmethod
    def stat_dtype(dtype: torch.dtype) -> torch.dtype:
        return torch.promote_types(dtype, torch.float32)

    @staticmethod
    def fwd(lg, tg, lse, tok, eps):
        V = lg.shape[1]
        x = lg.to(lse.dtype)
        valid = (tg >= 0) & (tg < V)
        l = torch.logsumexp(x, dim=-1)
        t = l - x.gather(1, tg.clamp(0, V - 1)[:, None]).squeeze(1)
        if eps != 0.0:
            t = (1.0 - eps) * t + eps * (l - x.sum(-1) / V)
        zero = torch.zeros_like(l)
        lse.copy_(torch.where(valid, l, zero))
        tok.copy_(torch.where(valid, t, zero))

    @staticmethod
    def bwd_(lg, tg, lse, scale, eps):
        V = lg.shape[1]
        x = lg.to(lse.dtype)
        valid = (tg >= 0) & (tg < V)
        p = torch.exp(x - lse[:, None]) - eps / V
        p.scatter_add_(1, tg.clamp(0, V - 1)[:, None],
                       torch.full_like(p[:, :1], -(1.0 - eps)))
        lg.copy_(torch.where(valid[:, None], p * scale, torch.zeros_like(p)))

    @staticmethod
    def total(tok):
        return tok.double().sum().to(tok.dtype).reshape(1)


def chunked_lm_loss_forward(ctx, rows, hidden2, weight, targets, n_valid,
                            epsilon, chunk_tokens, grad_view):
    """hidden2 [T, H], weight [V, H], targets [T] (already shifted). Saves
    hidden, weight, targets, lse and the denominator; never the logits."""
    T, V = hidden2.shape[0], weight.shape[0]
    C = max(1, min(int(chunk_tokens), T))
    sdt = rows.stat_dtype(hidden2.dtype)
    buf = hidden2.new_empty((C, V))
    lse = torch.empty(T, dtype=sdt, device=hidden2.device)
    tok = torch.empty_like(lse)
    for s in range(0, T, C):
        e = min(s + C, T)
        lg = buf[:e - s]
        torch.mm(hidden2[s:e], weight.t(), out=lg)
        rows.fwd(lg, targets[s:e], lse[s:e], tok[s:e], epsilon)
    denom = n_valid.clamp(min=1).to(sdt)
    ctx.save_for_backward(hidden2, weight, targets, lse, denom)
    ctx.meta = (rows, float(epsilon), C, grad_view)
    # one fixed-order sum over all rows: bitwise reproducible
    return (rows.total(tok) / denom).reshape(())


def chunked_lm_loss_backward(ctx, grad_out):
    """(dh, dW): dW is None when it went into the grad-arena view. The
    upstream gradient is applied here (the trainer divides the loss), as a
    device scalar: no host read."""
    from acco_amd.models import fuse
    hidden2, weight, targets, lse, denom = ctx.saved_tensors
    rows, eps, C, g_view = ctx.meta
    T, V = hidden2.shape[0], weight.shape[0]
    scale = grad_out.to(lse.dtype).reshape(1) / denom
    buf = hidden2.new_empty((C, V))
    dh = torch.empty_like(hidden2)
    dw = None
    if g_view is None and ctx.needs_input_grad[1]:
        dw = torch.zeros(weight.shape, device=weight.device,
                         dtype=torch.promote_types(weight.dtype,
                                                   torch.float32))
    for s in range(0, T, C):
        e = min(s + C, T)
        lg, h = buf[:e - s], hidden2[s:e]
        torch.mm(h, weight.t(), out=lg)
        rows.bwd_(lg, targets[s:e], lse[s:e], scale, eps)
        torch.mm(lg, weight, out=dh[s:e])
        if g_view is not None:
            fuse._add_wgrad(g_view, lg.t(), h)
        elif dw is not None and lg.is_cuda and lg.dtype != dw.dtype:
            # fp32 out of the bf16 GEMM: no wide copy of the chunk
            dw.add_(torch.mm(lg.t(), h, out_dtype=dw.dtype))
        elif dw is not None:
            dw.addmm_(lg.t().to(dw.dtype), h.to(dw.dtype))
    if g_view is not None:
        # once, after the last chunk: the DDP tracker counts covered elements
        # per notification
        fuse._notify(g_view)
    return dh, (dw.to(weight.dtype) if dw is not None else None)


class LinearCausalLMLossRefFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, hidden2, weight, targets, n_valid, epsilon, chunk_tokens,
                grad_view):
        return chunked_lm_loss_forward(ctx, TorchRows, hidden2, weight,
                                       targets, n_valid, epsilon,
                                       chunk_tokens, grad_view)

    @staticmethod
    def backward(ctx, grad_out):
        dh, dw = chunked_lm_loss_backward(ctx, grad_out)
        return dh, dw, None, None, None, None, None


def linear_causal_lm_loss(hidden: torch.Tensor, weight: torch.Tensor,
                          labels: torch.Tensor, epsilon: float = 0.0,
                          chunk_tokens: int = 4096,
                          grad_view: Optional[torch.Tensor] = None
                          ) -> torch.Tensor:
    """Mean shifted causal-LM loss of `hidden @ weight^T` over the valid
    tokens (label smoothing as label_smoothed_causal_lm_loss), `chunk_tokens`
    rows of logits at a time. hidden [B, S, H], weight [V, H], labels [B, S].
    With `grad_view` the weight gradient is accumulated into it in place and
    none is returned."""
    if int(chunk_tokens) < 1:
        raise ValueError(f"chunk_tokens must be >= 1, got {chunk_tokens}")
    targets, n_valid = shifted_targets(labels, weight.shape[0])
    return LinearCausalLMLossRefFn.apply(
        hidden.reshape(-1, hidden.shape[-1]), weight, targets, n_valid,
        float(epsilon), int(chunk_tokens), grad_view)


@torch.no_grad()
def grad_sumsq(g: torch.Tensor, partials: torch.Tensor) -> int:
    """Sum of squares of a gradient segment as fp32 partial sums: the
    reference writes one partial, slot 0, and returns the partial count."""
    partials.view(-1)[0] = g.float().square().sum()
    return 1


@torch.no_grad()
def sumsq_finalize(partials: torch.Tensor, out: torch.Tensor) -> None:
    """out[0] = sum of the partials, accumulated in double."""
    out.view(-1).copy_(partials.double().sum().float().reshape(1))


@torch.no_grad()
def clip_grad_scale(sumsq: torch.Tensor, grad_scale, max_norm: float,
                    eps: float = 1e-6):
    """Global-norm clipping folded into the gradient scale, the formula of
    torch.nn.utils.clip_grad_norm_ on the gradient `grad_scale · g`:

        norm  = sqrt(sumsq) · grad_scale
        coef  = clamp(max_norm / (norm + eps), max=1)
        scale = grad_scale · coef

    sumsq: 1-element fp32 tensor holding sum(g²) of the unscaled gradient;
    grad_scale: float or 1-element tensor (the engine's 1/count). Returns
    1-element fp32 (scale, norm, coef) on sumsq's device; no host sync. A
    non-finite norm propagates exactly as it does in torch."""
    norm = (sumsq.float().sqrt() * grad_scale).float().reshape(1)
    coef = torch.clamp(max_norm / (norm + eps), max=1.0)
    scale = (coef * grad_scale).float().reshape(1)
    return scale, norm, coef


@torch.no_grad()
def fused_adamw_step(p: torch.Tensor, g: torch.Tensor, m: torch.Tensor,
                     v: torch.Tensor, step: int, lr: float, beta1: float,
                     beta2: float, eps: float, weight_decay: float,
                     grad_scale: float = 1.0,
                     out_bf16: Optional[torch.Tensor] = None,
                     commit: bool = True) -> None:
    """Sharded AdamW step, torch.optim.AdamW-equivalent math (K3+K5 fused,
    reference trainer_decoupled.py:95-100).

    p, m, v fp32; g any float dtype (cast + scaled by `grad_scale` = 1/count,
    reference :98). If `commit` is False this is the ACCO *tentative* step
    (even com rounds, reference :79-84,113-125): the updated parameters are
    written to `out_bf16` but p/m/v/step are left untouched — equivalent to
    the reference's snapshot→step→rollback without the three state clones.
    """
    gf = g.float() * grad_scale
    t = step + 1
    bc1 = 1.0 - beta1 ** t
    bc2 = 1.0 - beta2 ** t
    if commit:
        p.mul_(1.0 - lr * weight_decay)
        m.mul_(beta1).add_(gf, alpha=1.0 - beta1)
        v.mul_(beta2).addcmul_(gf, gf, value=1.0 - beta2)
        denom = (v.sqrt() / math.sqrt(bc2)).add_(eps)
        p.addcdiv_(m, denom, value=-lr / bc1)
        if out_bf16 is not None:
            out_bf16.copy_(p)
    else:
        p_t = p * (1.0 - lr * weight_decay)
        m_t = m * beta1 + gf * (1.0 - beta1)
        v_t = v * beta2 + gf * gf * (1.0 - beta2)
        denom = (v_t.sqrt() / math.sqrt(bc2)).add_(eps)
        p_t.addcdiv_(m_t, denom, value=-lr / bc1)
        assert out_bf16 is not None, "tentative step must write out_bf16"
        out_bf16.copy_(p_t)
