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

#
# FP8 cache: k / v hold OCP e4m3 codes (torch.float8_e4m3fn: max 448, no inf)
# and k_scale / v_scale [B, Hkv, Smax] fp32 hold one scale per cache row; a
# row's value is float(code) * scale. kv_quantize / kv_dequantize are the
# executable definition of the format; the HIP kernels match kv_quantize bit
# for bit on IEEE fp32 arithmetic (the CPU).

E4M3_MAX = 448.0


def kv_quantize(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(codes e4m3 [..., D], scale fp32 [...]) of rows x [..., D]. Every step
    is one rounded fp32 operation: amax = max |x|, scale = amax / 448, inv =
    448 / amax (0 for a zero row), y = clamp(x * inv, -448, 448), code =
    round-to-nearest-even e4m3(y), subnormals kept. The row maximum maps to
    +-448 exactly; a zero row gives scale 0 and zero codes."""
    xf = x.float()
    amax = xf.abs().amax(-1)
    top = torch.full_like(amax, E4M3_MAX)
    scale = amax / top
    # a true division, not Tensor.__rtruediv__'s reciprocal-and-multiply
    inv = torch.where(amax > 0, top / amax, torch.zeros_like(amax))
    y = (xf * inv[..., None]).clamp(-E4M3_MAX, E4M3_MAX)
    return y.to(torch.float8_e4m3fn), scale


def kv_dequantize(codes: torch.Tensor, scale: torch.Tensor,
                  dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """float(code) * scale per row, computed and returned in `dtype`."""
    return codes.to(dtype) * scale.to(dtype)[..., None]


def weight_quantize(w: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(codes e4m3 [N, K], scale fp32 [N]) of a linear's weight [N, K]: the
    format of the e4m3 KV cache applied to the rows of `w` (kv_quantize), one
    scale per output row. The scale of a row is a factor of its whole dot
    product, so it multiplies the finished sum and never enters the K loop."""
    return kv_quantize(w)


def linear_w8(x: torch.Tensor, codes: torch.Tensor, scale: torch.Tensor,
              bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y [..., N] = (x [..., K] @ float(codes [N, K])^T) * scale [N] (+ bias
    [N]) for weights stored by weight_quantize, computed in fp32 (fp64 for an
    fp64 x) and returned in x's dtype."""
    acc = torch.promote_types(x.dtype, torch.float32)
    y = (x.to(acc) @ codes.to(acc).t()) * scale.to(acc)
    if bias is not None:
        y = y + bias.to(acc)
    return y.to(x.dtype)


_E2M1 = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)     # magnitude of code & 7


def weight_quantize_mxfp4(w: torch.Tensor
                          ) -> Tuple[torch.Tensor, torch.Tensor]:
    """(codes uint8 [N, K / 2], scales uint8 [N, K / 32]) of a linear's weight
    [N, K] in OCP MXFP4; K must be a multiple of 32. A code is a nibble: sign,
    two exponent bits, one mantissa bit, magnitudes 0, 0.5, 1, 1.5, 2, 3, 4,
    6; byte i of a row holds k = 2 i in its low nibble and k = 2 i + 1 in its
    high nibble (the packing of torch.float4_e2m1fn_x2, stored as plain
    uint8). Every 32 consecutive k share one e8m0 scale byte s, the scale
    2^(s - 127).

    The exponent is the OCP MX rule in exact operations: with amax the
    block's largest |w| in fp32, e = floor(log2(amax)) - 2 (torch.frexp),
    clamped into [-120, 120] so that every dequantised value is a normal bf16
    and s << 23 is the scale as fp32 bits; s = e + 127. A zero block takes
    byte 127 and zero codes; byte 255 (NaN) is never produced. A code is
    w / 2^e rounded to the nearest magnitude, ties to the even code,
    saturating at +-6: amax / 2^e lies in [4, 8), so values in (6, 8) * 2^e
    clip to 6 * 2^e. That is the specification's behaviour, not an
    oversight."""
    N, K = w.shape
    if K % 32 != 0:
        raise ValueError(f"weight_quantize_mxfp4 needs K % 32 == 0, got {K}")
    blocks = w.detach().float().reshape(N, K // 32, 32)
    amax = blocks.abs().amax(dim=-1)
    e = torch.frexp(amax)[1] - 3      # amax = m * 2^exp, m in [0.5, 1)
    e = torch.where(amax > 0, e.clamp(-120, 120), torch.zeros_like(e))
    v = torch.ldexp(blocks.double(), -e[..., None]).abs()    # exact
    grid = torch.tensor(_E2M1, dtype=torch.float64, device=w.device)
    hi = torch.bucketize(v, grid).clamp(max=7)      # first magnitude >= v
    lo = (hi - 1).clamp(min=0)
    d_lo, d_hi = v - grid[lo], grid[hi] - v
    code = torch.where((d_lo < d_hi) | ((d_lo == d_hi) & (lo % 2 == 0)),
                       lo, hi)
    code = (code + 8 * (blocks < 0)).to(torch.uint8)
    code = code.reshape(N, K // 2, 2)
    return code[..., 0] | (code[..., 1] << 4), (e + 127).to(torch.uint8)


def weight_dequantize_mxfp4(codes: torch.Tensor, scales: torch.Tensor,
                            dtype: torch.dtype) -> torch.Tensor:
    """The [N, K] values of MXFP4 codes [N, K / 2] and scales [N, K / 32] in
    `dtype`: exact in bf16 and anything wider (a two-bit significand times a
    power of two), for the scale bytes weight_quantize_mxfp4 produces."""
    N = codes.shape[0]
    nib = torch.stack((codes & 15, codes >> 4), dim=-1).reshape(N, -1, 32)
    lut = torch.tensor(_E2M1 + tuple(-m for m in _E2M1), dtype=dtype,
                       device=codes.device)
    scale = torch.ldexp(torch.ones((), device=codes.device),
                        scales.int() - 127).to(dtype)
    return (lut[nib.int()] * scale[..., None]).reshape(N, -1)


def linear_w4(x: torch.Tensor, codes: torch.Tensor, scales: torch.Tensor,
              bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y [..., N] = x [..., K] @ dequant(codes, scales)^T (+ bias [N]) for
    weights stored by weight_quantize_mxfp4, computed in fp32 (fp64 for an
    fp64 x) and returned in x's dtype."""
    acc = torch.promote_types(x.dtype, torch.float32)
    y = x.to(acc) @ weight_dequantize_mxfp4(codes, scales, acc).t()
    if bias is not None:
        y = y + bias.to(acc)
    return y.to(x.dtype)


def act_quantize_mxfp8(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(codes float8_e4m3fn [..., K], scales uint8 [..., K / 32]) of
    activation rows x [..., K] in OCP MXFP8; K must be a multiple of 32. Every
    32 consecutive k share one e8m0 scale byte s, the scale 2^(s - 127).

    The exponent is weight_quantize_mxfp4's rule with e4m3's largest exponent
    in place of e2m1's, in exact operations: with amax the block's largest
    |x| in fp32, e = floor(log2(amax)) - 8 (torch.frexp), clamped into
    [-120, 120]; s = e + 127. A zero block takes byte 127 and zero codes; byte
    255 (NaN) is never produced. A code is x / 2^e (exact) rounded to the
    nearest e4m3, ties to even, subnormals kept, saturating at +-448 (the
    clamp is applied in the wide type: torch's e4m3 cast does not saturate):
    amax / 2^e lies in [256, 512), so values in (448, 512) * 2^e clip to
    448 * 2^e. That is the specification's behaviour, not an oversight.
    Non-finite x is outside the contract."""
    K = x.shape[-1]
    if K % 32 != 0:
        raise ValueError(f"act_quantize_mxfp8 needs K % 32 == 0, got {K}")
    blocks = x.detach().float().reshape(*x.shape[:-1], K // 32, 32)
    amax = blocks.abs().amax(dim=-1)
    e = torch.frexp(amax)[1] - 9      # amax = m * 2^exp, m in [0.5, 1)
    e = torch.where(amax > 0, e.clamp(-120, 120), torch.zeros_like(e))
    v = torch.ldexp(blocks.double(), -e[..., None])          # exact
    codes = v.clamp(-E4M3_MAX, E4M3_MAX).float().to(torch.float8_e4m3fn)
    return codes.reshape(x.shape), (e + 127).to(torch.uint8)


def act_dequantize_mxfp8(codes: torch.Tensor, scales: torch.Tensor,
                         dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """The [..., K] values of MXFP8 codes [..., K] and scales [..., K / 32] in
    `dtype`: exact in fp32 and wider (a four-bit significand times a power of
    two), and in bf16 where the value is a normal bf16."""
    K = codes.shape[-1]
    scale = torch.ldexp(torch.ones((), device=codes.device),
                        scales.int() - 127).to(dtype)
    blocks = codes.to(dtype).reshape(*codes.shape[:-1], K // 32, 32)
    return (blocks * scale[..., None]).reshape(codes.shape)


def linear_w4a8(x: torch.Tensor, codes: torch.Tensor, scales: torch.Tensor,
                bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y [..., N] = dequant(act_quantize_mxfp8(x)) @ dequant(codes, scales)^T
    (+ bias [N]) for weights stored by weight_quantize_mxfp4: linear_w4 with
    x rounded to MXFP8 first. Computed in fp32 (fp64 for an fp64 x) and
    returned in x's dtype. Non-finite x is outside the contract."""
    acc = torch.promote_types(x.dtype, torch.float32)
    xq = act_dequantize_mxfp8(*act_quantize_mxfp8(x), acc)
    y = xq @ weight_dequantize_mxfp4(codes, scales, acc).t()
    if bias is not None:
        y = y + bias.to(acc)
    return y.to(x.dtype)


@torch.no_grad()
def kv_append(k_cache: torch.Tensor, v_cache: torch.Tensor,
              cache_len: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
              q: Optional[torch.Tensor] = None,
              cos: Optional[torch.Tensor] = None,
              sin: Optional[torch.Tensor] = None,
              k_scale: Optional[torch.Tensor] = None,
              v_scale: Optional[torch.Tensor] = None
              ) -> Optional[torch.Tensor]:
    """Write k, v [B, T, Hkv, D] of T new tokens per sequence into the caches,
    in place: token t of sequence b goes to row p = clamp(cache_len[b]) + t,
    and a row at or beyond Smax is dropped. With `cos` / `sin` ([>= Smax, D])
    K is rotated by row p, its absolute position, exactly as rope_apply
    rotates it in a full forward, and the rotated q [B, T, H, D] is returned
    (a dropped token's q takes the table's last row); without them K is copied
    and None is returned. `cache_len` is not modified. With `k_scale` /
    `v_scale` the caches are e4m3: each new row (K after the rotation, in k's
    dtype) goes through kv_quantize, its codes to the cache and its scale to
    the same row of the scale tensor."""
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
    for cache, new, sc in ((k_cache, k, k_scale), (v_cache, v, v_scale)):
        rows = new.permute(0, 2, 1, 3).gather(2, idx)
        if sc is None:
            cache.copy_(torch.where(take, rows.to(cache.dtype), cache))
            continue
        codes, scale = kv_quantize(rows)
        # select on the bytes: torch.where has no float8 kernel everywhere
        cache.view(torch.uint8).copy_(torch.where(
            take, codes.view(torch.uint8), cache.view(torch.uint8)))
        sc.copy_(torch.where(take[..., 0], scale, sc))
    return q_rot


def _wide_cache(cache: torch.Tensor, row_scale: Optional[torch.Tensor],
                wide: torch.dtype) -> torch.Tensor:
    """The cache in the math dtype: dequantised when it has row scales."""
    if row_scale is None:
        return cache.to(wide)
    return kv_dequantize(cache, row_scale, wide)


def decode_attention(q: torch.Tensor, k_cache: torch.Tensor,
                     v_cache: torch.Tensor, cache_len: torch.Tensor,
                     scale: Optional[float] = None,
                     window: Optional[int] = None,
                     k_scale: Optional[torch.Tensor] = None,
                     v_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Attention of one query token per sequence against the cache.

    q [B, H, D] is the query of the LAST cached token, position L - 1 with
    L = clamp(cache_len[b], 0, Smax); it attends keys [max(0, L - window), L)
    (`window` None or 0 = no window; the convention of causal_attention:
    j > L - 1 - window). Rows at or beyond L are never used, whatever they
    hold. L = 0 gives zeros. Math in the wider of q's dtype and fp32; returns
    [B, H, D] in q's dtype. With `k_scale` / `v_scale` the caches are e4m3
    and are dequantised first (kv_dequantize), then the same math."""
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
    k = torch.where(a4, _wide_cache(k_cache, k_scale, wide), zero)
    v = torch.where(a4, _wide_cache(v_cache, v_scale, wide), zero)
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


def extend_attention(q: torch.Tensor, k_cache: torch.Tensor,
                     v_cache: torch.Tensor, cache_len: torch.Tensor,
                     scale: Optional[float] = None,
                     window: Optional[int] = None,
                     k_scale: Optional[torch.Tensor] = None,
                     v_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Attention of T new query tokens per sequence against the cache, which
    already holds their K / V (kv_append with the same `cache_len`).

    q [B, T, H, D]; `cache_len` is the length BEFORE the T tokens. With
    L0 = clamp(cache_len[b], 0, Smax), query t sits at p = L0 + t and attends
    keys max(0, p + 1 - window) <= j <= p (`window` None or 0 = no window,
    the convention of decode_attention and causal_attention). A query with
    p >= Smax (its token was dropped by the append) gives +0. Rows above the
    keys a query attends are never used, whatever they hold. Math in the
    wider of q's dtype and fp32; returns [B, T, H, D] in q's dtype. T = 1 is
    decode_attention(q[:, 0], ..., cache_len + 1). `k_scale` / `v_scale`: an
    e4m3 cache, as in decode_attention."""
    B, T, H, D = q.shape
    Hkv, Smax = k_cache.shape[1], k_cache.shape[2]
    wide = torch.promote_types(q.dtype, torch.float32)
    if scale is None:
        scale = 1.0 / math.sqrt(D)
    L0 = cache_len.long().clamp(0, Smax)
    p = L0[:, None] + torch.arange(T, device=q.device)[None, :]   # [B, T]
    j = torch.arange(Smax, device=q.device)
    allow = (j[None, None, :] <= p[:, :, None]) & (p < Smax)[:, :, None]
    if window:                                                    # [B, T, Smax]
        allow = allow & (j[None, None, :] > p[:, :, None] - int(window))
    # a row no query of the sequence attends is replaced before any arithmetic
    used = allow.any(1)[:, None, :, None]                         # [B,1,Smax,1]
    zero = torch.zeros((), dtype=wide, device=q.device)
    k = torch.where(used, _wide_cache(k_cache, k_scale, wide), zero)
    v = torch.where(used, _wide_cache(v_cache, v_scale, wide), zero)
    if Hkv != H:
        k = k.repeat_interleave(H // Hkv, dim=1)
        v = v.repeat_interleave(H // Hkv, dim=1)
    a4 = allow[:, None]                                           # [B,1,T,Smax]
    s = torch.einsum("bthd,bhjd->bhtj", q.to(wide), k) * scale
    s = s.masked_fill(~a4, float("-inf"))
    m = s.amax(-1, keepdim=True).clamp(min=torch.finfo(wide).min)
    pr = torch.exp(s - m)                                         # masked: 0
    l = pr.sum(-1, keepdim=True)
    o = torch.einsum("bhtj,bhjd->bhtd", pr, v)
    o = o / l.clamp(min=torch.finfo(wide).tiny)
    return o.permute(0, 2, 1, 3).to(q.dtype)


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


# ------------------------------------- draft verification (speculative decoding)
# The executable definition of ops.spec_verify (kernel: csrc/spec_verify.hip).

SPEC_ROW_TAG = 0x80000000        # Philox word 1: no sampler row has bit 31
SPEC_ACCEPT_WORD = 0xFFFFFFFF    # Philox word 0 of u_t: no index reaches it


def _spec_uniform(word0, word1, step: int, seed: int):
    """sample_uniform at the Philox counter (word0, word1, step_lo, step_hi),
    word0 and word1 broadcast against each other."""
    import numpy as np
    seed, step = int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1)
    w0, w1 = np.broadcast_arrays(np.asarray(word0, dtype=np.uint64),
                                 np.asarray(word1, dtype=np.uint64))
    full = lambda v: np.full(w0.shape, v, dtype=np.uint64)   # noqa: E731
    out = philox4x32_10((w0, w1, full(step & 0xFFFFFFFF), full(step >> 32)),
                        (full(seed & 0xFFFFFFFF), full(seed >> 32)))[0]
    return ((out >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def _spec_softmax(key, T: float):
    """(probabilities, (x - max) / T, sanitised x) of rows of keys [B, V] in
    fp64; NaN (key 0) has mass 0, a row without a finite logit is all 0."""
    import numpy as np
    valid = key > 0
    x = _bf16_bits_to_f64(sample_key_bits(key))
    xmax = np.where(valid, x, -np.inf).max(axis=1, keepdims=True)
    a = np.where(valid, (x - np.where(np.isfinite(xmax), xmax, 0.0)) / T, 0.0)
    w = np.where(valid, np.exp(a), 0.0)
    z = w.sum(axis=1, keepdims=True)
    return w / np.where(z > 0, z, 1.0), a, x


def spec_verify(p_logits: torch.Tensor, q_logits: torch.Tensor,
                draft_tokens: torch.Tensor, *, temperature: float, seed: int,
                step: int, done: Optional[torch.Tensor] = None,
                eos_id: int = -1, details: Optional[list] = None):
    """(n_accept int32 [B], next_token int64 [B], accept_prob fp32 [B, k]):
    the accept / reject / resample step of speculative decoding over target
    logits p_logits [B, k+1, V], draft logits q_logits [B, k, V] and the
    drafted tokens x [B, k]. Logits are taken as bf16 and sanitised as the
    sampler's (sample_keys: -0 -> +0, +-inf clamped, NaN has mass 0).

    temperature > 0, p_t = softmax(p_logits[b, t] / T), q_t likewise (a row
    without a finite logit is all 0): x_t is accepted iff
    u_t · q_t(x_t) < p_t(x_t) (no division: q_t(x_t) = 0 is defined; a token
    outside [0, V) has p = q = 0 and rejects); accept_prob[b, t] =
    min(1, p_t(x_t) / q_t(x_t)), 0 when both are 0. n_accept = accepted tokens
    before the first rejection. n_accept = t < k: next_token = argmax over i
    with p_t(i) > q_t(i) of log(p_t(i) - q_t(i)) + g_i, lowest index on ties
    (a Gumbel-max draw from the residual); an empty residual draws from p_t
    as below. n_accept = k: next_token = argmax_i x_i / T + g_i over the
    non-NaN i of p_k, the sampler's draw (0 without a finite logit).
    temperature == 0: x_t is accepted iff it is the lowest-index argmax of
    p row t, next_token is that argmax of row n_accept, accept_prob is 0 or
    1, nothing is drawn.

    Generator: Philox4x32-10 under key (seed_lo, seed_hi) at counter
    (w0, 2^31 | (b (k + 1) + t), step_lo, step_hi): w0 = i for g_i of row
    (b, t), w0 = 2^32 - 1 for u_t; both map the word as sample_uniform does,
    g = -log(-log(u)). sample_logits uses (i, row, step_lo, step_hi) with
    i, row < 2^31, so no call of it shares a counter with this one, whatever
    the (seed, step). Needs B (k + 1) < 2^31. Every output is a pure function
    of the arguments.

    done (uint8 [B], updated in place) with 0 <= eos_id < V: a set flag gives
    n_accept 0, next_token eos_id and accept_prob 0, nothing drawn; otherwise
    done[b] |= next_token == eos_id. `details`, a list, receives per row t a
    dict of the fp64 arrays the tests' preconditions need (p, q, a_p, a_q, g,
    u, px, qx, the sanitised x, T, and cand, the row's candidate token)."""
    import numpy as np
    if p_logits.dim() != 3 or q_logits.dim() != 3 \
            or p_logits.shape[1] < 2 or p_logits.shape[2] < 1 \
            or tuple(q_logits.shape) != (p_logits.shape[0],
                                         p_logits.shape[1] - 1,
                                         p_logits.shape[2]):
        raise ValueError("need p_logits [B, k+1, V] and q_logits [B, k, V] "
                         f"with k, V >= 1, got {tuple(p_logits.shape)} and "
                         f"{tuple(q_logits.shape)}")
    B, k1, V = p_logits.shape
    k = k1 - 1
    if tuple(draft_tokens.shape) != (B, k):
        raise ValueError(f"draft_tokens must be [B, k] = [{B}, {k}], got "
                         f"{tuple(draft_tokens.shape)}")
    if not (0.0 <= float(temperature) < 1e30):
        raise ValueError(f"temperature must be >= 0, got {temperature}")
    if B * k1 >= 2 ** 31:
        raise ValueError(f"B (k + 1) must be below 2^31, got {B * k1}")
    if done is not None and not 0 <= int(eos_id) < V:
        raise ValueError(f"with done, eos_id must be in [0, {V}), got "
                         f"{eos_id}")
    dev = p_logits.device

    def keys(t):
        return sample_keys(t.detach().to(device="cpu", dtype=torch.bfloat16)
                           .contiguous().view(torch.int16).numpy()
                           .view(np.uint16))
    kp, kq = keys(p_logits), keys(q_logits)
    x = draft_tokens.detach().to("cpu").numpy().astype(np.int64)
    greedy = float(temperature) == 0.0
    T = 1.0 if greedy else float(np.float32(temperature))
    rows_b = np.arange(B)
    accept = np.zeros((B, k), dtype=bool)
    aprob = np.zeros((B, k), dtype=np.float64)
    cand = np.zeros((B, k1), dtype=np.int64)
    for t in range(k1):
        if greedy:
            cand[:, t] = kp[:, t].argmax(axis=1)      # lowest index on ties
            if t < k:
                accept[:, t] = x[:, t] == cand[:, t]
                aprob[:, t] = accept[:, t]
            continue
        p, a_p, xp = _spec_softmax(kp[:, t], T)
        word1 = (SPEC_ROW_TAG | (rows_b * k1 + t))[:, None]
        g = -np.log(-np.log(_spec_uniform(np.arange(V)[None, :], word1, step,
                                          seed)))
        score = np.where(kp[:, t] > 0, xp / T + g, -np.inf)
        cand[:, t] = score.argmax(axis=1)             # the draw from p_t
        det = dict(p=p, a_p=a_p, g=g, x=xp, T=T)
        if t < k:
            q, a_q, _ = _spec_softmax(kq[:, t], T)
            ok = (x[:, t] >= 0) & (x[:, t] < V)
            xc = np.clip(x[:, t], 0, V - 1)
            px = np.where(ok, p[rows_b, xc], 0.0)
            qx = np.where(ok, q[rows_b, xc], 0.0)
            u = _spec_uniform(SPEC_ACCEPT_WORD, word1[:, 0], step, seed)
            accept[:, t] = u * qx < px
            aprob[:, t] = np.where(px >= qx, px > 0,
                                   px / np.where(qx > 0, qx, 1.0))
            r = p - q
            pos = r > 0
            res = np.where(pos, np.log(np.where(pos, r, 1.0)) + g, -np.inf)
            cand[:, t] = np.where(pos.any(axis=1), res.argmax(axis=1),
                                  cand[:, t])
            det.update(q=q, a_q=a_q, u=u, px=px, qx=qx)
        if details is not None:
            det["cand"] = cand[:, t].copy()
            details.append(det)
    n_accept = np.cumprod(accept, axis=1).sum(axis=1).astype(np.int32)
    next_token = cand[rows_b, n_accept]
    if done is not None:
        done_np = done.detach().to("cpu").numpy()      # shared when on CPU
        fin = done_np != 0
        n_accept[fin] = 0
        next_token[fin] = int(eos_id)
        aprob[fin] = 0.0
        done_np[:] = fin | (next_token == int(eos_id))
        if done.device.type != "cpu":
            done.copy_(torch.from_numpy(done_np))
    return (torch.from_numpy(n_accept).to(dev),
            torch.from_numpy(next_token).to(dev),
            torch.from_numpy(aprob.astype(np.float32)).to(dev))


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
