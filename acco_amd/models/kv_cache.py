"""KV cache for generation: per-layer K / V of every token seen so far, so a
new token costs one single-token forward (`decode_step`) instead of a
re-forward of the whole context.

Layout (ops.kv_append / ops.decode_attention): per layer a `k` and a `v`
[B, Hkv, max_len, D] in the model's dtype, K stored after RoPE; `lens` int32
[B] on the device = tokens cached per sequence, so a batch may be ragged.
`lens` is never read on the host: `steps` is the host's own count of the
longest sequence (the prompt width plus the decode steps taken), which is all
that is needed to refuse a step past `max_len`."""

from __future__ import annotations

from typing import List, Optional, Tuple

import torch


class KVCache:
    def __init__(self, k: List[torch.Tensor], v: List[torch.Tensor],
                 lens: torch.Tensor, max_len: int,
                 rope: Optional[Tuple[torch.Tensor, torch.Tensor]] = None):
        self.k, self.v = k, v
        self.lens = lens
        self.max_len = int(max_len)
        self.rope = rope      # fp32 (cos, sin) [max_len, D], Llama only
        self.steps = 0        # host-side upper bound of max(lens)

    @classmethod
    def allocate(cls, model, batch: int, max_len: int, device=None,
                 dtype=None) -> "KVCache":
        """An empty cache for `batch` sequences of up to `max_len` tokens of
        `model` (LlamaForCausalLM or GPTNeoForCausalLM). `device` / `dtype`
        default to those of the model's parameters."""
        cfg = model.cfg
        if not 1 <= int(max_len) <= int(cfg.max_position_embeddings):
            raise ValueError(
                f"max_len must be in [1, max_position_embeddings = "
                f"{cfg.max_position_embeddings}], got {max_len}")
        p = next(model.parameters())
        device = p.device if device is None else torch.device(device)
        dtype = p.dtype if dtype is None else dtype
        hkv = int(getattr(cfg, "num_kv_heads", cfg.num_heads))
        shape = (int(batch), hkv, int(max_len), int(cfg.head_dim))
        n = int(cfg.num_layers)
        k = [torch.zeros(shape, device=device, dtype=dtype) for _ in range(n)]
        v = [torch.zeros(shape, device=device, dtype=dtype) for _ in range(n)]
        lens = torch.zeros(int(batch), device=device, dtype=torch.int32)
        rope = None
        if hasattr(cfg, "rope_theta"):
            from acco_amd.ops import torch_ref
            # row p of these equals row p of the table of any full forward
            rope = torch_ref.rope_cos_sin(int(max_len), int(cfg.head_dim),
                                          cfg.rope_theta, device)
        return cls(k, v, lens, max_len, rope)

    @property
    def batch(self) -> int:
        return self.k[0].shape[0]

    def begin(self, width: int, lens: torch.Tensor) -> None:
        """The cache now holds a prompt of `width` columns, `lens[b]` of them
        valid in sequence b."""
        self.lens = lens.to(device=self.lens.device,
                            dtype=torch.int32).contiguous()
        self.steps = int(width)

    def room_for(self, n: int = 1) -> None:
        """Raise if `n` more tokens would pass max_len (host arithmetic on
        the step count; no device read)."""
        if self.steps + n > self.max_len:
            raise ValueError(
                f"KV cache is full: {self.steps} tokens cached, {n} more "
                f"would pass max_len = {self.max_len}")


def padded_prompt_len(S: int, max_pos: int) -> int:
    """Width the prompt is right-padded to: the next multiple of 256 if that
    stays within max_position_embeddings, else of 64, else S. Attention is
    causal, so the pad cannot change an earlier position; it only moves the
    prompt from the reference math onto the flash kernels."""
    for mult in (256, 64):
        up = -(-S // mult) * mult
        if up <= max_pos:
            return up
    return S


def prefill(lm, backbone, input_ids: torch.Tensor,
            lens: Optional[torch.Tensor], cache: KVCache) -> torch.Tensor:
    """Shared body of LlamaForCausalLM.prefill / GPTNeoForCausalLM.prefill
    (`backbone` = lm.model / lm.transformer; the callers hold no_grad)."""
    from acco_amd.models.fuse import arena_linear
    B, S = input_ids.shape
    if B != cache.batch or not 1 <= S <= cache.max_len:
        raise ValueError(
            f"prompt [B, S] = [{B}, {S}] does not fit a cache of batch "
            f"{cache.batch} and max_len {cache.max_len}")
    dev = input_ids.device
    if lens is None:
        lens = torch.full((B,), S, device=dev, dtype=torch.int32)
    lens = lens.to(device=dev, dtype=torch.int32).clamp(1, S)
    pad = padded_prompt_len(S, int(lm.cfg.max_position_embeddings)) - S
    ids = torch.nn.functional.pad(input_ids, (0, pad)) if pad else input_ids
    # every layer appends at row 0; the rows the pad (and a ragged batch's
    # right-padding) writes lie at or beyond lens[b]: never read, and
    # overwritten by later appends
    cache.lens = torch.zeros(B, device=dev, dtype=torch.int32)
    hidden = backbone(ids, cache=cache)
    cache.begin(S, lens)
    last = hidden[torch.arange(B, device=dev), lens.long() - 1]   # [B, hid]
    return arena_linear(lm.lm_head, last)
