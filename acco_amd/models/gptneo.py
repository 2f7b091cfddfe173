"""GPT-Neo-family causal LM, MI355X-native.

From-scratch module with ``state_dict`` keys matching HF
``GPTNeoForCausalLM`` (transformer.wte/wpe, transformer.h.N.ln_1,
attn.attention.{q,k,v,out}_proj, mlp.c_fc/c_proj, transformer.ln_f,
lm_head tied to wte), so HF checkpoints load directly.

GPT-Neo specifics faithfully kept (reference config/model/gpt-neo-125M.json):
- learned absolute position embeddings (wpe);
- alternating global / local (banded, window 256) causal attention;
- NO attention scaling (scale = 1.0 — GPT-Neo quirk);
- gelu_new MLP activation; q/k/v projections have no bias, out_proj does.
"""

from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn

from acco_amd import ops
from acco_amd.models.fuse import arena_linear, arena_lm_loss
from acco_amd.models.config import GPTNeoConfig
from acco_amd.models.kv_cache import prefill


class GPTNeoSelfAttention(nn.Module):
    def __init__(self, cfg: GPTNeoConfig, attention_type: str):
        super().__init__()
        d = cfg.hidden_size
        self.cfg = cfg
        self.attention_type = attention_type
        self.k_proj = nn.Linear(d, d, bias=False)
        self.v_proj = nn.Linear(d, d, bias=False)
        self.q_proj = nn.Linear(d, d, bias=False)
        self.out_proj = nn.Linear(d, d, bias=True)
        self._fused_kvq = None    # (w_view, g_view, splits) via models.fuse

    def forward(self, x: torch.Tensor,
                doc_start: Optional[torch.Tensor] = None,
                doc_end: Optional[torch.Tensor] = None,
                kv=None) -> torch.Tensor:
        """`kv` = (k_cache, v_cache, cache_len), prefill only: K and V of
        every position are also appended to the cache; None (the training
        forward) launches nothing for it."""
        B, S, d = x.shape
        H, hd = self.cfg.num_heads, self.cfg.head_dim
        if self._fused_kvq is not None:
            from acco_amd import ops as _ops
            from acco_amd.models.fuse import FusedArenaLinearFn
            w, g, splits = self._fused_kvq
            kvq = FusedArenaLinearFn.apply(x, w, g)
            window = (self.cfg.window_size
                      if self.attention_type == "local" else 0)
            if (kvq.is_cuda and hd == 64 and S % 256 == 0
                    and _ops.have_kernel("attn_fwd_packed")):
                from acco_amd.ops.autograd import AttnQKVPackedFn
                # GPT-Neo packing order k|v|q; no RoPE; no 1/sqrt(d) scale
                offs = (2 * d, 0, d)
                doc = () if doc_start is None else (doc_start, doc_end)
                o = AttnQKVPackedFn.apply(kvq, None, None, H, H, hd, 1.0,
                                          window, offs, *doc)
                if kv is not None:
                    _ops.kv_append(
                        kv[0], kv[1], kv[2],
                        kvq[..., :d].unflatten(-1, (H, hd)),
                        kvq[..., d:2 * d].unflatten(-1, (H, hd)))
                return arena_linear(self.out_proj, o)
            k, v, q = torch.split(kvq, splits, dim=-1)
            q = q.contiguous().view(B, S, H, hd)
            k = k.contiguous().view(B, S, H, hd)
            v = v.contiguous().view(B, S, H, hd)
        else:
            q = self.q_proj(x).view(B, S, H, hd)
            k = self.k_proj(x).view(B, S, H, hd)
            v = self.v_proj(x).view(B, S, H, hd)
        window = self.cfg.window_size if self.attention_type == "local" else None
        if kv is not None:
            ops.kv_append(kv[0], kv[1], kv[2], k, v)
        if doc_start is None:
            o = ops.causal_attention(q, k, v, scale=1.0, window=window)
        else:
            o = ops.causal_attention(q, k, v, scale=1.0, window=window,
                                     doc_start=doc_start, doc_end=doc_end)
        return arena_linear(self.out_proj, o.reshape(B, S, d))

    def decode(self, x: torch.Tensor, cache, layer: int,
               lens1: torch.Tensor) -> torch.Tensor:
        """One token per sequence, x [B, 1, hidden]: project, append K and V
        to layer `layer` of the cache at cache.lens[b], attend the lens1 =
        lens + 1 cached tokens (the last window_size of them in a local
        layer). Uses the per-projection weights, which alias the arena when
        one is installed."""
        B = x.shape[0]
        H, hd = self.cfg.num_heads, self.cfg.head_dim
        q = self.q_proj(x).view(B, H, hd)
        k = self.k_proj(x).view(B, 1, H, hd)
        v = self.v_proj(x).view(B, 1, H, hd)
        kc, vc = cache.k[layer], cache.v[layer]
        ops.kv_append(kc, vc, cache.lens, k, v)
        window = (self.cfg.window_size
                  if self.attention_type == "local" else None)
        o = ops.decode_attention(q, kc, vc, lens1, scale=1.0, window=window)
        return arena_linear(self.out_proj, o.reshape(B, 1, -1))


class GPTNeoAttention(nn.Module):
    """Wrapper level kept so state_dict keys read attn.attention.* like HF."""

    def __init__(self, cfg: GPTNeoConfig, layer_id: int):
        super().__init__()
        self.attention = GPTNeoSelfAttention(cfg, cfg.layer_attention_type(layer_id))

    def forward(self, x, doc_start=None, doc_end=None, kv=None):
        if kv is not None:
            return self.attention(x, doc_start, doc_end, kv)
        return self.attention(x, doc_start, doc_end)


class GPTNeoMLP(nn.Module):
    def __init__(self, cfg: GPTNeoConfig):
        super().__init__()
        self.c_fc = nn.Linear(cfg.hidden_size, cfg.inner_size, bias=True)
        self.c_proj = nn.Linear(cfg.inner_size, cfg.hidden_size, bias=True)

    def forward(self, x):
        return arena_linear(self.c_proj, ops.gelu_new(arena_linear(self.c_fc, x)))


class GPTNeoBlock(nn.Module):
    def __init__(self, cfg: GPTNeoConfig, layer_id: int):
        super().__init__()
        self.ln_1 = nn.LayerNorm(cfg.hidden_size, eps=cfg.layer_norm_epsilon)
        self.attn = GPTNeoAttention(cfg, layer_id)
        self.ln_2 = nn.LayerNorm(cfg.hidden_size, eps=cfg.layer_norm_epsilon)
        self.mlp = GPTNeoMLP(cfg)

    def forward(self, pending, residual, doc_start=None, doc_end=None,
                kv=None, decode=None):
        """(pending, residual) form — every residual add fused into the
        following LayerNorm kernel (see LlamaDecoderLayer); returns the
        un-added MLP output + running residual, ln_f completes the last add.
        `kv` (prefill) is handed to the attention; `decode` = (cache, layer
        index, lens + 1) makes this a single-token step on the cache. Both
        None: the training forward."""
        h1, residual = ops.add_layer_norm(pending, residual, self.ln_1.weight,
                                          self.ln_1.bias, self.ln_1.eps)
        if decode is not None:
            a = self.attn.attention.decode(h1, *decode)
        elif kv is not None:
            a = self.attn(h1, doc_start, doc_end, kv)
        else:
            a = self.attn(h1, doc_start, doc_end)
        h2, residual = ops.add_layer_norm(a, residual, self.ln_2.weight,
                                          self.ln_2.bias, self.ln_2.eps)
        return self.mlp(h2), residual


class GPTNeoModel(nn.Module):
    def __init__(self, cfg: GPTNeoConfig):
        super().__init__()
        self.cfg = cfg
        self.wte = nn.Embedding(cfg.vocab_size, cfg.hidden_size)
        self.wpe = nn.Embedding(cfg.max_position_embeddings, cfg.hidden_size)
        self.h = nn.ModuleList(GPTNeoBlock(cfg, i) for i in range(cfg.num_layers))
        self.ln_f = nn.LayerNorm(cfg.hidden_size, eps=cfg.layer_norm_epsilon)
        # per-layer activation recompute (train.activation_checkpointing)
        self.gradient_checkpointing = False

    def forward(self, input_ids: torch.Tensor,
                doc_start: Optional[torch.Tensor] = None,
                cache=None) -> torch.Tensor:
        """`cache` (a KVCache, prefill only): every layer appends its K / V
        to it at cache.lens. None: the training forward, unchanged."""
        S = input_ids.shape[1]
        pos = torch.arange(S, device=input_ids.device)
        if cache is not None:
            pending = self.wte(input_ids) + self.wpe(pos)[None]
            residual = None
            for i, block in enumerate(self.h):
                pending, residual = block(
                    pending, residual,
                    kv=(cache.k[i], cache.v[i], cache.lens))
            y, _ = ops.add_layer_norm(pending, residual, self.ln_f.weight,
                                      self.ln_f.bias, self.ln_f.eps)
            return y
        doc = ()
        if doc_start is None:
            pending = self.wte(input_ids) + self.wpe(pos)[None]
        else:
            # document masking of packed rows: the learned absolute
            # positions restart with every document, so a document computes
            # what it would compute alone in a row. The key-side array of
            # the backward kernel is derived here, once per forward.
            doc_start = doc_start.to(device=input_ids.device,
                                     dtype=torch.int32).contiguous()
            doc = (doc_start, ops.doc_end_from_start(doc_start))
            pending = self.wte(input_ids) + self.wpe(pos[None] - doc_start)
        residual = None
        if (self.gradient_checkpointing and self.training
                and torch.is_grad_enabled()):
            from torch.utils.checkpoint import checkpoint
            for block in self.h:
                pending, residual = checkpoint(block, pending, residual,
                                               *doc, use_reentrant=False)
        else:
            for block in self.h:
                pending, residual = block(pending, residual, *doc)
        y, _ = ops.add_layer_norm(pending, residual, self.ln_f.weight,
                                  self.ln_f.bias, self.ln_f.eps)
        return y

    def decode_step(self, tokens: torch.Tensor, cache) -> torch.Tensor:
        """Hidden state [B, hidden] of one new token per sequence at position
        cache.lens[b] (wpe is read there; the host-side step count keeps it
        below max_len); appends to every layer of the cache and advances
        cache.lens once, after the last layer."""
        pos = cache.lens.long().clamp(0, self.wpe.num_embeddings - 1)
        pending = (self.wte(tokens) + self.wpe(pos))[:, None]
        residual = None
        lens1 = cache.lens + 1
        for i, block in enumerate(self.h):
            pending, residual = block(pending, residual,
                                      decode=(cache, i, lens1))
        y, _ = ops.add_layer_norm(pending, residual, self.ln_f.weight,
                                  self.ln_f.bias, self.ln_f.eps)
        cache.lens = lens1
        return y[:, 0]


class GPTNeoForCausalLM(nn.Module):
    config_class = GPTNeoConfig
    # train.fused_lm_loss / train.lm_loss_chunk_tokens (LlamaForCausalLM has
    # the note)
    fused_lm_loss = False
    lm_loss_chunk_tokens = 4096

    def __init__(self, cfg: GPTNeoConfig):
        super().__init__()
        self.cfg = cfg
        self.transformer = GPTNeoModel(cfg)
        self.lm_head = nn.Linear(cfg.hidden_size, cfg.vocab_size, bias=False)
        if cfg.tie_word_embeddings:
            self.lm_head.weight = self.transformer.wte.weight
        self.apply(self._init_weights)

    def _init_weights(self, module):
        std = self.cfg.initializer_range
        if isinstance(module, nn.Linear):
            module.weight.data.normal_(0.0, std)
            if module.bias is not None:
                module.bias.data.zero_()
        elif isinstance(module, nn.Embedding):
            module.weight.data.normal_(0.0, std)
        elif isinstance(module, nn.LayerNorm):
            module.weight.data.fill_(1.0)
            module.bias.data.zero_()

    def forward(self, input_ids: torch.Tensor,
                labels: Optional[torch.Tensor] = None,
                attention_mask: Optional[torch.Tensor] = None,
                doc_start: Optional[torch.Tensor] = None,
                label_smoothing: float = 0.0):
        """`attention_mask` is accepted and unused; `doc_start` (int32
        [B, S], ops.doc_start_from_eos) keeps attention inside each document
        of a packed row and restarts the positions per document.
        `label_smoothing` is the HF-LabelSmoother epsilon of the loss. With
        `fused_lm_loss` set and labels given the result is (loss, None)."""
        hidden = (self.transformer(input_ids) if doc_start is None
                  else self.transformer(input_ids, doc_start))
        if labels is not None and self.fused_lm_loss:
            # chunked head + loss: the [B, S, V] logits never exist
            loss = arena_lm_loss(self.lm_head, hidden, labels,
                                 label_smoothing, self.lm_loss_chunk_tokens)
            return (loss, None)
        logits = arena_linear(self.lm_head, hidden)
        if labels is None:
            return (logits,)
        loss = ops.label_smoothed_causal_lm_loss(logits, labels,
                                                 label_smoothing)
        return (loss, logits)

    @torch.no_grad()
    def prefill(self, input_ids: torch.Tensor, lens: Optional[torch.Tensor],
                cache) -> torch.Tensor:
        """Run the prompt [B, S] (sequence b holds lens[b] <= S tokens, the
        rest is right-padding; None = all S) through the blocks, fill `cache`
        and return the logits [B, V] of each sequence's last prompt token."""
        return prefill(self, self.transformer, input_ids, lens, cache)

    @torch.no_grad()
    def decode_step(self, tokens: torch.Tensor, cache) -> torch.Tensor:
        """Logits [B, V] after one more token per sequence, tokens [B], given
        everything already in `cache`; raises ValueError once the cache is
        full (a host-side count, no device read)."""
        cache.room_for(1)
        hidden = self.transformer.decode_step(tokens, cache)
        cache.steps += 1
        return arena_linear(self.lm_head, hidden)
