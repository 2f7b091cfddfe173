"""Synthetic OpenWebText/Alpaca-shaped data for benchmarking.

This environment has no network, so the benchmark path trains
on random token ids of the reference workload's shape (const-length packed
sequences, reference config/train/acco.yaml:4,16). Deterministic per index.
"""

from __future__ import annotations

from typing import Optional

import torch
from torch.utils.data import Dataset


class SyntheticCausalLMDataset(Dataset):
    def __init__(self, n_sequences: int, seq_len: int, vocab_size: int,
                 seed: int = 1234):
        self.n = int(n_sequences)
        self.seq_len = int(seq_len)
        self.vocab = int(vocab_size)
        self.seed = int(seed)

    def __len__(self) -> int:
        return self.n

    def __getitem__(self, idx: int):
        g = torch.Generator().manual_seed(self.seed * 1_000_003 + idx)
        ids = torch.randint(0, self.vocab, (self.seq_len,), generator=g)
        return {"input_ids": ids}


def collate_input_ids(batch):
    """Stack const-length sequences (reference trainer_base.py:131-132)."""
    return {"input_ids": torch.stack(
        [torch.as_tensor(b["input_ids"], dtype=torch.long) for b in batch])}


class DocMaskCollator:
    """collate_input_ids plus a `doc_start` entry (train.doc_mask): the
    int32 [B, S] document starts of the packed rows, derived from the EOS
    that the packer appends to every document (ops.doc_start_from_eos)."""

    def __init__(self, eos_token_id: int):
        self.eos_token_id = int(eos_token_id)

    def __call__(self, batch):
        from acco_amd import ops
        out = collate_input_ids(batch)
        out["doc_start"] = ops.doc_start_from_eos(out["input_ids"],
                                                  self.eos_token_id)
        return out


def resolve_doc_mask_eos(doc_mask, tokenizer, model) -> Optional[int]:
    """The EOS id that train.doc_mask splits packed rows at, or None when
    the flag is off: the tokenizer's when there is one, else the model
    config's `eos_token_id`. Neither: an error at start-up."""
    if not doc_mask:
        return None
    eos = getattr(tokenizer, "eos_token_id", None)
    if eos is None:
        eos = getattr(getattr(model, "cfg", None), "eos_token_id", None)
    if eos is None:
        raise ValueError(
            "train.doc_mask=true needs an EOS token id to find the document "
            "boundaries: pass a tokenizer with eos_token_id or set "
            "eos_token_id in the model config")
    return int(eos)


def make_padded_collator(pad_token_id: int, pad_to_multiple: int = 64):
    """Ragged-batch collator for the finetune path (const_len_batch=false):
    right-pads input_ids and masks padded positions with -100 in labels —
    the behaviour of the reference's DataCollatorForLanguageModeling
    (trainer_base.py:209). Padding to a multiple of 64 keeps the flash
    kernels' S%64 contract."""
    def collate(batch):
        seqs = [torch.as_tensor(b["input_ids"], dtype=torch.long)
                for b in batch]
        longest = max(s.numel() for s in seqs)
        target = ((longest + pad_to_multiple - 1) // pad_to_multiple
                  * pad_to_multiple)
        ids = torch.full((len(seqs), target), pad_token_id, dtype=torch.long)
        labels = torch.full((len(seqs), target), -100, dtype=torch.long)
        for i, s in enumerate(seqs):
            ids[i, :s.numel()] = s
            labels[i, :s.numel()] = s
        return {"input_ids": ids, "labels": labels}
    return collate
