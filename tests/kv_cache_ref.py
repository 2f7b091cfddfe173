"""Teacher-forced comparison of cached generation with one full forward,
shared by test_kv_cache.py (CPU, fp64 / fp32) and
test_gpu_decode_attention.py (GPU, bf16)."""

import torch

from acco_amd.models.kv_cache import KVCache


def teacher_forced(model, ids, prefix, max_len):
    """(cached logits, full-forward logits), each [n, V]: prefill on the
    ragged prefixes, decode_step fed the true next tokens until the longest
    sequence ends; the full-forward rows are those of the same positions."""
    B, S = ids.shape
    lens = torch.tensor(prefix, dtype=torch.int32, device=ids.device)
    rows = torch.arange(B, device=ids.device)
    with torch.no_grad():
        full = model(ids)[0]
    cache = KVCache.allocate(model, B, max_len)
    width = max(prefix)
    got = [model.prefill(ids[:, :width], lens, cache)]
    want = [full[rows, lens.long() - 1]]
    for step in range(S - width):
        pos = lens.long() + step
        got.append(model.decode_step(ids[rows, pos], cache))
        want.append(full[rows, pos])
    assert cache.steps == S
    assert torch.equal(cache.lens.cpu(),
                       torch.tensor(prefix, dtype=torch.int32) + (S - width))
    return torch.cat(got).double(), torch.cat(want).double()
