"""Teacher-forced `extend` run shared by test_extend_attention.py (CPU, fp64)
and test_gpu_extend_attention.py (GPU, bf16)."""

import torch

from acco_amd.models.kv_cache import KVCache


def teacher_forced_extend(model, ids, prefix, width, max_len):
    """prefill on the ragged prefixes, then extend in slices of `width` fed
    the true next tokens until every sequence reaches S = ids.shape[1]; a
    sequence that is done rides along with n_new = 0. Returns (logits [n, V],
    b [n], pos [n], cache): row i is the model's output at ids[b[i], pos[i]]."""
    B, S = ids.shape
    dev = ids.device
    lens = torch.tensor(prefix, dtype=torch.int32, device=dev)
    rows = torch.arange(B, device=dev)
    cache = KVCache.allocate(model, B, max_len)
    got = [model.prefill(ids[:, :max(prefix)], lens, cache)]
    bs, ps = [rows], [lens.long() - 1]
    done, todo = 0, S - min(prefix)
    while done < todo:
        T = min(width, todo - done)
        pos = lens.long()[:, None] + done + torch.arange(T, device=dev)[None]
        n_new = (S - lens - done).clamp(0, T)
        logits = model.extend(ids.gather(1, pos.clamp(max=S - 1)), cache,
                              n_new=n_new)
        valid = torch.arange(T, device=dev)[None] < n_new[:, None]
        got.append(logits[valid])
        bs.append(rows[:, None].expand(B, T)[valid])
        ps.append(pos[valid])
        done += T
    assert cache.steps == max(prefix) + todo
    assert bool((cache.lens == S).all())
    return torch.cat(got).double(), torch.cat(bs), torch.cat(ps), cache
