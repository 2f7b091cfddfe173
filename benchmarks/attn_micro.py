"""Attention kernel micro-benchmark / profiling target.

Default: the flagship shape (llama-1b, b8 s1024); --8b: llama-8b heads at
b4 s512; --s2048 / --s512: the flagship heads at S=2048 (b4) / S=512 (b16),
the same token count. Next to the times it prints what the placement of the
workgroups on the 8 XCDs predicts: the tile-iterations of the heaviest class
id % 8 over the mean, for the 2-D (row block, head) grid the kernels used to
launch and for the order they launch now (attn_block_order).
"""

import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from acco_amd import ops

BLOCK_ROWS, TILE = 256, 64        # 32x32 kernels: rows per workgroup / tile


def xcd_imbalance(order, n_blk, heavy_last):
    """Heaviest id % 8 class over the mean, in causal tile-iterations.
    order: (row block, head) per linear block id."""
    per_blk = BLOCK_ROWS // TILE
    sums = [0] * 8
    for i, (rb, _) in enumerate(order):
        sums[i % 8] += per_blk * ((rb + 1) if heavy_last else (n_blk - rb))
    return max(sums) * 8 / sum(sums)


def placement_prediction(B, S, H):
    n_blk = S // BLOCK_ROWS
    out = {}
    for kern, heavy_last in (("fwd/dq", True), ("dkv", False)):
        grid2d = [(rb, bh) for bh in range(B * H) for rb in range(n_blk)]
        out[kern] = [xcd_imbalance(grid2d, n_blk, heavy_last), None]
        ext = ops.hip_ext()
        if hasattr(ext, "attn_block_order"):
            order = ext.attn_block_order(n_blk, B, H, heavy_last).tolist()
            out[kern][1] = xcd_imbalance(order, n_blk, heavy_last)
    return out


def main():
    torch.manual_seed(0)
    B, S, H, Hkv, Dh = 8, 1024, 32, 8, 64
    if "--8b" in sys.argv:
        B, S, H, Hkv, Dh = 4, 512, 32, 8, 128
    if "--s2048" in sys.argv:
        B, S = 4, 2048
    if "--s512" in sys.argv:
        B, S = 16, 512
    print(f"shape: B={B} S={S} H={H} Hkv={Hkv} D={Dh}")
    for kern, (old, new) in placement_prediction(B, S, H).items():
        new_s = "n/a (no attn_block_order)" if new is None else f"{new:.3f}"
        print(f"heaviest XCD / mean, {kern}: 2-D grid {old:.3f}, "
              f"block order {new_s}")
    q = torch.randn(B, S, H, Dh, device="cuda").bfloat16()
    k = torch.randn(B, S, Hkv, Dh, device="cuda").bfloat16()
    v = torch.randn(B, S, Hkv, Dh, device="cuda").bfloat16()
    do = torch.randn(B, S, H, Dh, device="cuda").bfloat16()
    sc = Dh ** -0.5
    o, l = ops.hip_ext().attn_fwd(q, k, v, sc, 0)
    delta = (do.float() * o.float()).sum(-1).permute(0, 2, 1).contiguous()

    iters = 20
    for _ in range(3):
        ops.hip_ext().attn_fwd(q, k, v, sc, 0)
        ops.hip_ext().attn_bwd(q, k, v, do, l, delta, sc, 0)
    torch.cuda.synchronize()
    t = time.time()
    for _ in range(iters):
        ops.hip_ext().attn_fwd(q, k, v, sc, 0)
    torch.cuda.synchronize()
    dt_f = (time.time() - t) / iters
    t = time.time()
    for _ in range(iters):
        ops.hip_ext().attn_bwd(q, k, v, do, l, delta, sc, 0)
    torch.cuda.synchronize()
    dt_b = (time.time() - t) / iters
    fl_f = 2 * 2 * B * H * S * S * Dh * 0.5          # causal: half the tiles
    fl_b = fl_f * 2.5
    print(f"attn fwd:  {dt_f*1e3:.3f} ms, ~{fl_f/dt_f/1e12:.0f} TF/s")
    print(f"attn bwd:  {dt_b*1e3:.3f} ms, ~{fl_b/dt_b/1e12:.0f} TF/s")
    dt = dt_f + dt_b
    print(f"attn fwd+bwd: {dt*1e3:.3f} ms, "
          f"~{(fl_f+fl_b)/dt/1e12:.0f} TF/s combined")


if __name__ == "__main__":
    main()
