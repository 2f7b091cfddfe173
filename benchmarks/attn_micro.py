"""Attention kernel micro-benchmark / profiling target.

Default: the flagship shape (llama-1b, b8 s1024); --8b: llama-8b heads at
b4 s512; --s2048 / --s512: the flagship heads at S=2048 (b4) / S=512 (b16),
the same token count. Next to the times it prints what the placement of the
workgroups on the 8 XCDs predicts: the tile-iterations of the heaviest class
id % 8 over the mean, for the 2-D (row block, head) grid the kernels used to
launch and for the order they launch now (attn_block_order).

--doc-len N lays documents of N tokens over the shape (N = S: one document,
the DOC kernels with nothing to mask) and times the plain and the DOC path
in this process, alternating (plain, DOC, plain, DOC, plain): the three
repeats of the plain path give the run-to-run spread to read the DOC times
against.
Next to each time it prints the tile iterations the kernels' ranges predict,
per workgroup loop ("staged": every tile a block loads) and per wave
("computed": the tiles a wave does not skip).
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


def tile_iterations(S, doc_len):
    """Predicted tile iterations of one (b, h) for documents of doc_len
    tokens (doc_len = None: the plain kernels), from the ranges of
    attention_common.h: {kernel: (staged, computed)}."""
    nt = S // TILE
    ds = [(s // doc_len) * doc_len if doc_len else 0 for s in range(S)]
    de = [min(d + doc_len, S) if doc_len else S for d in ds]
    waves = BLOCK_ROWS // 32
    fwd_staged = fwd_comp = dkv_staged = dkv_comp = 0
    for blk in range(S // BLOCK_ROWS):
        r0 = blk * BLOCK_ROWS
        # forward / dq: kv tiles of a q block
        j_lo = min(ds[r0] // TILE, nt - 1)
        j_hi = (r0 + BLOCK_ROWS - 1) // TILE
        fwd_staged += max(0, j_hi - j_lo + 1)
        # dkv: q tiles of a kv block
        qt_lo = r0 // TILE
        qt_hi = min(nt - 1, (de[r0 + BLOCK_ROWS - 1] - 1) // TILE)
        dkv_staged += max(0, qt_hi - qt_lo + 1)
        for w in range(waves):
            w0 = r0 + 32 * w
            fwd_comp += sum(1 for j in range(j_lo, j_hi + 1)
                            if j * TILE <= w0 + 31
                            and j * TILE + TILE - 1 >= ds[w0])
            dkv_comp += sum(1 for t in range(qt_lo, qt_hi + 1)
                            if t * TILE + TILE - 1 >= w0
                            and t * TILE < de[w0 + 31])
    return {"fwd": (fwd_staged, fwd_comp), "dq": (fwd_staged, fwd_comp),
            "dkv": (dkv_staged, dkv_comp)}


def time_paths(q, k, v, do, sc, doc, iters=1000):
    """(fwd ms, bwd ms) of one path; doc = () or (doc_start, doc_end)."""
    ext = ops.hip_ext()
    o, l = ext.attn_fwd(q, k, v, sc, 0, *doc[:1])
    delta = ext.attn_delta(do, o)
    for _ in range(3):
        ext.attn_fwd(q, k, v, sc, 0, *doc[:1])
        ext.attn_bwd(q, k, v, do, l, delta, sc, 0, *doc)
    torch.cuda.synchronize()
    t = time.time()
    for _ in range(iters):
        ext.attn_fwd(q, k, v, sc, 0, *doc[:1])
    torch.cuda.synchronize()
    dt_f = (time.time() - t) / iters
    t = time.time()
    for _ in range(iters):
        ext.attn_bwd(q, k, v, do, l, delta, sc, 0, *doc)
    torch.cuda.synchronize()
    return dt_f * 1e3, (time.time() - t) / iters * 1e3


def doc_comparison(q, k, v, do, sc, doc_len):
    B, S = q.shape[:2]
    pos = torch.arange(S, device="cuda")
    ds = ((pos // doc_len) * doc_len).to(torch.int32).expand(B, S).contiguous()
    de = ops.doc_end_from_start(ds)
    plain_it, doc_it = tile_iterations(S, None), tile_iterations(S, doc_len)
    print(f"doc-len {doc_len}: {(S + doc_len - 1) // doc_len} documents per "
          "row; tile iterations per (b, h), staged / computed:")
    for kern in ("fwd", "dq", "dkv"):
        print(f"  {kern:4s} plain {plain_it[kern][0]:4d} / "
              f"{plain_it[kern][1]:4d}   doc {doc_it[kern][0]:4d} / "
              f"{doc_it[kern][1]:4d}")
    for rep in range(5):
        doc = (ds, de) if rep % 2 else ()
        f, b = time_paths(q, k, v, do, sc, doc)
        print(f"{'doc  ' if doc else 'plain'} #{rep // 2}: fwd {f:.3f} ms  "
              f"bwd {b:.3f} ms")


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
    if "--doc-len" in sys.argv:
        doc_len = int(sys.argv[sys.argv.index("--doc-len") + 1])
        if not (0 < doc_len <= S and S % BLOCK_ROWS == 0):
            raise SystemExit("--doc-len needs 0 < N <= S and S % 256 == 0")
        doc_comparison(q, k, v, do, sc, doc_len)
        return
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
