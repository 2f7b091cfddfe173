"""MXFP4 x MXFP8 GEMM micro-benchmark: ops.gemm_w4a8 (the activation
quantiser's time included) next to ops.gemm_w4, the quantiser alone and
F.linear on the bf16 weight of the same shape, in one process. The method and
the helpers are gemm_wq_micro.py's.

1. M in ROWS rows of bf16 x against the (N, K) of linear_w8_micro.SHAPES, the
   four variants alternating window by window; every call of a window takes
   the next of several copies of the weight that add up to 1 GiB in bf16, so
   the weight comes from HBM. Reports the best window and all windows of each
   variant and the tiles and splits ops.gemm_w4a8_tiles chose.
2. The routing floor ops.W4A8_GEMM_MIN_ROWS these rows give, the rule of
   gemm_wq_cap mirrored: the smallest M of ROWS such that at it and at every
   larger one gemm_w4a8's best window is no longer than gemm_w4's at every
   shape (None: there is no such M).
3. acco_amd.models.generate on a preset (random weights, B = 1, prompt 2048,
   16 new tokens, greedy): MXFP4 weights with act_dtype against MXFP4 weights
   without it, alternating.

Prints one JSON line per measurement. Needs a GPU: there is no CPU fallback.
"""

import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from acco_amd import ops  # noqa: E402
from benchmarks.linear_w8_micro import SHAPES, window_seconds  # noqa: E402

FP4, FP8 = torch.float4_e2m1fn_x2, torch.float8_e4m3fn
ROWS = [65, 128, 256, 512, 1024, 2048, 4096]


def bench_shape(N, K, rows, calls, windows, rotate_bytes=1 << 30):
    copies = max(2, min(256, -(-rotate_bytes // (2 * N * K))))
    ws = [torch.randn(N, K, device="cuda", dtype=torch.bfloat16) * 0.02
          for _ in range(copies)]
    qs = [ops.torch_ref.weight_quantize_mxfp4(w) for w in ws]
    out = []
    for M in rows:
        x = torch.randn(M, K, device="cuda", dtype=torch.bfloat16)
        run = {"gemm_w4": lambda i: ops.gemm_w4(x, *qs[i % copies]),
               "gemm_w4a8": lambda i: ops.gemm_w4a8(x, *qs[i % copies]),
               "quant": lambda i: ops.act_quantize_mxfp8(x),
               "bf16": lambda i: F.linear(x, ws[i % copies])}
        n = max(3, min(calls, int(2e12 / (2.0 * M * N * K))))
        times = {k: [] for k in run}
        for k in run:
            window_seconds(run[k], min(n, copies))      # warm-up
        for _ in range(windows):
            for k in run:
                times[k].append(window_seconds(run[k], n))
        row = {"bench": "gemm_w4a8", "M": M, "N": N, "K": K, "copies": copies,
               "calls": n, "tiles": ops.gemm_w4a8_tiles(M, N, K)}
        for k in run:
            row.update({k + "_us": min(times[k]) * 1e6,
                        k + "_us_windows": [s * 1e6 for s in times[k]]})
        row["w4a8_over_w4"] = row["gemm_w4a8_us"] / row["gemm_w4_us"]
        row["w4a8_over_bf16"] = row["gemm_w4a8_us"] / row["bf16_us"]
        row["quant_share"] = row["quant_us"] / row["gemm_w4a8_us"]
        print(json.dumps(row), flush=True)
        out.append(row)
    return out


def min_rows(results, rows):
    """The floor the measured rows give (the docstring's rule)."""
    floor = None
    for M in sorted(rows, reverse=True):
        if any(r["gemm_w4a8_us"] > r["gemm_w4_us"] for r in results
               if r["M"] == M):
            break
        floor = M
    print(json.dumps({"bench": "gemm_w4a8_min_rows", "min_rows": floor}),
          flush=True)


def bench_generate(preset, prompt_len, new_tokens, repeats):
    from acco_amd.config import load_config
    from acco_amd.models import build_model, generate, quantize_weights
    torch.manual_seed(0)
    model = build_model(load_config([f"model={preset}"]).model)
    model = model.to("cuda", dtype=torch.bfloat16).eval()
    models = {"fp4": quantize_weights(model, dtype=FP4),
              "fp4_act_fp8": quantize_weights(model, dtype=FP4, act_dtype=FP8)}
    ids = torch.randint(0, model.cfg.vocab_size, (1, prompt_len),
                        device="cuda")
    ops.W4A8_GEMM_MIN_ROWS = 65     # an explicit act_dtype routes from 65

    def run(m):
        start = torch.cuda.Event(enable_timing=True)
        end = torch.cuda.Event(enable_timing=True)
        start.record()
        generate(m, ids, max_new=new_tokens, temperature=0.0, seed=0,
                 eos_token_id=None)
        end.record()
        torch.cuda.synchronize()
        return start.elapsed_time(end) / 1e3

    times = {k: [] for k in models}
    for k in models:
        run(models[k])                              # warm-up
    for _ in range(repeats):
        for k in models:
            times[k].append(run(models[k]))
    for k in models:
        print(json.dumps({
            "bench": "generate", "model": preset, "weights": k,
            "prompt": prompt_len, "new_tokens": new_tokens,
            "seconds": min(times[k]), "seconds_runs": times[k]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--rows", type=int, nargs="*", default=ROWS)
    ap.add_argument("--preset", default="llama-1b")
    ap.add_argument("--prompt", type=int, default=2048)
    ap.add_argument("--new-tokens", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--skip-generate", action="store_true")
    ap.add_argument("--skip-shapes", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gemm_w4a8_micro.py needs a GPU")
    if not args.skip_shapes:
        results = []
        for N, K in SHAPES:
            results += bench_shape(N, K, args.rows, args.calls, args.windows)
        min_rows(results, args.rows)
    if not args.skip_generate:
        bench_generate(args.preset, args.prompt, args.new_tokens, args.repeats)


if __name__ == "__main__":
    main()
