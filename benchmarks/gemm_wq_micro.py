"""Tiled quantised GEMM micro-benchmark: ops.gemm_w8 / ops.gemm_w4 next to
ops.linear_w8 / ops.linear_w4 (the skinny kernel at M = 64, above it the
fallback that dequantises the weight to a bf16 temporary and calls
torch.matmul: what W8Linear / W4Linear ran before they routed by row count)
and F.linear on the bf16 weight of the same shape, in one process. The manner
of linear_w4_micro.py; the helpers are linear_w8_micro.py's.

1. M in ROWS rows of bf16 x against the (N, K) of linear_w8_micro.SHAPES, per
   format the three variants alternating window by window; every call of a
   window takes the next of several copies of the weight that add up to 1 GiB
   in bf16, so the weight comes from HBM. A window is fewer calls at large
   shapes (about 2 TFLOP of product per window). Reports the best window and
   all windows of each variant, the tiles and splits ops.gemm_w?_tiles chose
   and the peak memory one call of each path allocates.
2. The routing caps ops.W8_GEMM_MAX_ROWS / ops.W4_GEMM_MAX_ROWS these rows
   give: the largest M of ROWS above 64 such that at it and at every smaller
   one the GEMM's best window is no longer than the linear's at every shape
   (None: through the last; 64: nowhere).
3. acco_amd.models.generate on a preset (random weights, bf16, B = 1, prompt
   128, 128 new tokens, greedy) in bf16, fp8 and fp4, each quantised model
   with the modules routed to the GEMM (caps None) and as before (caps 64),
   alternating.

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

FP4 = torch.float4_e2m1fn_x2
ROWS = [64, 65, 128, 256, 512, 1024, 2048, 4096]
FORMATS = {"fp8": (ops.torch_ref.weight_quantize, ops.linear_w8, ops.gemm_w8,
                   ops.gemm_w8_tiles),
           "fp4": (ops.torch_ref.weight_quantize_mxfp4, ops.linear_w4,
                   ops.gemm_w4, ops.gemm_w4_tiles)}


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn(0)
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def bench_shape(N, K, rows, calls, windows, rotate_bytes=1 << 30):
    copies = max(2, min(256, -(-rotate_bytes // (2 * N * K))))
    ws = [torch.randn(N, K, device="cuda", dtype=torch.bfloat16) * 0.02
          for _ in range(copies)]
    out = []
    for fmt, (quantize, linear, gemm, tiles) in FORMATS.items():
        qs = [quantize(w) for w in ws]
        for M in rows:
            x = torch.randn(M, K, device="cuda", dtype=torch.bfloat16)
            run = {"linear": lambda i: linear(x, *qs[i % copies]),
                   "gemm": lambda i: gemm(x, *qs[i % copies]),
                   "bf16": lambda i: F.linear(x, ws[i % copies])}
            n = max(3, min(calls, int(2e12 / (2.0 * M * N * K))))
            times = {k: [] for k in run}
            for k in run:
                window_seconds(run[k], min(n, copies))      # warm-up
            for _ in range(windows):
                for k in run:
                    times[k].append(window_seconds(run[k], n))
            row = {"bench": "gemm_wq", "format": fmt, "M": M, "N": N, "K": K,
                   "copies": copies, "calls": n, "tiles": tiles(M, N, K)}
            for k in run:
                row.update({k + "_us": min(times[k]) * 1e6,
                            k + "_us_windows": [s * 1e6 for s in times[k]],
                            k + "_peak_MiB": peak_bytes(run[k]) / 2 ** 20})
            row["gemm_over_linear"] = row["gemm_us"] / row["linear_us"]
            row["gemm_over_bf16"] = row["gemm_us"] / row["bf16_us"]
            print(json.dumps(row), flush=True)
            out.append(row)
        del qs
    return out


def caps(results, rows):
    """Per format the cap the measured rows give (the docstring's rule)."""
    for fmt in FORMATS:
        cap = 64
        for M in [m for m in rows if m > 64]:
            if any(r["gemm_us"] > r["linear_us"] for r in results
                   if r["format"] == fmt and r["M"] == M):
                break
            cap = M
        else:
            cap = None
        print(json.dumps({"bench": "gemm_wq_cap", "format": fmt,
                          "max_rows": cap}), flush=True)


def bench_generate(preset, prompt_len, new_tokens, repeats):
    from acco_amd.config import load_config
    from acco_amd.models import build_model, generate, quantize_weights
    torch.manual_seed(0)
    model = build_model(load_config([f"model={preset}"]).model)
    model = model.to("cuda", dtype=torch.bfloat16).eval()
    q8, q4 = quantize_weights(model), quantize_weights(model, dtype=FP4)
    # (model, the two caps while it runs): 64 routes every call as before
    models = {"bf16": (model, None), "fp8_gemm": (q8, None),
              "fp8_before": (q8, 64), "fp4_gemm": (q4, None),
              "fp4_before": (q4, 64)}
    ids = torch.randint(0, model.cfg.vocab_size, (1, prompt_len),
                        device="cuda")

    def run(m, cap):
        ops.W8_GEMM_MAX_ROWS = ops.W4_GEMM_MAX_ROWS = cap
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
        run(*models[k])                              # warm-up
    for _ in range(repeats):
        for k in models:
            times[k].append(run(*models[k]))
    for k in models:
        print(json.dumps({
            "bench": "generate", "model": preset, "weights": k,
            "prompt": prompt_len, "new_tokens": new_tokens,
            "tokens_per_s": new_tokens / min(times[k]),
            "seconds_runs": times[k]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--rows", type=int, nargs="*", default=ROWS)
    ap.add_argument("--preset", default="llama-1b")
    ap.add_argument("--new-tokens", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--skip-generate", action="store_true")
    ap.add_argument("--skip-shapes", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gemm_wq_micro.py needs a GPU")
    if not args.skip_shapes:
        results = []
        for N, K in SHAPES:
            results += bench_shape(N, K, args.rows, args.calls, args.windows)
        caps(results, args.rows)
    if not args.skip_generate:
        bench_generate(args.preset, 128, args.new_tokens, args.repeats)


if __name__ == "__main__":
    main()
