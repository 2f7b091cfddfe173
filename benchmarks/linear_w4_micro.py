"""MXFP4 weight-only decode linear micro-benchmark: ops.linear_w4 (e2m1 codes,
one e8m0 scale per 32 weights) next to ops.linear_w8 (e4m3 codes, one scale
per output row) and F.linear on the bf16 weight of the same shape, in one
process. The manner of linear_w8_micro.py, whose helpers it uses.

1. M in {1, 8, 32, 64} rows of bf16 x against the (N, K) of
   linear_w8_micro.SHAPES. Time per call from device events over many calls,
   the three variants alternating window by window; every call of a window
   takes the next of several copies of the weight that add up to 1 GiB in
   bf16, more than the caches hold, so the weight comes from HBM. GB/s counts
   the weight bytes the call has to read (N K / 2 codes plus N K / 32 scales
   for fp4; N K plus 4 N for fp8; 2 N K for bf16). The split counts are what
   ops.linear_w4_splits and ops.linear_w8_splits chose.
2. acco_amd.models.generate on a preset (random weights, bf16, B = 1, prompt
   128, 128 new tokens, greedy) in bf16, fp8 and fp4 (quantised once, outside
   the timed call), alternating. Tokens per second from device events around
   the whole call.

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
from benchmarks.linear_w8_micro import ROWS, SHAPES, window_seconds  # noqa: E402

FP4 = torch.float4_e2m1fn_x2


def bench_shape(N, K, calls, windows, rotate_bytes=1 << 30):
    copies = max(2, min(256, -(-rotate_bytes // (2 * N * K))))
    ws = [torch.randn(N, K, device="cuda", dtype=torch.bfloat16) * 0.02
          for _ in range(copies)]
    q8 = [ops.torch_ref.weight_quantize(w) for w in ws]
    q4 = [ops.torch_ref.weight_quantize_mxfp4(w) for w in ws]
    for M in ROWS:
        x = torch.randn(M, K, device="cuda", dtype=torch.bfloat16)
        run = {"bf16": lambda i: F.linear(x, ws[i % copies]),
               "fp8": lambda i: ops.linear_w8(x, *q8[i % copies]),
               "fp4": lambda i: ops.linear_w4(x, *q4[i % copies])}
        nbytes = {"bf16": 2 * N * K, "fp8": N * K + 4 * N,
                  "fp4": N * K // 2 + N * K // 32}
        times = {k: [] for k in run}
        for k in run:
            window_seconds(run[k], copies)          # warm-up: every copy once
        for _ in range(windows):
            for k in run:
                times[k].append(window_seconds(run[k], calls))
        row = {"bench": "linear_w4", "M": M, "N": N, "K": K, "copies": copies,
               "fp4_splits": ops.linear_w4_splits(M, N, K),
               "fp8_splits": ops.linear_w8_splits(M, N, K)}
        for k in run:
            t = min(times[k])
            row.update({k + "_us": t * 1e6, k + "_GBps": nbytes[k] / t / 1e9,
                        k + "_us_windows": [s * 1e6 for s in times[k]]})
        row["fp4_over_fp8"] = row["fp4_us"] / row["fp8_us"]
        row["fp4_over_bf16"] = row["fp4_us"] / row["bf16_us"]
        print(json.dumps(row), flush=True)


def bench_generate(preset, prompt_len, new_tokens, repeats):
    from acco_amd.config import load_config
    from acco_amd.models import build_model, generate, quantize_weights
    torch.manual_seed(0)
    model = build_model(load_config([f"model={preset}"]).model)
    model = model.to("cuda", dtype=torch.bfloat16).eval()
    models = {"bf16": model, "fp8": quantize_weights(model),
              "fp4": quantize_weights(model, dtype=FP4)}
    ids = torch.randint(0, model.cfg.vocab_size, (1, prompt_len),
                        device="cuda")

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
        run(models[k])                               # warm-up
    for _ in range(repeats):
        for k in models:
            times[k].append(run(models[k]))
    for k in models:
        print(json.dumps({
            "bench": "generate", "model": preset, "weight_dtype": k,
            "prompt": prompt_len, "new_tokens": new_tokens,
            "tokens_per_s": new_tokens / min(times[k]),
            "seconds_runs": times[k]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--preset", default="llama-1b")
    ap.add_argument("--new-tokens", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--skip-generate", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("linear_w4_micro.py needs a GPU")
    for N, K in SHAPES:
        bench_shape(N, K, args.calls, args.windows)
    if not args.skip_generate:
        bench_generate(args.preset, 128, args.new_tokens, args.repeats)


if __name__ == "__main__":
    main()
