"""FP8 weight-only decode linear micro-benchmark: ops.linear_w8 (e4m3 codes,
one scale per output row) next to F.linear on the bf16 weight of the same
shape, which is what a decode step runs without quantize_weights.

1. M in {1, 8, 32, 64} rows of bf16 x against (N, K) of the shipped configs:
   4096x4096, 6144x4096 (q|k|v rows), 14336x4096, 4096x14336, 128256x4096
   (llama3-8b), 768x768, 50257x768 (gpt-neo-125M). Time per call from device
   events over many calls, the two variants alternating window by window;
   every call of a window takes the next of several copies of the weight that
   add up to 1 GiB, more than the caches hold, so the weight comes from HBM.
   GB/s counts the weight bytes the call has to read (N K for codes plus 4 N
   for scales; 2 N K for bf16). The split count is what
   ops.linear_w8_splits chose.
2. acco_amd.models.generate on a preset (random weights, bf16, B = 1, prompt
   128, 128 new tokens, greedy), with and without weight_dtype fp8 (quantised
   once, outside the timed call), alternating. Tokens per second from device
   events around the whole call.

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

SHAPES = [(4096, 4096), (6144, 4096), (14336, 4096), (4096, 14336),
          (128256, 4096), (768, 768), (50257, 768)]
ROWS = [1, 8, 32, 64]


def window_seconds(fn, calls):
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    start.record()
    for i in range(calls):
        fn(i)
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / 1e3 / calls


def bench_shape(N, K, calls, windows, rotate_bytes=1 << 30):
    copies = max(2, min(256, -(-rotate_bytes // (2 * N * K))))
    ws = [torch.randn(N, K, device="cuda", dtype=torch.bfloat16) * 0.02
          for _ in range(copies)]
    qs = [ops.torch_ref.weight_quantize(w) for w in ws]
    for M in ROWS:
        x = torch.randn(M, K, device="cuda", dtype=torch.bfloat16)
        run = {"bf16": lambda i: F.linear(x, ws[i % copies]),
               "fp8": lambda i: ops.linear_w8(x, *qs[i % copies])}
        nbytes = {"bf16": 2 * N * K, "fp8": N * K + 4 * N}
        times = {k: [] for k in run}
        for k in run:
            window_seconds(run[k], copies)          # warm-up: every copy once
        for _ in range(windows):
            for k in run:
                times[k].append(window_seconds(run[k], calls))
        n_split, k_chunk = ops.linear_w8_splits(M, N, K)
        row = {"bench": "linear_w8", "M": M, "N": N, "K": K,
               "n_split": n_split, "k_chunk": k_chunk, "copies": copies}
        for k in run:
            t = min(times[k])
            row.update({k + "_us": t * 1e6, k + "_GBps": nbytes[k] / t / 1e9,
                        k + "_us_windows": [s * 1e6 for s in times[k]]})
        row["fp8_over_bf16"] = row["fp8_us"] / row["bf16_us"]
        print(json.dumps(row), flush=True)


def bench_generate(preset, prompt_len, new_tokens, repeats):
    from acco_amd.config import load_config
    from acco_amd.models import build_model, generate, quantize_weights
    torch.manual_seed(0)
    model = build_model(load_config([f"model={preset}"]).model)
    model = model.to("cuda", dtype=torch.bfloat16).eval()
    models = {"bf16": model, "fp8": quantize_weights(model)}
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
        raise SystemExit("linear_w8_micro.py needs a GPU")
    for N, K in SHAPES:
        bench_shape(N, K, args.calls, args.windows)
    if not args.skip_generate:
        bench_generate(args.preset, 128, args.new_tokens, args.repeats)


if __name__ == "__main__":
    main()
