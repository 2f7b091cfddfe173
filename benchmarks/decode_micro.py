"""Generation micro-benchmark: what the KV cache buys, and the decode
attention kernel alone.

1. tools/generate.py's generate() on the llama-1b preset (random weights,
   bf16, B = 1, prompt 128, 128 new tokens, greedy), use_cache off and on in
   this process, alternating (off, on, off, on) after one full warm-up run of
   each, so every sequence length the timed runs meet has been launched
   before. Seconds per generated token, from device events around the whole
   call (the per-token host read of the logits is part of both paths).
2. ops.decode_attention (attn_decode + combine) at the llama-1b heads
   (H 32, Hkv 8, D 64), (B, L) in {1, 8} x {1024, 4096}, cache full. Time per
   call from device events over many calls, and the K and V bytes the call has
   to read per second. "hot" calls one cache again and again (at these sizes
   it stays in the L2 / Infinity Cache); "rotating" walks over copies that
   add up to 1 GiB, more than the caches hold.

Prints one JSON line per measurement. Needs a GPU: there is no CPU fallback.
"""

import argparse
import importlib.util
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

from acco_amd import ops  # noqa: E402


def _generate_fn():
    spec = importlib.util.spec_from_file_location(
        "generate_tool", os.path.join(REPO, "tools", "generate.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.generate


def event_seconds(fn):
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    start.record()
    out = fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / 1e3, out


def bench_generate(preset, prompt_len, new_tokens, repeats):
    from acco_amd.config import load_config
    from acco_amd.models import build_model
    generate = _generate_fn()
    torch.manual_seed(0)
    model = build_model(load_config([f"model={preset}"]).model)
    model = model.to("cuda", dtype=torch.bfloat16).eval()
    max_len = int(model.cfg.max_position_embeddings)
    ids = torch.randint(0, model.cfg.vocab_size, (1, prompt_len),
                        device="cuda")

    def run(use_cache):
        return generate(model, ids, new_tokens, 0.0, max_len,
                        use_cache=use_cache)

    for use_cache in (False, True):
        run(use_cache)                       # warm-up: every shape once
    times = {False: [], True: []}
    for _ in range(repeats):
        for use_cache in (False, True):
            sec, out = event_seconds(lambda: run(use_cache))
            assert out.shape[1] == prompt_len + new_tokens
            times[use_cache].append(sec / new_tokens)
    for use_cache in (False, True):
        t = times[use_cache]
        print(json.dumps({
            "bench": "generate", "model": preset, "use_cache": use_cache,
            "prompt": prompt_len, "new_tokens": new_tokens,
            "s_per_token": min(t), "s_per_token_runs": t}), flush=True)
    return min(times[False]), min(times[True])


def bench_decode_kernel(B, L, H=32, Hkv=8, D=64, calls=400,
                        rotate_bytes=1 << 30):
    dev, dt = "cuda", torch.bfloat16
    cache_bytes = 2 * B * Hkv * L * D * 2            # K and V, bf16
    copies = max(1, min(512, -(-rotate_bytes // cache_bytes)))
    kcs = [torch.randn(B, Hkv, L, D, device=dev, dtype=dt)
           for _ in range(copies)]
    vcs = [torch.randn(B, Hkv, L, D, device=dev, dtype=dt)
           for _ in range(copies)]
    q = torch.randn(B, H, D, device=dev, dtype=dt)
    lens = torch.full((B,), L, device=dev, dtype=torch.int32)
    n_split, chunk = ops.decode_attention_splits(B * Hkv, L)
    out = {}
    for mode, n in (("hot", 1), ("rotating", copies)):
        def loop(count):
            for i in range(count):
                ops.decode_attention(q, kcs[i % n], vcs[i % n], lens)
        loop(max(20, n))                             # warm-up
        torch.cuda.synchronize()
        sec, _ = event_seconds(lambda: loop(calls))
        out[mode] = sec / calls
    print(json.dumps({
        "bench": "attn_decode+combine", "B": B, "L": L, "H": H, "Hkv": Hkv,
        "D": D, "n_split": n_split, "chunk": chunk,
        "cache_bytes": cache_bytes, "copies": copies,
        "us_hot": out["hot"] * 1e6, "us_rotating": out["rotating"] * 1e6,
        "GBps_hot": cache_bytes / out["hot"] / 1e9,
        "GBps_rotating": cache_bytes / out["rotating"] / 1e9}), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama-1b")
    ap.add_argument("--prompt", type=int, default=128)
    ap.add_argument("--new-tokens", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--skip-generate", action="store_true")
    ap.add_argument("--skip-kernel", action="store_true")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("decode_micro.py measures on the GPU; none found")
    if not args.skip_generate:
        off, on = bench_generate(args.model, args.prompt, args.new_tokens,
                                 args.repeats)
        print(json.dumps({"bench": "generate", "off_over_on": off / on}),
              flush=True)
    if not args.skip_kernel:
        for B in (1, 8):
            for L in (1024, 4096):
                bench_decode_kernel(B, L)


if __name__ == "__main__":
    main()
