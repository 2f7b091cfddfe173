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
3. ops.extend_attention (attn_extend, + combine when the grid splits) at the
   same heads, (B, T, L0) in {(1, 8, 1024), (8, 8, 4096), (1, 256, 3840)},
   Smax = L0 + T, by the method of 2, next to what served the same result
   before it: T successive ops.decode_attention calls (T = 8), or the fp32
   reference math torch_ref.extend_attention (T = 256).

4. Next to every row of 2 and 3 the same call on an e4m3 cache ("kv_dtype":
   "fp8": codes of one byte and one fp32 scale per row, quantised from the
   same random rows), same shapes, same method; its cache_bytes count the
   codes and the scales. 1 gets a third run, use_cache on with the fp8 cache.

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
                        use_cache=bool(use_cache),
                        kv_dtype=FP8 if use_cache == "fp8" else None)

    variants = (False, True, "fp8")
    for use_cache in variants:
        run(use_cache)                       # warm-up: every shape once
    times = {v: [] for v in variants}
    for _ in range(repeats):
        for use_cache in variants:
            sec, out = event_seconds(lambda: run(use_cache))
            assert out.shape[1] == prompt_len + new_tokens
            times[use_cache].append(sec / new_tokens)
    for use_cache in variants:
        t = times[use_cache]
        print(json.dumps({
            "bench": "generate", "model": preset, "use_cache": use_cache,
            "prompt": prompt_len, "new_tokens": new_tokens,
            "s_per_token": min(t), "s_per_token_runs": t}), flush=True)
    return min(times[False]), min(times[True])


FP8 = torch.float8_e4m3fn


def _caches(shape, copies, fp8):
    """`copies` random caches of `shape`: bf16 tensors, or (codes, scales)
    pairs of the same rows for an e4m3 cache."""
    rows = [torch.randn(shape, device="cuda", dtype=torch.bfloat16)
            for _ in range(copies)]
    return [ops.torch_ref.kv_quantize(r) for r in rows] if fp8 else rows


def _scales(kc, vc):
    """(k_cache, v_cache, keyword arguments) of one cache op call."""
    if isinstance(kc, tuple):
        return kc[0], vc[0], dict(k_scale=kc[1], v_scale=vc[1])
    return kc, vc, {}


def bench_decode_kernel(B, L, H=32, Hkv=8, D=64, calls=400,
                        rotate_bytes=1 << 30, fp8=False):
    dev, dt = "cuda", torch.bfloat16
    # K and V: bf16 rows, or one-byte codes and an fp32 scale per row
    cache_bytes = 2 * B * Hkv * L * (D + 4 if fp8 else D * 2)
    copies = max(1, min(512, -(-rotate_bytes // cache_bytes)))
    kcs = _caches((B, Hkv, L, D), copies, fp8)
    vcs = _caches((B, Hkv, L, D), copies, fp8)
    q = torch.randn(B, H, D, device=dev, dtype=dt)
    lens = torch.full((B,), L, device=dev, dtype=torch.int32)
    n_split, chunk = ops.decode_attention_splits(B * Hkv, L)
    out = {}
    for mode, n in (("hot", 1), ("rotating", copies)):
        def loop(count):
            for i in range(count):
                kc, vc, sc = _scales(kcs[i % n], vcs[i % n])
                ops.decode_attention(q, kc, vc, lens, **sc)
        loop(max(20, n))                             # warm-up
        torch.cuda.synchronize()
        sec, _ = event_seconds(lambda: loop(calls))
        out[mode] = sec / calls
    print(json.dumps({
        "bench": "attn_decode+combine", "kv_dtype": "fp8" if fp8 else "bf16",
        "B": B, "L": L, "H": H, "Hkv": Hkv, "D": D, "n_split": n_split, "chunk": chunk,
        "cache_bytes": cache_bytes, "copies": copies,
        "us_hot": out["hot"] * 1e6, "us_rotating": out["rotating"] * 1e6,
        "GBps_hot": cache_bytes / out["hot"] / 1e9,
        "GBps_rotating": cache_bytes / out["rotating"] / 1e9}), flush=True)


def bench_extend_kernel(B, T, L0, H=32, Hkv=8, D=64, calls=200,
                        rotate_bytes=1 << 30, fp8=False):
    dev, dt = "cuda", torch.bfloat16
    Smax = L0 + T
    cache_bytes = 2 * B * Hkv * Smax * (D + 4 if fp8 else D * 2)
    copies = max(1, min(512, -(-rotate_bytes // cache_bytes)))
    kcs = _caches((B, Hkv, Smax, D), copies, fp8)
    vcs = _caches((B, Hkv, Smax, D), copies, fp8)
    q = torch.randn(B, T, H, D, device=dev, dtype=dt)
    lens = torch.full((B,), L0, device=dev, dtype=torch.int32)
    lens_t = [lens + t + 1 for t in range(T)]
    n_blk, n_split, chunk = ops.extend_attention_splits(
        B * Hkv, T * (H // Hkv), Smax)

    def extend(kc, vc):
        kc, vc, sc = _scales(kc, vc)
        ops.extend_attention(q, kc, vc, lens, **sc)

    def decodes(kc, vc):
        kc, vc, sc = _scales(kc, vc)
        for t in range(T):
            ops.decode_attention(q[:, t], kc, vc, lens_t[t], **sc)

    def reference(kc, vc):
        kc, vc, sc = _scales(kc, vc)
        ops.torch_ref.extend_attention(q, kc, vc, lens, **sc)

    base_name, base = (("decode_x_T", decodes) if T <= 8
                       else ("fp32_reference", reference))
    out = {}
    for name, fn, count in (("extend", extend, calls),
                            (base_name, base, max(10, calls // T))):
        for mode, n in (("hot", 1), ("rotating", copies)):
            def loop(k):
                for i in range(k):
                    fn(kcs[i % n], vcs[i % n])
            loop(max(5, min(n, count)))              # warm-up
            torch.cuda.synchronize()
            sec, _ = event_seconds(lambda: loop(count))
            out[name + "_" + mode] = sec / count * 1e6
    print(json.dumps({
        "bench": "attn_extend", "kv_dtype": "fp8" if fp8 else "bf16", "B": B,
        "T": T, "L0": L0, "H": H, "Hkv": Hkv, "D": D, "n_blk": n_blk, "n_split": n_split, "chunk": chunk,
        "cache_bytes": cache_bytes, "copies": copies, "baseline": base_name,
        **{"us_" + k: v for k, v in out.items()}}), flush=True)


def bench_sample_kernel(V=128256, B=8, calls=200, windows=3):
    """ops.sample_logits alone (logits randn * 3, T = 0.8): us per call by
    filter, best of `windows` windows of `calls` calls."""
    x = (torch.randn(B, V, device="cuda") * 3).bfloat16()
    row = {"bench": "sample_logits", "V": V, "B": B}
    for name, kw in (("none", {}), ("top_k50_top_p0.9",
                                    dict(top_k=50, top_p=0.9)),
                     ("greedy", dict(temperature=0.0))):
        def loop(count):
            for i in range(count):
                ops.sample_logits(x, **{"temperature": 0.8, "seed": 1,
                                        "step": i, **kw})
        loop(10)                                     # warm-up
        torch.cuda.synchronize()
        times = [event_seconds(lambda: loop(calls))[0] / calls * 1e6
                 for _ in range(windows)]
        row["us_" + name], row["us_" + name + "_windows"] = min(times), times
    print(json.dumps(row), flush=True)


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
                for fp8 in (False, True):
                    bench_decode_kernel(B, L, fp8=fp8)
        for B, T, L0 in ((1, 8, 1024), (8, 8, 4096), (1, 256, 3840)):
            for fp8 in (False, True):
                bench_extend_kernel(B, T, L0, fp8=fp8)
        bench_sample_kernel()


if __name__ == "__main__":
    main()
