"""Speculative decoding on one GPU: what ops.spec_verify costs, and what
generate(draft=...) gains or loses against the plain loop.

1. Verify kernels (spec_verify.hip, both launches) at V in {50304, 128256},
   B in {1, 8}, k in {2, 4, 8}, temperature 0.8 and greedy: device events
   over many calls, best of a few windows. q is p plus unit noise and the
   drafted tokens are q's argmax, so every row runs its residual pass.
2. generate on a model preset, B = 1, prompt 128, 128 new tokens, greedy and
   T = 0.8: the plain loop against draft = the MXFP4 and the e4m3 copy of the
   model itself at spec_k in {2, 4}. All variants run in one process,
   alternating, after a warm-up of each. Tokens per second from device
   events around the whole call, rounds counted at the target's extend, and
   the mean number of drafted tokens accepted per round.

The presets have random weights: what a quantised self-draft accepts there
says little about a trained model. One JSON line per measurement.
"""

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from acco_amd import ops  # noqa: E402


def window_seconds(fn, calls):
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    start.record()
    for i in range(calls):
        fn(i)
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / 1e3 / calls


def bench_verify(calls, windows):
    g = torch.Generator().manual_seed(0)
    for V in (50304, 128256):
        for B in (1, 8):
            for k in (2, 4, 8):
                p = (torch.randn(B, k + 1, V, generator=g) * 3).bfloat16()
                q = (p[:, :k].float()
                     + torch.randn(B, k, V, generator=g)).bfloat16()
                p, q = p.cuda(), q.cuda()
                x = q.argmax(-1)
                row = {"bench": "spec_verify", "V": V, "B": B, "k": k,
                       "logit_bytes": 2 * V * B * (2 * k + 1)}
                for name, T in (("sampled", 0.8), ("greedy", 0.0)):
                    def run(i):
                        ops.spec_verify(p, q, x, temperature=T, seed=1,
                                        step=i)
                    window_seconds(run, 10)
                    times = [window_seconds(run, calls)
                             for _ in range(windows)]
                    row[name + "_us"] = min(times) * 1e6
                    row[name + "_us_windows"] = [t * 1e6 for t in times]
                print(json.dumps(row), flush=True)


def bench_generate(preset, prompt_len, new_tokens, repeats):
    from acco_amd.config import load_config
    from acco_amd.models import build_model, generate, quantize_weights
    torch.manual_seed(0)
    model = build_model(load_config([f"model={preset}"]).model)
    model = model.to("cuda", dtype=torch.bfloat16).eval()
    drafts = {"fp4": quantize_weights(model, torch.float4_e2m1fn_x2),
              "fp8": quantize_weights(model, torch.float8_e4m3fn)}
    variants = {"plain": None}
    variants.update({f"{d}_k{k}": (drafts[d], k)
                     for d in drafts for k in (2, 4)})
    ids = torch.randint(0, model.cfg.vocab_size, (1, prompt_len),
                        device="cuda")
    rounds = []
    extend = model.extend
    model.extend = lambda *a, **kw: (rounds.append(1), extend(*a, **kw))[1]

    def run(spec, T):
        del rounds[:]
        kw = {} if spec is None else dict(draft=spec[0], spec_k=spec[1])
        start = torch.cuda.Event(enable_timing=True)
        end = torch.cuda.Event(enable_timing=True)
        start.record()
        generate(model, ids, max_new=new_tokens, temperature=T, seed=0,
                 eos_token_id=None, **kw)
        end.record()
        torch.cuda.synchronize()
        return start.elapsed_time(end) / 1e3, len(rounds)

    for T in (0.0, 0.8):
        times = {name: [] for name in variants}
        n_rounds = {}
        for name, spec in variants.items():
            run(spec, T)                                 # warm-up
        for _ in range(repeats):
            for name, spec in variants.items():
                t, n_rounds[name] = run(spec, T)
                times[name].append(t)
        for name, spec in variants.items():
            row = {"bench": "generate_spec", "model": preset,
                   "variant": name, "temperature": T, "prompt": prompt_len,
                   "new_tokens": new_tokens,
                   "tokens_per_s": new_tokens / min(times[name]),
                   "seconds_runs": times[name]}
            if spec is not None:
                row.update(rounds=n_rounds[name], accepted_per_round=(
                    new_tokens / n_rounds[name] - 1))
            print(json.dumps(row), flush=True)


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
        raise SystemExit("spec_decode_micro.py needs a GPU")
    bench_verify(args.calls, args.windows)
    if not args.skip_generate:
        bench_generate(args.preset, 128, args.new_tokens, args.repeats)


if __name__ == "__main__":
    main()
