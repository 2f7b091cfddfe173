"""Sample text from a trained checkpoint (sanity/demo tool).

Greedy or temperature sampling. By default every new token re-forwards the
whole context (sliding over the last max_position_embeddings tokens); with
--kv-cache the prompt is prefilled once into a KV cache and every new token
is one single-token decode step on it (models/kv_cache.py), which needs
prompt + max-new <= max_position_embeddings. Both paths share the sampling
code and the seeded generator, which run on the CPU: the logits are copied to
the host every token. --device-sampling (implies --kv-cache) runs
acco_amd.models.generate instead: top-k / top-p and the draw happen on the
model's device from a counter-based generator, so the same --seed gives other
tokens than the CPU paths. --prefill-chunk N (implies --kv-cache) pushes the
prompt through the cache N tokens at a time. --kv-dtype fp8 (implies
--kv-cache) stores the cache as e4m3 codes with one scale per row, about half
the bytes per cached token. --weight-dtype fp8 generates from
models.quantize_weights(model): every linear as e4m3 codes with one scale per
output row, half the weight bytes per token (any of the paths above; the HIP
kernel serves a bf16 model on the GPU). --weight-dtype fp4 does the same in
OCP MXFP4: e2m1 codes with one power-of-two scale per 32 weights, about 0.53
bytes per weight; with it, --act-dtype fp8 rounds the activations of the
prefill to OCP MXFP8 for the MXFP4 x MXFP8 GEMM. --draft-weight-dtype {fp8,fp4} --spec-k K (implies
--device-sampling; not with --top-k / --top-p) decodes speculatively with a
quantised copy of the checkpoint as its own draft: K drafted tokens per
round, checked by one forward of the model and ops.spec_verify. Beyond the
reference's surface (it has no
generation path); useful for judging what a checkpoint learned.

Usage (config overrides use the same syntax as main.py):
  python tools/generate.py --ckpt checkpoints/<id>_model.pt \\
      --tokenizer corpus/tokenizer --prompt "the" --max-new 64 \\
      --temperature 0.8 [--kv-cache] model=gptneo [model.hidden_size=... ...]
  ... --device-sampling --top-k 50 --top-p 0.9 ...
"""

from __future__ import annotations

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _sample(step: torch.Tensor, temperature: float,
            gen: torch.Generator) -> torch.Tensor:
    """Next token [B, 1] from the last position's logits [B, V] (on the CPU)."""
    if temperature <= 0:
        return step.argmax(-1, keepdim=True)
    probs = torch.softmax(step / temperature, dim=-1)
    return torch.multinomial(probs, 1, generator=gen)


@torch.no_grad()
def generate(model, ids: torch.Tensor, max_new: int, temperature: float,
             max_len: int, seed: int = 0,
             use_cache: bool = False,
             prefill_chunk: int = 0, kv_dtype=None) -> torch.Tensor:
    gen = torch.Generator(device="cpu").manual_seed(seed)
    model.eval()
    if use_cache or prefill_chunk > 0 or kv_dtype is not None:
        return _generate_cached(model, ids, max_new, temperature, max_len,
                                gen, prefill_chunk, kv_dtype)
    for _ in range(max_new):
        out = model(ids[:, -max_len:])
        logits = out[0] if isinstance(out, tuple) else out
        nxt = _sample(logits[:, -1, :].float().cpu(), temperature, gen)
        ids = torch.cat([ids, nxt.to(ids.device)], dim=1)
    return ids


def _generate_cached(model, ids, max_new, temperature, max_len, gen,
                     prefill_chunk=0, kv_dtype=None):
    """One prefill (in slices of `prefill_chunk` tokens when that is set),
    then one decode_step per token; there is no sliding window over the
    context here, so it all has to fit."""
    from acco_amd.models.kv_cache import KVCache, prefill_chunked
    total = ids.shape[1] + max_new
    if total > max_len:
        raise ValueError(
            f"--kv-cache needs prompt + max-new <= max_position_embeddings: "
            f"{ids.shape[1]} + {max_new} > {max_len} (the uncached path "
            "slides over the context instead)")
    if max_new <= 0:
        return ids
    cache = KVCache.allocate(model, ids.shape[0], total, dtype=kv_dtype)
    if 0 < prefill_chunk < ids.shape[1]:
        logits = prefill_chunked(model, ids, None, cache, prefill_chunk)
    else:
        logits = model.prefill(ids, None, cache)
    for i in range(max_new):
        nxt = _sample(logits.float().cpu(), temperature, gen).to(ids.device)
        ids = torch.cat([ids, nxt], dim=1)
        if i + 1 < max_new:
            logits = model.decode_step(nxt[:, 0], cache)
    return ids


def main(argv=None) -> str:
    ap = argparse.ArgumentParser()
    ap.add_argument("--ckpt", required=True,
                    help=".pt state dict or HF-style model dir")
    ap.add_argument("--tokenizer", required=True,
                    help="dir with tokenizer.json")
    ap.add_argument("--prompt", default="the")
    ap.add_argument("--max-new", type=int, default=64)
    ap.add_argument("--temperature", type=float, default=0.8)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--kv-cache", action="store_true",
                    help="prefill once, then one cached decode step per "
                         "token (needs prompt + max-new <= "
                         "max_position_embeddings)")
    ap.add_argument("--prefill-chunk", type=int, default=0,
                    help="push the prompt through the cache this many "
                         "tokens at a time (implies --kv-cache; 0 = one "
                         "prefill of the whole prompt)")
    ap.add_argument("--kv-dtype", choices=("bf16", "fp8"), default="bf16",
                    help="fp8: keep the KV cache as e4m3 codes with one "
                         "scale per row (implies --kv-cache); bf16: in the "
                         "model's dtype")
    ap.add_argument("--weight-dtype", choices=("bf16", "fp8", "fp4"),
                    default="bf16",
                    help="fp8: generate from a copy of the model whose "
                         "linears hold e4m3 weight codes with one scale per "
                         "output row; fp4: MXFP4 codes with one scale per 32 "
                         "weights; bf16: the checkpoint's own weights")
    ap.add_argument("--act-dtype", choices=("bf16", "fp8"), default="bf16",
                    help="fp8 (needs --weight-dtype fp4): calls of 65 rows "
                         "and more (the prefill) round their activations to "
                         "OCP MXFP8 and run the MXFP4 x MXFP8 GEMM; decode "
                         "steps stay weight-only")
    ap.add_argument("--device-sampling", action="store_true",
                    help="sample on the model's device with "
                         "acco_amd.models.generate (implies --kv-cache): no "
                         "copy of the logits to the host per token; draws "
                         "come from its own seeded generator, not the CPU one")
    ap.add_argument("--top-k", type=int, default=0,
                    help="keep the k largest logits (0 = off; needs "
                         "--device-sampling)")
    ap.add_argument("--top-p", type=float, default=1.0,
                    help="nucleus mass (>= 1 = off; needs --device-sampling)")
    ap.add_argument("--draft-weight-dtype", choices=("fp8", "fp4"),
                    default=None,
                    help="speculative decoding with a quantised copy of the "
                         "checkpoint as the draft (implies "
                         "--device-sampling; not with --top-k / --top-p)")
    ap.add_argument("--spec-k", type=int, default=4,
                    help="drafted tokens per round with --draft-weight-dtype")
    ap.add_argument("overrides", nargs="*",
                    help="config overrides, e.g. model=gptneo")
    args = ap.parse_args(argv)
    if args.prefill_chunk < 0:
        ap.error("need --prefill-chunk >= 0")
    if args.top_k < 0 or not args.top_p > 0:
        ap.error("need --top-k >= 0 and --top-p > 0")
    if args.act_dtype == "fp8" and args.weight_dtype != "fp4":
        ap.error("--act-dtype fp8 needs --weight-dtype fp4")
    if args.draft_weight_dtype is not None:
        if args.top_k != 0 or args.top_p < 1.0:
            ap.error("--draft-weight-dtype does not combine with --top-k / "
                     "--top-p")
        if args.spec_k < 1:
            ap.error("need --spec-k >= 1")
        args.device_sampling = True
    if (args.top_k != 0 or args.top_p < 1.0) and not args.device_sampling:
        ap.error("--top-k / --top-p need --device-sampling")

    from acco_amd.config import load_config
    from acco_amd.models import build_model, load_pretrained
    from tokenizers import Tokenizer

    device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
    tok = Tokenizer.from_file(os.path.join(args.tokenizer, "tokenizer.json"))

    cfg = load_config(args.overrides)
    model = build_model(cfg.model,
                        vocab_size_override=tok.get_vocab_size())
    load_pretrained(model, args.ckpt)
    model = model.to(device)
    codes = {"fp8": torch.float8_e4m3fn, "fp4": torch.float4_e2m1fn_x2}
    draft = None
    if args.draft_weight_dtype is not None:
        from acco_amd.models import quantize_weights
        draft = quantize_weights(model.eval(), codes[args.draft_weight_dtype])
    if args.weight_dtype != "bf16":
        from acco_amd.models import quantize_weights
        model = quantize_weights(
            model.eval(), codes[args.weight_dtype],
            torch.float8_e4m3fn if args.act_dtype == "fp8" else None)

    ids = torch.tensor([tok.encode(args.prompt).ids], device=device)
    kv_dtype = torch.float8_e4m3fn if args.kv_dtype == "fp8" else None
    max_len = int(model.cfg.max_position_embeddings)
    if args.device_sampling:
        from acco_amd.models import generate as generate_on_device
        model.eval()
        # stops at the model config's eos_token_id, if it has one
        out, n_new = generate_on_device(
            model, ids, max_new=max(args.max_new, 0),
            temperature=max(args.temperature, 0.0), top_k=args.top_k,
            top_p=args.top_p, seed=args.seed,
            prefill_chunk=args.prefill_chunk, kv_dtype=kv_dtype,
            draft=draft, spec_k=args.spec_k)
        out = out[:, :ids.shape[1] + int(n_new[0])]
    else:
        out = generate(model, ids, args.max_new, args.temperature, max_len,
                       seed=args.seed, use_cache=args.kv_cache,
                       prefill_chunk=args.prefill_chunk, kv_dtype=kv_dtype)
    text = tok.decode(out[0].tolist())
    print(text)
    return text


if __name__ == "__main__":
    main()
