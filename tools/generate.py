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
tokens than the CPU paths. Beyond the reference's surface (it has no
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
             use_cache: bool = False) -> torch.Tensor:
    gen = torch.Generator(device="cpu").manual_seed(seed)
    model.eval()
    if use_cache:
        return _generate_cached(model, ids, max_new, temperature, max_len,
                                gen)
    for _ in range(max_new):
        out = model(ids[:, -max_len:])
        logits = out[0] if isinstance(out, tuple) else out
        nxt = _sample(logits[:, -1, :].float().cpu(), temperature, gen)
        ids = torch.cat([ids, nxt.to(ids.device)], dim=1)
    return ids


def _generate_cached(model, ids, max_new, temperature, max_len, gen):
    """One prefill, then one decode_step per token; there is no sliding
    window over the context here, so it all has to fit."""
    from acco_amd.models.kv_cache import KVCache
    total = ids.shape[1] + max_new
    if total > max_len:
        raise ValueError(
            f"--kv-cache needs prompt + max-new <= max_position_embeddings: "
            f"{ids.shape[1]} + {max_new} > {max_len} (the uncached path "
            "slides over the context instead)")
    if max_new <= 0:
        return ids
    cache = KVCache.allocate(model, ids.shape[0], total)
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
    ap.add_argument("overrides", nargs="*",
                    help="config overrides, e.g. model=gptneo")
    args = ap.parse_args(argv)
    if args.top_k < 0 or not args.top_p > 0:
        ap.error("need --top-k >= 0 and --top-p > 0")
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

    ids = torch.tensor([tok.encode(args.prompt).ids], device=device)
    max_len = int(model.cfg.max_position_embeddings)
    if args.device_sampling:
        from acco_amd.models import generate as generate_on_device
        model.eval()
        # stops at the model config's eos_token_id, if it has one
        out, n_new = generate_on_device(
            model, ids, max_new=max(args.max_new, 0),
            temperature=max(args.temperature, 0.0), top_k=args.top_k,
            top_p=args.top_p, seed=args.seed)
        out = out[:, :ids.shape[1] + int(n_new[0])]
    else:
        out = generate(model, ids, args.max_new, args.temperature, max_len,
                       seed=args.seed, use_cache=args.kv_cache)
    text = tok.decode(out[0].tolist())
    print(text)
    return text


if __name__ == "__main__":
    main()
