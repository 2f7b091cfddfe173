"""ms/step of the ACCO round at the llama-1b shape (bench.py's set-up) with a
given max_grad_norm, plus the com round timed alone on an idle device."""

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

import bench


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--max-grad-norm", type=float, default=0.0)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    args = ap.parse_args()

    from acco_amd.engine import arena
    from acco_amd.engine.acco import AccoEngine
    from acco_amd.engine.scheduler import LRSchedule
    from acco_amd.engine.sharded_adamw import ShardedAdamW
    from acco_amd.models import LlamaConfig, LlamaForCausalLM
    from acco_amd.models.fuse import install_fused_projections
    from acco_amd.parallel.comm import CommBackend, ShardSpec

    device = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    torch.manual_seed(42)
    mcfg = LlamaConfig(**bench.MODELS["llama-1b"])
    model = LlamaForCausalLM(mcfg)
    n_live = arena.live_numel(model)
    spec = ShardSpec.build(n_live, 1, buckets=8)
    params = arena.flatten_params(model, torch.bfloat16, device,
                                  pad_to=spec.total)
    grads = arena.attach_grad_arena(model, torch.bfloat16, device,
                                    pad_to=spec.total)
    comm = CommBackend(device)
    install_fused_projections(model, params, grads)
    opt = ShardedAdamW(spec, 0, device, lr=6e-4, betas=(0.9, 0.95), eps=1e-8,
                       weight_decay=0.1, max_grad_norm=args.max_grad_norm)
    opt.init_master_from_buffer(params)
    sched = LRSchedule(6e-4, 1000, 50_000, "cosine")
    pool = bench.make_batch_pool(8, 8, 1024, mcfg.vocab_size, device, 1234)
    idx = [0]

    def next_batch():
        t = pool[idx[0] % len(pool)]
        idx[0] += 1
        return {"input_ids": t.to(device, non_blocking=True)}

    def forward_backward(inputs):
        ids = inputs["input_ids"]
        loss, _ = model(ids, labels=ids)
        loss.backward()
        return loss.detach()

    eng = AccoEngine(params_arena=params, grads_arena=grads, n_live=n_live,
                     spec=spec, comm=comm, rank=0, device=device, opt=opt,
                     sched=sched, forward_backward=forward_backward,
                     next_batch=next_batch, n_grad_accumulation=1)
    state = {}
    warmup, steps = args.warmup, args.steps

    def boundary(r):
        if r == warmup:
            torch.cuda.synchronize()
            state["t0"] = time.time()
        elif r == warmup + steps:
            torch.cuda.synchronize()
            state["t1"] = time.time()

    eng.on_round_boundary = boundary
    eng.enable_arena_swap(model, grads)
    eng.train_acco(nb_grad_tot=1 << 60, n_warmup_steps=0,
                   max_rounds=warmup + steps)
    torch.cuda.synchronize()
    timed = eng.com_log[warmup:warmup + steps]
    res = {"max_grad_norm": args.max_grad_norm,
           "ms_per_step": (state["t1"] - state["t0"]) / steps * 1e3,
           "com_round_ms_overlapped": 1e3 * sum(e["t"] for e in timed)
           / len(timed),
           "loss": float(eng.loss_static),
           "grad_norm_last": eng.com_log[-1].get("grad_norm"),
           "clip_coef_last": eng.com_log[-1].get("clip_coef")}

    # the com round alone, device otherwise idle
    alone = []
    for i in range(12):
        eng.com_buffer.copy_(eng.grads)
        eng.count_grad_this_round.fill_(1)
        torch.cuda.synchronize()
        t = time.time()
        eng.communication_round(commit=bool(i % 2))
        torch.cuda.synchronize()
        alone.append(time.time() - t)
    alone = sorted(alone[2:])
    res["com_round_ms_alone_median"] = 1e3 * alone[len(alone) // 2]
    res["com_round_ms_alone_min"] = 1e3 * alone[0]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
