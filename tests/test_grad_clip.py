"""Global gradient-norm clipping on the CPU path: the ops reference against
torch.nn.utils.clip_grad_norm_, single-process clipped ACCO rounds, the
native DDP and the threaded ACCO engine (world 2, gloo) against clipped
oracles, and the config / trainer / com-log surface."""

import glob
import importlib.util
import json
import os

import pytest
import torch
import torch.nn as nn

from tests import test_acco_oracle as acco_t
from tests import test_ddp_native as ddp_t
from tests.conftest import run_distributed
from tests.dist_utils import init_worker, teardown_worker

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------- ops against torch
@pytest.mark.parametrize("max_norm,grad_scale", [
    (0.5, 1.0),                          # clipped
    (1e4, 1.0),                          # not clipped
    (0.5, torch.tensor([0.25])),         # clipped, tensor scale (1/count)
    (1e4, torch.tensor([0.25])),
])
def test_ops_reference_matches_clip_grad_norm(max_norm, grad_scale):
    from acco_amd import ops
    gen = torch.Generator().manual_seed(3)
    shapes = [(7, 5), (11,), (3, 4, 2)]
    raw = [torch.randn(*s, generator=gen) for s in shapes]
    flat = torch.cat([g.reshape(-1) for g in raw])

    n_part = ops.grad_sumsq_partials(flat.numel(), flat.dtype, "cpu")
    assert n_part == 1
    partials = torch.full((n_part,), float("nan"))
    assert ops.grad_sumsq(flat, partials) == 1
    sumsq = torch.full((1,), float("nan"))
    ops.sumsq_finalize(partials, sumsq)
    scale, norm, coef = ops.clip_grad_scale(sumsq, grad_scale, max_norm)
    for t in (scale, norm, coef):
        assert t.shape == (1,) and t.dtype == torch.float32

    params = [nn.Parameter(torch.zeros(*s)) for s in shapes]
    for p, g in zip(params, raw):
        p.grad = g * float(grad_scale)
    total = torch.nn.utils.clip_grad_norm_(params, max_norm)
    want = torch.cat([p.grad.reshape(-1) for p in params])
    assert torch.allclose(norm, total.reshape(1), rtol=1e-6, atol=0)
    assert torch.allclose(flat * scale, want, rtol=1e-6, atol=1e-9)
    assert (float(coef) < 1.0) == (float(total) > max_norm)
    if float(total) <= max_norm:
        assert float(coef) == 1.0 and float(scale) == float(grad_scale)


def test_clip_grad_scale_non_finite_propagates():
    from acco_amd import ops
    for bad in (float("inf"), float("nan")):
        scale, norm, coef = ops.clip_grad_scale(torch.tensor([bad]), 0.5, 1.0)
        want = torch.clamp(1.0 / (torch.tensor([bad]) + 1e-6), max=1.0) * 0.5
        assert torch.equal(scale.isnan(), want.isnan())
        assert bad != bad or float(scale) == float(want)
        assert not torch.isfinite(norm).all()


# ---------------------------------------- single-process engine rounds
def _cpu_engine(max_grad_norm):
    from acco_amd.engine.acco import AccoEngine
    from acco_amd.engine.scheduler import LRSchedule
    from acco_amd.engine.sharded_adamw import ShardedAdamW
    from acco_amd.parallel.comm import CommBackend, ShardSpec
    n = 29
    spec = ShardSpec.build(n, 1, buckets=3, align=2)
    device = torch.device("cpu")
    gen = torch.Generator().manual_seed(5)
    opt = ShardedAdamW(spec, 0, device, lr=1e-2, weight_decay=0.01,
                       max_grad_norm=max_grad_norm)
    opt.p.copy_(torch.randn(spec.owned, generator=gen))
    opt.m.copy_(torch.randn(spec.owned, generator=gen) * 0.01)
    opt.v.copy_(torch.rand(spec.owned, generator=gen) * 0.001)
    opt.step_count = 2
    arena = torch.zeros(spec.total)
    eng = AccoEngine(params_arena=arena, grads_arena=torch.zeros(spec.total),
                     n_live=n, spec=spec, comm=CommBackend(device), rank=0,
                     device=device, opt=opt,
                     sched=LRSchedule(1e-2, 4, 100, "cosine"),
                     forward_backward=None, next_batch=None)
    grads = torch.zeros(spec.total)
    grads[:n] = torch.randn(n, generator=gen) * 2.0
    return eng, grads


def test_engine_rounds_clip_tentative_then_commit():
    from acco_amd.ops import torch_ref
    max_norm, count = 0.7, 3
    eng, grads = _cpu_engine(max_norm)
    opt = eng.opt
    assert opt.clipping
    for commit in (False, True):
        p0, m0, v0 = opt.p.clone(), opt.m.clone(), opt.v.clone()
        eng.com_buffer.copy_(grads)
        eng.count_grad_this_round.fill_(count)
        lr, step = eng.sched.lr(), opt.step_count
        assert eng.communication_round(commit=commit) == count

        total = (grads / count).norm()
        assert float(total) > max_norm
        coef = torch.clamp(max_norm / (total + 1e-6), max=1.0)
        p, m, v = p0.clone(), m0.clone(), v0.clone()
        out = torch.empty_like(p)
        torch_ref.fused_adamw_step(p, grads, m, v, step, lr, 0.9, 0.95, 1e-8,
                                   0.01, grad_scale=float(coef) / count,
                                   out_bf16=out, commit=commit)
        assert torch.allclose(eng.com_buffer, out, rtol=1e-6, atol=1e-8)
        entry = eng.com_log[-1]
        assert abs(entry["grad_norm"] - float(total)) <= 1e-6 * float(total)
        assert abs(entry["clip_coef"] - float(coef)) <= 1e-6
        if commit:
            assert torch.allclose(opt.p, p, rtol=1e-6, atol=1e-8)
            assert torch.allclose(opt.m, m, rtol=1e-6, atol=1e-8)
            assert torch.allclose(opt.v, v, rtol=1e-6, atol=1e-10)
            assert opt.step_count == step + 1
        else:                       # the tentative round leaves the state
            assert torch.equal(opt.p, p0) and torch.equal(opt.m, m0)
            assert torch.equal(opt.v, v0) and opt.step_count == step


def test_engine_round_without_clipping_is_unchanged():
    """Off (None and 0): no norm in the com log, and the round equals the
    round of an engine whose max_grad_norm never binds, bit for bit."""
    results = []
    for mx in (None, 0, 1e30):
        eng, grads = _cpu_engine(mx)
        eng.com_buffer.copy_(grads)
        eng.count_grad_this_round.fill_(3)
        eng.communication_round(commit=True)
        assert ("grad_norm" in eng.com_log[-1]) == (mx == 1e30)
        results.append((eng.com_buffer.clone(), eng.opt.p.clone(),
                        eng.opt.m.clone(), eng.opt.v.clone()))
    for other in results[1:]:
        for a, b in zip(results[0], other):
            assert torch.equal(a, b)


# ------------------------------------------------------------- DDP ws2
DDP_MAX_NORM = 1.2


def _worker_ddp_clip(rank, world, port, tmpdir):
    init_worker(rank, world, port)
    from acco_amd.engine import arena
    from acco_amd.engine.sharded_adamw import ShardedAdamW
    from acco_amd.parallel.comm import CommBackend, ShardSpec
    from acco_amd.parallel.ddp import NativeZeroDDP

    model = ddp_t.make_model()
    device = torch.device("cpu")
    n = arena.live_numel(model)
    spec = ShardSpec.build(n, world, buckets=2, align=2)
    params = arena.flatten_params(model, torch.float32, device,
                                  pad_to=spec.total)
    grads = arena.attach_grad_arena(model, torch.float32, device,
                                    pad_to=spec.total)
    comm = CommBackend(device)
    opt = ShardedAdamW(spec, rank, device, lr=ddp_t.LR, weight_decay=0.01,
                       max_grad_norm=DDP_MAX_NORM)
    opt.init_master_from_buffer(params)
    ddp = NativeZeroDDP(model, params, grads, n, spec, comm, rank, opt)

    norms, coefs = [], []
    for step in range(ddp_t.STEPS):
        for micro in range(ddp_t.N_ACC):
            if micro == ddp_t.N_ACC - 1:
                ddp.begin_sync_microbatch()
            loss = ddp_t.loss_fn(model, ddp_t.make_batch(rank, step, micro))
            (loss / ddp_t.N_ACC).backward()
        ddp.finish_step(grad_scale=1.0 / world)
        ddp.zero_grad()
        norms.append(float(opt.grad_norm))
        coefs.append(float(opt.clip_coef))

    torch.save({"params": params[:n].clone(), "norms": norms, "coefs": coefs},
               os.path.join(tmpdir, f"p_{rank}.pt"))
    teardown_worker()


def test_native_ddp_clip_matches_adamw_oracle_ws2():
    world = 2
    tmpdir = run_distributed(_worker_ddp_clip, world, timeout=180)
    res = [torch.load(os.path.join(tmpdir, f"p_{r}.pt"), weights_only=False)
           for r in range(world)]
    assert torch.equal(res[0]["params"], res[1]["params"])
    assert res[0]["norms"] == res[1]["norms"]

    # oracle: AdamW on rank-averaged accumulated grads + clip_grad_norm_
    model = ddp_t.make_model()
    opt = torch.optim.AdamW(model.parameters(), lr=ddp_t.LR,
                            betas=(0.9, 0.95), eps=1e-8, weight_decay=0.01)
    norms = []
    for step in range(ddp_t.STEPS):
        opt.zero_grad()
        for rank in range(world):
            for micro in range(ddp_t.N_ACC):
                loss = ddp_t.loss_fn(model,
                                     ddp_t.make_batch(rank, step, micro))
                (loss / (ddp_t.N_ACC * world)).backward()
        norms.append(float(torch.nn.utils.clip_grad_norm_(
            model.parameters(), DDP_MAX_NORM)))
        opt.step()
    # pre-clip norms 1.1868, 1.2130, 1.2506, 1.2742, 1.0695: steps 1-3 clip
    assert [x > DDP_MAX_NORM for x in norms] == [False, True, True, True,
                                                 False], norms
    assert torch.allclose(torch.tensor(res[0]["norms"]), torch.tensor(norms),
                          rtol=1e-5, atol=0)
    assert [c < 1.0 for c in res[0]["coefs"]] == [x > DDP_MAX_NORM
                                                  for x in norms]
    flat = torch.cat([p.detach().reshape(-1) for p in model.parameters()])
    assert torch.allclose(res[0]["params"], flat, atol=1e-6, rtol=1e-5), \
        (res[0]["params"] - flat).abs().max()


# ------------------------------------------------- ACCO ws2 threaded oracle
ACCO_MAX_NORM = 0.8
D, TARGET = acco_t.D, acco_t.TARGET


def _worker_acco_clip(rank, world, port, tmpdir):
    init_worker(rank, world, port)
    from acco_amd.engine import arena
    from acco_amd.engine.acco import AccoEngine
    from acco_amd.engine.scheduler import LRSchedule
    from acco_amd.engine.sharded_adamw import ShardedAdamW
    from acco_amd.parallel.comm import CommBackend, ShardSpec

    torch.manual_seed(7)          # same init on both ranks
    model = nn.Linear(D, 1, bias=False)
    device = torch.device("cpu")
    spec = ShardSpec.build(D, world, buckets=2, align=2)
    params = arena.flatten_params(model, torch.float32, device,
                                  pad_to=spec.total)
    grads = arena.attach_grad_arena(model, torch.float32, device,
                                    pad_to=spec.total)
    comm = CommBackend(device)
    opt = ShardedAdamW(spec, rank, device, lr=1e-2, betas=(0.9, 0.95),
                       eps=1e-8, weight_decay=0.01)
    sched = LRSchedule(1e-2, 4, TARGET, "cosine")
    batches = acco_t.make_batches(rank)
    bptr = [0]

    def next_batch():
        b = batches[bptr[0] % len(batches)]
        bptr[0] += 1
        return b

    def forward_backward(batch):
        x, y = batch
        loss = ((x @ model.weight.t() - y) ** 2).mean()
        loss.backward()
        return loss.detach()

    eng = AccoEngine(params_arena=params, grads_arena=grads, n_live=D,
                     spec=spec, comm=comm, rank=rank, device=device, opt=opt,
                     sched=sched, forward_backward=forward_backward,
                     next_batch=next_batch, n_grad_accumulation=acco_t.N_ACC,
                     max_grad_norm=ACCO_MAX_NORM)
    opt.init_master_from_buffer(params)
    eng.enable_arena_swap(model, grads)
    eng.trace = []
    eng.train_acco(TARGET, n_warmup_steps=0)

    torch.save({"params": eng.params[:D].clone(), "trace": eng.trace,
                "round_idx": eng.round_idx,
                "count_grad_tot": eng.count_grad_tot,
                "com_log": eng.com_log},
               os.path.join(tmpdir, f"res_{rank}.pt"))
    teardown_worker()


def _oracle_replay_clip(w0, traces, world, max_norm, lr=1e-2):
    """test_acco_oracle.oracle_replay with G/cnt clipped to `max_norm`
    before the AdamW math; also returns each round's pre-clip norm."""
    from acco_amd.engine.scheduler import LRSchedule
    sched = LRSchedule(lr, 4, TARGET, "cosine")
    batches = {r: acco_t.make_batches(r) for r in range(world)}
    ptr = {r: 0 for r in range(world)}

    def take(r):
        b = batches[r][ptr[r] % len(batches[r])]
        ptr[r] += 1
        return b

    P = w0.clone()
    master = P.clone()
    m = torch.zeros(D)
    v = torch.zeros(D)
    step = 0
    count_tot = 0
    accum, buffer, count_local, count_round = {}, {}, {}, {}
    for r in range(world):
        g = acco_t.model_grad(P, take(r))
        accum[r] = g.clone()
        buffer[r] = g.clone()
        count_local[r] = 1
        count_round[r] = 1

    norms = []
    for idx in range(len(traces[0])):
        commit = idx % 2 == 1
        G = sum(buffer[r] for r in range(world))
        cnt = sum(count_round[r] for r in range(world))
        g = G / cnt
        norm = g.norm()
        norms.append(float(norm))
        g = g * torch.clamp(max_norm / (norm + 1e-6), max=1.0)
        newP, newM, newV = acco_t._adamw_math(master, m, v, step, g,
                                              sched.lr())
        if commit:
            master, m, v = newP, newM, newV
            step += 1
            count_tot += cnt
            sched.advance(cnt)
        for r in range(world):
            k_new = traces[r][idx] - count_local[r]
            assert k_new >= 0
            for _ in range(k_new):
                accum[r] = accum[r] + acco_t.model_grad(P, take(r))
            count_local[r] = traces[r][idx]
        P = newP.clone()
        for r in range(world):
            buffer[r] = accum[r].clone()
            count_round[r] = count_local[r]
            if idx % 2 == 0:
                accum[r] = torch.zeros(D)
                count_local[r] = 0
    return P, count_tot, norms


def test_acco_clip_matches_oracle_ws2():
    tmpdir = run_distributed(_worker_acco_clip, 2, timeout=240)
    res = [torch.load(os.path.join(tmpdir, f"res_{r}.pt"),
                      weights_only=False) for r in range(2)]
    assert torch.equal(res[0]["params"], res[1]["params"])
    assert res[0]["round_idx"] == res[1]["round_idx"]
    assert res[0]["count_grad_tot"] >= TARGET

    torch.manual_seed(7)
    w0 = nn.Linear(D, 1, bias=False).weight.detach().view(-1).clone()
    traces = {r: res[r]["trace"] for r in range(2)}
    assert len(traces[0]) == len(traces[1]) == res[0]["round_idx"]

    P, count_tot, norms = _oracle_replay_clip(w0, traces, 2, ACCO_MAX_NORM)
    assert count_tot == res[0]["count_grad_tot"]
    assert torch.allclose(P, res[0]["params"], atol=1e-6, rtol=1e-6), \
        (P, res[0]["params"])
    # both ranks logged the same global norm, the oracle's (the com thread
    # may have run one round more than the compute thread consumed)
    logged = [[e["grad_norm"] for e in res[r]["com_log"]] for r in range(2)]
    assert logged[0][:len(norms)] == logged[1][:len(norms)]
    assert torch.allclose(torch.tensor(logged[0][:len(norms)]),
                          torch.tensor(norms), rtol=1e-5, atol=1e-7)


# --------------------------------------------------- config and trainer
PRESETS = ["acco", "ddp", "dpu", "acco-ft", "ddp-ft", "dpu-ft"]


@pytest.mark.parametrize("preset", PRESETS)
def test_presets_default_to_no_clipping(preset):
    from acco_amd.config import load_config
    cfg = load_config([f"train={preset}"])
    assert cfg.train.max_grad_norm == 0


def test_max_grad_norm_override_parses():
    from acco_amd.config import load_config
    assert load_config(["train.max_grad_norm=0.5"]).train.max_grad_norm == 0.5
    assert load_config(["train.max_grad_norm=null"]).train.max_grad_norm is None


def _run_trainer_clip(rank, world, port, tmpdir, method):
    os.environ.update({"MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port),
                       "RANK": str(rank), "LOCAL_RANK": str(rank),
                       "WORLD_SIZE": str(world)})
    os.chdir(tmpdir)
    from acco_amd.config import load_config
    from acco_amd.data.synthetic import SyntheticCausalLMDataset
    from acco_amd.engine.trainer import DecoupledTrainer
    from acco_amd.models import GPTNeoConfig, GPTNeoForCausalLM

    cfg = load_config([
        f"train={method}", "data=synthetic", "model=gptneo",
        "train.nb_steps_tot=8", "train.batch_size=2", "train.max_length=16",
        "train.use_mixed_precision=false", "train.save=false",
        "train.warmup=2", "train.n_warmup_steps=0",
        "train.dataloader_num_workers=0", "train.comm_buckets=2",
        "train.dataloader_persistent_workers=false",
        "train.max_grad_norm=0.5",
    ])
    torch.manual_seed(42)
    mcfg = GPTNeoConfig(hidden_size=32, num_layers=2, num_heads=2,
                        vocab_size=64, max_position_embeddings=32,
                        window_size=8)
    trainer = DecoupledTrainer(model=GPTNeoForCausalLM(mcfg),
                               train_dataset=SyntheticCausalLMDataset(
                                   32, 16, 64, seed=5 + rank),
                               eval_dataset=None, args=cfg.train,
                               run_name="clip")
    assert trainer.opt.max_grad_norm == 0.5
    trainer.train()
    torch.save({"params": trainer.params[:trainer.n_live].clone()},
               os.path.join(tmpdir, f"p_{rank}.pt"))
    teardown_worker()


def _load_summary_tool():
    spec = importlib.util.spec_from_file_location(
        "com_log_summary", os.path.join(ROOT, "tools", "com_log_summary.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _scalar_tags(tmpdir):
    tags = {}
    for path in glob.glob(os.path.join(tmpdir, "scalars", "clip", "*.jsonl")):
        for line in open(path):
            rec = json.loads(line)
            tags.setdefault(rec["tag"], []).append(rec["value"])
    return tags


@pytest.mark.parametrize("method", ["acco", "ddp"])
def test_trainer_runs_with_max_grad_norm_ws2(method, capsys):
    tmpdir = run_distributed(_run_trainer_clip, 2, args=(method,),
                             timeout=300)
    res = [torch.load(os.path.join(tmpdir, f"p_{r}.pt"), weights_only=False)
           for r in range(2)]
    assert torch.equal(res[0]["params"], res[1]["params"])
    assert torch.isfinite(res[0]["params"]).all()
    norms = _scalar_tags(tmpdir).get("grad_norm/0")
    assert norms and all(x > 0 and x == x for x in norms)
    if method != "acco":
        return
    logs = glob.glob(os.path.join(tmpdir, "com_logs_*.json"))
    assert logs
    rounds = json.load(open(logs[0]))
    assert rounds and all(r["grad_norm"] > 0 and 0 < r["clip_coef"] <= 1
                          for r in rounds)
    capsys.readouterr()
    _load_summary_tool().summarize(logs[0])
    out = capsys.readouterr().out
    assert "grad norm" in out and "clipped rounds=" in out
    assert "total com-round wall time" in out


def test_com_log_summary_without_norm_keys(tmp_path, capsys):
    rounds = [{"round": i, "commit": bool(i % 2), "t": 0.01 * (i + 1),
               "count": 2} for i in range(4)]
    plain = tmp_path / "plain.json"
    plain.write_text(json.dumps(rounds))
    tool = _load_summary_tool()
    tool.summarize(str(plain))
    out = capsys.readouterr().out
    assert "grad norm" not in out and "total com-round wall time" in out

    for i, r in enumerate(rounds):
        r["grad_norm"] = 1.0 + i
        r["clip_coef"] = 1.0 if i < 3 else 0.25
    clipped = tmp_path / "clipped.json"
    clipped.write_text(json.dumps(rounds))
    tool.summarize(str(clipped))
    out = capsys.readouterr().out
    assert "mean=2.5" in out and "p50=3" in out and "max=4" in out
    assert "clipped rounds=25.0%" in out
