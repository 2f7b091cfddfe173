"""Global gradient-norm clipping on the GPU: the grad_sumsq / sumsq_finalize
kernels against exact and fp64 references at every size where they take
another path, the argument checks of their bindings, and the clipped com
round of the ACCO engine, bit for bit against the fused AdamW given the
engine's own scale tensor.

Inputs come from CPU generators seeded by case name; references are
evaluated on the CPU; the extension entry points are called directly.

Accuracy bound (derived, not measured). All terms x² are non-negative, so a
sum that passes each term through at most k fp32 roundings is off by at most
about k·2^-24 relative. With P partials (blocks) of 256 threads, T = 256·P,
one thread holds at most n/T + VEC + 1 elements, and its elements cannot pass
through more roundings than it holds elements plus the fixed tree (lane 4,
wave 6, block 3, finalize 1): the bound (2·ceil(n/T) + 64)·2^-24 covers it
with room.
"""

import functools
import math

import pytest
import torch

from tests import streaming_ref as sr

pytestmark = pytest.mark.gpu

_DT = {"bf16": torch.bfloat16, "fp32": torch.float32}
_VEC = {"bf16": 8, "fp32": 4}
SIZES = [0, 1, 3, 7, 8, 9, 1027, 4352, 8389413]
U24 = 2.0 ** -24


def _ext():
    from acco_amd import ops
    return ops.hip_ext()


def _grid(n, dt):
    """elementwise_grid over the 16-byte chunks: 256 threads, 2048 cap."""
    chunks = -(-n // _VEC[dt])
    return min(2048, max(1, -(-chunks // 256)))


def _nan(k, device="cuda", dtype=torch.float32):
    return torch.full((k,), math.nan, device=device, dtype=dtype)


def _bound(n, partials):
    return (2 * math.ceil(n / (partials * 256)) + 64) * U24


def _sumsq(g, extra=0):
    """(finalized fp32 scalar, the partials written, count) of g on the GPU;
    workspace and result are NaN before each call."""
    ext = _ext()
    dt = "bf16" if g.dtype == torch.bfloat16 else "fp32"
    want = _grid(g.numel(), dt)
    ws = _nan(want + extra)
    count = ext.grad_sumsq(g, ws)
    assert count == want == ext.grad_sumsq_grid(g.numel(), dt == "bf16")
    assert torch.isnan(ws[count:]).all()        # nothing past the grid
    out = _nan(1)
    ext.sumsq_finalize(ws[:count], out)
    return out, ws[:count].clone(), count


# ------------------------------------------------------------ exact cases
def _exact_input(n, dt):
    """±1 with probability 1/4, else 0; 1 forced at the first 9 and last 9
    elements and on both sides of every multiple of 2048·256·VEC. Every
    partial sum is an integer below 2^24: exact in fp32 in any order."""
    gen = sr.case_generator(f"grad_sumsq_exact_{n}_{dt}")
    r = torch.rand(n, generator=gen)
    x = torch.zeros(n)
    x[r < 0.125] = 1.0
    x[(r >= 0.125) & (r < 0.25)] = -1.0
    trip = 2048 * 256 * _VEC[dt]
    forced = list(range(9)) + list(range(n - 9, n))
    for edge in range(trip, n + 1, trip):
        forced += [edge - 1, edge]
    forced = [i for i in forced if 0 <= i < n]
    if forced:
        x[torch.tensor(forced)] = 1.0
    assert n < 2 ** 24
    return x.to(_DT[dt]), int((x != 0).sum())


@pytest.mark.parametrize("dt", ["bf16", "fp32"])
@pytest.mark.parametrize("n", SIZES)
def test_grad_sumsq_exact(n, dt):
    """n = 8 389 413 = 8·(2·524288 + 100) + 5: two full grid-stride trips
    plus 100 chunks plus a 5-element tail in bf16; four trips plus 201
    chunks plus a 1-element tail in fp32."""
    x, nonzero = _exact_input(n, dt)
    out, partials, count = _sumsq(x.cuda(), extra=3)
    assert float(partials.double().sum()) == nonzero
    assert float(out) == nonzero
    assert out.dtype == torch.float32


# --------------------------------------------------------------- accuracy
@functools.lru_cache(maxsize=None)
def _randn_input(n, dt):
    """Shared by the tests below: clone before changing it."""
    gen = sr.case_generator(f"grad_sumsq_randn_{n}_{dt}")
    return (3.0 * torch.randn(n, generator=gen)).to(_DT[dt])


@pytest.mark.parametrize("dt", ["bf16", "fp32"])
@pytest.mark.parametrize("n", [4352, 8389413])
def test_grad_sumsq_accuracy(n, dt):
    x = _randn_input(n, dt)
    ref = float(x.double().square().sum())
    out, _, count = _sumsq(x.cuda())
    rel = abs(float(out.double()) - ref) / ref
    bound = _bound(n, count)
    print(f"RATIO grad_sumsq n={n} {dt} rel {rel:.3e} bound {bound:.3e} "
          f"ratio {rel / bound:.4f}")
    assert rel <= bound


@pytest.mark.parametrize("dt", ["bf16", "fp32"])
def test_grad_sumsq_deterministic(dt):
    g = _randn_input(8389413, dt).cuda()
    out1, p1, _ = _sumsq(g)
    out2, p2, _ = _sumsq(g)
    assert torch.equal(p1, p2) and torch.equal(out1, out2)


@pytest.mark.parametrize("dt", ["bf16", "fp32"])
@pytest.mark.parametrize("bad", [math.inf, -math.inf, math.nan])
def test_grad_sumsq_non_finite(bad, dt):
    """One inf element gives inf, one NaN gives NaN: nothing is skipped."""
    for n, at in [(4352, 4351), (1027, 1025), (8389413, 4194304)]:
        x = _randn_input(n, dt).clone()
        x[at] = bad
        out, _, _ = _sumsq(x.cuda())
        if math.isnan(bad):
            assert math.isnan(float(out))
        else:
            assert float(out) == math.inf


# ------------------------------------------------------------- rejections
def _bf16(n):
    return torch.ones(n, device="cuda", dtype=torch.bfloat16)


def _f32(n):
    return torch.ones(n, device="cuda")


def _call_sumsq(g=lambda: _bf16(4352), partials=lambda: _nan(3)):
    def call(ext):
        ws = partials()
        try:
            ext.grad_sumsq(g(), ws)
        finally:
            torch.cuda.synchronize()
            if ws.is_floating_point():
                assert torch.isnan(ws).all()    # nothing was written
    return call


def _call_finalize(partials=lambda: _f32(3), out=lambda: _nan(1)):
    def call(ext):
        o = out()
        try:
            ext.sumsq_finalize(partials(), o)
        finally:
            torch.cuda.synchronize()
            assert torch.isnan(o).all()
    return call


REJECTED = {
    "g_on_cpu": _call_sumsq(g=lambda: torch.ones(4352).bfloat16()),
    "g_fp16": _call_sumsq(g=lambda: _f32(4352).half()),
    "g_fp64": _call_sumsq(g=lambda: _f32(4352).double()),
    "g_strided": _call_sumsq(g=lambda: _f32(8704)[::2]),
    "g_bf16_off_16_bytes": _call_sumsq(g=lambda: _bf16(4356)[4:]),
    "g_bf16_off_2_bytes": _call_sumsq(g=lambda: _bf16(4353)[1:]),
    "g_fp32_off_16_bytes": _call_sumsq(g=lambda: _f32(4353)[1:],
                                       partials=lambda: _nan(8)),
    "partials_short": _call_sumsq(partials=lambda: _nan(2)),
    "partials_fp64": _call_sumsq(
        partials=lambda: _nan(3, dtype=torch.float64)),
    "partials_on_cpu": _call_sumsq(partials=lambda: _nan(3, device="cpu")),
    "partials_strided": _call_sumsq(partials=lambda: _nan(6)[::2]),
    "finalize_out_two": _call_finalize(out=lambda: _nan(2)),
    "finalize_out_on_cpu": _call_finalize(out=lambda: _nan(1, device="cpu")),
    "finalize_out_fp64": _call_finalize(
        out=lambda: _nan(1, dtype=torch.float64)),
    "finalize_partials_on_cpu": _call_finalize(partials=lambda: torch.ones(3)),
    "finalize_partials_fp64": _call_finalize(
        partials=lambda: _f32(3).double()),
    "grid_negative_n": lambda ext: ext.grad_sumsq_grid(-1, True),
}


@pytest.mark.parametrize("name", list(REJECTED))
def test_grad_clip_binding_rejects(name):
    with pytest.raises(RuntimeError):
        REJECTED[name](_ext())
    torch.cuda.synchronize()        # nothing was launched, nothing faulted


# ------------------------------------------------- optimizer integration
N_LIVE = 13000          # 3 buckets of 4352: three blocks per bf16 segment
COUNT = 2               # 1/count is exact in fp32
HYPER = dict(lr=1e-3, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.1)
STEP0 = 3


def _round_state():
    """bf16 grads of norm >> 1 (padding zero) and an fp32 p/m/v state."""
    from acco_amd.parallel.comm import ShardSpec
    spec = ShardSpec.build(N_LIVE, 1, buckets=3)
    assert spec.seg == 4352 and spec.total == 13056
    gen = sr.case_generator("grad_clip_round")
    grads = torch.zeros(spec.total)
    grads[:N_LIVE] = 3.0 * torch.randn(N_LIVE, generator=gen)
    p = torch.randn(spec.total, generator=gen)
    m = (torch.rand(spec.total, generator=gen) - 0.5) * 0.02
    v = torch.rand(spec.total, generator=gen) * 0.001
    return spec, grads.bfloat16(), p, m, v


def _engine(max_grad_norm, grad_reduce_dtype=None):
    from acco_amd.engine.acco import AccoEngine
    from acco_amd.engine.scheduler import LRSchedule
    from acco_amd.engine.sharded_adamw import ShardedAdamW
    from acco_amd.parallel.comm import CommBackend
    spec, grads, p, m, v = _round_state()
    device = torch.device("cuda")
    opt = ShardedAdamW(spec, 0, device, **HYPER)
    opt.p.copy_(p)
    opt.m.copy_(m)
    opt.v.copy_(v)
    opt.step_count = STEP0
    arena = torch.zeros(spec.total, dtype=torch.bfloat16, device=device)
    eng = AccoEngine(params_arena=arena, grads_arena=torch.zeros_like(arena),
                     n_live=N_LIVE, spec=spec, comm=CommBackend(device),
                     rank=0, device=device, opt=opt,
                     sched=LRSchedule(1e-3, 10, 1000, "cosine"),
                     forward_backward=None, next_batch=None,
                     grad_reduce_dtype=grad_reduce_dtype,
                     max_grad_norm=max_grad_norm)
    eng.com_buffer.copy_(grads)
    eng.count_grad_this_round.fill_(COUNT)
    return eng, grads


def _manual_round(eng, grads, scale, lr, commit, fp32_reduce):
    """Per-bucket ops.fused_adamw_step from the initial state with `scale`;
    returns (new com buffer, p, m, v)."""
    from acco_amd import ops
    spec, _, p, m, v = _round_state()
    p, m, v = p.cuda(), m.cuda(), v.cuda()
    buf = grads.cuda().float() if fp32_reduce else grads.cuda().clone()
    for j in range(spec.nb):
        seg = spec.seg_view(buf, j, 0)
        ops.fused_adamw_step(
            spec.owned_view(p, j), seg, spec.owned_view(m, j),
            spec.owned_view(v, j), STEP0, lr, *HYPER["betas"], HYPER["eps"],
            HYPER["weight_decay"], grad_scale=scale, out_bf16=seg,
            commit=commit)
    return buf.bfloat16(), p, m, v


@pytest.mark.parametrize("reduce_dtype", [None, "fp32"])
@pytest.mark.parametrize("commit", [False, True])
def test_clipped_round_bitwise(commit, reduce_dtype):
    """The clipped com round equals the fused AdamW given the engine's own
    scale tensor, and that scale is clip_grad_norm_'s in fp64 to the kernel
    bound plus four roundings (sqrt, + eps, the division, one product; the
    products with 1/count = 0.5 are exact)."""
    max_norm = 1.0
    eng, grads = _engine(max_norm, reduce_dtype)
    lr = eng.sched.lr()
    n = eng.communication_round(commit=commit)
    torch.cuda.synchronize()
    assert n == COUNT
    scale = eng.opt.clip_scale
    assert scale.shape == (1,) and scale.dtype == torch.float32

    g64 = grads.double()
    norm64 = math.sqrt(float(g64.square().sum())) / COUNT
    assert norm64 > 100 * max_norm
    coef64 = min(1.0, max_norm / (norm64 + 1e-6))
    scale64 = coef64 / COUNT
    seg_partials = _grid(eng.spec.seg, "fp32" if reduce_dtype else "bf16")
    bound = _bound(eng.spec.seg, seg_partials) + 4 * U24
    rel = abs(float(scale.double()) - scale64) / scale64
    print(f"RATIO clip scale rel {rel:.3e} bound {bound:.3e}")
    assert rel <= bound
    assert abs(float(eng.opt.grad_norm) - norm64) / norm64 <= bound
    assert abs(float(eng.opt.clip_coef) - coef64) / coef64 <= bound
    entry = eng.com_log[-1]
    assert entry["grad_norm"] == float(eng.opt.grad_norm)
    assert entry["clip_coef"] == float(eng.opt.clip_coef)

    buf, p, m, v = _manual_round(eng, grads, scale, lr, commit,
                                 reduce_dtype == "fp32")
    assert torch.equal(eng.com_buffer, buf)
    assert torch.equal(eng.opt.p, p)
    assert torch.equal(eng.opt.m, m)
    assert torch.equal(eng.opt.v, v)
    assert eng.opt.step_count == STEP0 + int(commit)
    if not commit:                  # the tentative round leaves the state
        _, _, p0, m0, v0 = _round_state()
        assert torch.equal(eng.opt.p.cpu(), p0)
        assert torch.equal(eng.opt.m.cpu(), m0)
        assert torch.equal(eng.opt.v.cpu(), v0)


@pytest.mark.parametrize("commit", [False, True])
def test_huge_max_norm_equals_clipping_off(commit):
    on, _ = _engine(1e30)
    off, _ = _engine(None)
    assert on.opt.clipping and not off.opt.clipping
    on.communication_round(commit=commit)
    off.communication_round(commit=commit)
    torch.cuda.synchronize()
    assert float(on.opt.clip_coef) == 1.0
    assert torch.equal(on.com_buffer, off.com_buffer)
    for a, b in [(on.opt.p, off.opt.p), (on.opt.m, off.opt.m),
                 (on.opt.v, off.opt.v)]:
        assert torch.equal(a, b)
    assert "grad_norm" in on.com_log[-1] and "grad_norm" not in off.com_log[-1]


# -------------------------------------------------------------- engine run
def test_acco_engine_single_gpu_clipped():
    """test_gpu_engine.test_acco_engine_single_gpu with max_grad_norm."""
    from acco_amd.engine import arena
    from acco_amd.engine.acco import AccoEngine
    from acco_amd.engine.scheduler import LRSchedule
    from acco_amd.engine.sharded_adamw import ShardedAdamW
    from acco_amd.models import LlamaConfig, LlamaForCausalLM
    from acco_amd.parallel.comm import CommBackend, ShardSpec

    torch.manual_seed(0)
    device = torch.device("cuda")
    cfg = LlamaConfig(hidden_size=256, num_layers=2, num_heads=4,
                      num_kv_heads=2, intermediate_size=512, vocab_size=1024,
                      max_position_embeddings=512)
    model = LlamaForCausalLM(cfg)
    n = arena.live_numel(model)
    spec = ShardSpec.build(n, 1, buckets=4)
    params = arena.flatten_params(model, torch.bfloat16, device,
                                  pad_to=spec.total)
    grads = arena.attach_grad_arena(model, torch.bfloat16, device,
                                    pad_to=spec.total)
    comm = CommBackend(device)
    opt = ShardedAdamW(spec, 0, device, lr=1e-3)
    opt.init_master_from_buffer(params)
    sched = LRSchedule(1e-3, 10, 1000, "cosine")

    ids = torch.randint(0, 1024, (2, 128), device=device)

    def forward_backward(_):
        loss, _l = model(ids, labels=ids)
        loss.backward()
        return loss.detach()

    eng = AccoEngine(params_arena=params, grads_arena=grads, n_live=n,
                     spec=spec, comm=comm, rank=0, device=device, opt=opt,
                     sched=sched, forward_backward=forward_backward,
                     next_batch=lambda: {}, n_grad_accumulation=1,
                     max_grad_norm=0.05)
    p0 = params[:n].clone()
    eng.train_acco(nb_grad_tot=1 << 60, max_rounds=6)
    torch.cuda.synchronize()
    assert eng.round_idx == 6
    assert opt.step_count == 3
    assert torch.isfinite(params[:n].float()).all()
    assert not torch.equal(params[:n], p0)
    assert len(eng.com_log) >= 6
    for entry in eng.com_log:
        assert math.isfinite(entry["grad_norm"]) and entry["grad_norm"] > 0
        assert 0 < entry["clip_coef"] <= 1
