"""The streaming kernels (gelu_new, SwiGLU, RoPE, shifted CE, fused AdamW,
colsum, gemm_nt) against fp64 references, at the shapes where they can go
wrong: grid-stride loops on their second trip, tails, single-chunk rows,
every buffer-type instantiation, empty inputs; and every argument check of
their bindings.

bf16 outputs must lie within (0.5 + S) ulp (+ a derived cancellation floor)
of the fp64 reference, fp32 outputs within 8x the fp32 torch reference's own
error; both rules, the floors, the references and the case lists live in
streaming_ref.py, and test_streaming_ref.py holds the fp32 torch formulas to
the same criterion on the CPU. Inputs come from a CPU generator seeded from
the case name; the extension entry points are called directly, so a case
pins the kernel and not the dispatch. References are evaluated on the CPU,
where the self-test validated them."""

import functools
import math

import pytest
import torch

from tests import streaming_ref as sr

pytestmark = pytest.mark.gpu


def _ext():
    from acco_amd import ops
    return ops.hip_ext()


def _assert_half_ulp(what, got, ref64, floor=0.0):
    ratio, idx = sr.within_half_ulp(got.cpu(), ref64, floor)
    print(f"RATIO {what} {ratio:.4f}")
    assert ratio <= 1.0, (
        f"{what}: err/limit {ratio:.4f} at flat index {idx}: got "
        f"{got.flatten()[idx].item()!r}, want {ref64.flatten()[idx].item()!r}")


def _assert_fp32(what, got, ref64, tol):
    err = float((got.cpu().double() - ref64).abs().max()) if ref64.numel() \
        else 0.0
    print(f"FP32 {what} err {err:.3e} tol {tol:.3e}")
    assert got.dtype == torch.float32
    assert err <= tol, f"{what}: max abs err {err:.3e} > tol {tol:.3e}"


def _still_alive():
    """After an empty call: the stream holds no launch error."""
    torch.cuda.synchronize()
    assert float((torch.ones(4, device="cuda") + 1).sum()) == 8.0


# ------------------------------------------------------------- gelu_new
@functools.lru_cache(maxsize=None)
def _sweep():
    x = sr.all_bf16_patterns()
    return x, sr.gelu_floors(x[torch.isfinite(x)])


def test_gelu_fwd_every_bf16_value():
    x, (floor, _) = _sweep()
    out = _ext().gelu_fwd(x.cuda()).cpu()
    ok = torch.isfinite(x)
    _assert_half_ulp("gelu_fwd sweep", out[ok], sr.gelu64(x[ok]), floor)


@pytest.mark.parametrize("dout", sr.GELU_DOUT)
def test_gelu_bwd_every_bf16_value(dout):
    """|x| <= 2^60 only: beyond it x^2 overflows fp32 and 0·inf follows, in
    the kernel and in the fp32 reference alike."""
    x, (_, floor) = _sweep()
    d = torch.full_like(x, dout)
    dx = _ext().gelu_bwd(d.cuda(), x.cuda()).cpu()
    ok = torch.isfinite(x) & (x.float().abs() <= sr.GELU_BWD_MAX)
    _assert_half_ulp(f"gelu_bwd sweep dout={dout}", dx[ok],
                     d[ok].double() * sr.gelu_grad64(x[ok]),
                     floor * abs(float(d[0, 0])))


def test_gelu_second_grid_stride_trip():
    g = sr.case_generator("gelu_stride")
    x = (torch.randn(*sr.STRIDE_SHAPE, generator=g) * 3).bfloat16()
    d = (torch.randn(*sr.STRIDE_SHAPE, generator=g) * 3).bfloat16()
    assert x.numel() // 8 > 2048 * 256
    f_fwd, f_bwd = sr.gelu_floors(x)
    ext = _ext()
    _assert_half_ulp("gelu_fwd stride", ext.gelu_fwd(x.cuda()), sr.gelu64(x),
                     f_fwd)
    _assert_half_ulp("gelu_bwd stride", ext.gelu_bwd(d.cuda(), x.cuda()),
                     d.double() * sr.gelu_grad64(x), f_bwd * d.double().abs())


# --------------------------------------------------------------- SwiGLU
def _check_swiglu(what, g, u, dout, out, dg, du):
    dg64, du64 = sr.swiglu64(g, u, dout)
    _assert_half_ulp(f"swiglu out {what}", out, sr.swiglu64(g, u),
                     sr.swiglu_flush_floor(g, u))
    _assert_half_ulp(f"swiglu dg {what}", dg, dg64,
                     sr.swiglu_dg_floor(dout, u))
    _assert_half_ulp(f"swiglu du {what}", du, du64,
                     sr.swiglu_flush_floor(g, dout))


@pytest.mark.parametrize("dout", sr.SWIGLU_DOUT)
@pytest.mark.parametrize("u", sr.SWIGLU_U)
def test_swiglu_every_bf16_gate(u, dout):
    """|g| <= 2^100 so that no product overflows."""
    g = sr.all_bf16_patterns()
    uu, dd = torch.full_like(g, u), torch.full_like(g, dout)
    ext = _ext()
    out = ext.swiglu_fwd(g.cuda(), uu.cuda()).cpu()
    dg, du = (t.cpu() for t in ext.swiglu_bwd(dd.cuda(), g.cuda(), uu.cuda()))
    ok = torch.isfinite(g) & (g.float().abs() <= sr.SWIGLU_G_MAX)
    _check_swiglu(f"sweep u={u} dout={dout}", g[ok], uu[ok], dd[ok], out[ok],
                  dg[ok], du[ok])


def test_swiglu_second_grid_stride_trip():
    gen = sr.case_generator("swiglu_stride")
    g, u, d = ((torch.randn(*sr.STRIDE_SHAPE, generator=gen) * 3).bfloat16()
               for _ in range(3))
    ext = _ext()
    out = ext.swiglu_fwd(g.cuda(), u.cuda())
    dg, du = ext.swiglu_bwd(d.cuda(), g.cuda(), u.cuda())
    _check_swiglu("stride", g, u, d, out, dg, du)


@pytest.mark.parametrize("rows,two_i", sr.SWIGLU_PACKED_SHAPES)
def test_swiglu_packed(rows, two_i):
    """[5, 16]: one vec8 per row; [37, 528]: 33 per row, odd;
    [2304, 4096]: second grid-stride trip. dgu is compared whole, so both
    halves must be written and nothing else."""
    gen = sr.case_generator(f"swiglu_packed_{rows}_{two_i}")
    I = two_i // 2
    gu = (torch.randn(rows, two_i, generator=gen) * 3).bfloat16()
    d = (torch.randn(rows, I, generator=gen) * 3).bfloat16()
    ext = _ext()
    out = ext.swiglu_packed_fwd(gu.cuda())
    dgu = ext.swiglu_packed_bwd(d.cuda(), gu.cuda())
    assert out.shape == (rows, I) and dgu.shape == gu.shape
    _check_swiglu(f"packed {rows}x{two_i}", gu[:, :I], gu[:, I:], d, out,
                  dgu[:, :I], dgu[:, I:])


# ----------------------------------------------------------------- RoPE
@pytest.mark.parametrize("bwd", [False, True])
@pytest.mark.parametrize("shape", sr.ROPE_SHAPES)
def test_rope(shape, bwd):
    """Tables five rows longer than S; B = 2 makes s = tok % S matter; odd
    H; D = 8 (one item per head); the last shape passes the grid cap."""
    from acco_amd.ops import torch_ref
    B, S_, H, D = shape
    gen = sr.case_generator("rope_%d_%d_%d_%d" % shape)
    x = torch.randn(B, S_, H, D, generator=gen).bfloat16()
    cos, sin = torch_ref.rope_cos_sin(S_ + sr.ROPE_TABLE_EXTRA, D, 10000.0,
                                      "cpu")
    y = _ext().rope_fwd(x.cuda(), cos.cuda(), sin.cuda(), bwd)
    _assert_half_ulp(f"rope {shape} bwd={bwd}", y,
                     sr.rope64(x, cos, sin, bwd), sr.rope_floor(x))


# ------------------------------------------------------------------- CE
_CE_CASES = sr.ce_cases()


@pytest.mark.parametrize("shape,eps,var", _CE_CASES,
                         ids=[sr.ce_case_name(*c) for c in _CE_CASES])
def test_ce(shape, eps, var):
    """lse, loss and the whole dlogits of ce_fwd / ce_bwd / ce_bwd_dev."""
    B, S_, V = shape
    logits, labels = sr.ce_inputs(shape, eps, var)
    t = sr.ce_tolerances(logits, labels, eps)
    what = sr.ce_case_name(shape, eps, var)
    ext = _ext()
    lg, lb = logits.cuda(), labels.cuda()
    acc, lse = ext.ce_fwd(lg, lb, eps)
    dloss_dev = torch.tensor([sr.CE_DLOSS], device="cuda")
    dlogits = ext.ce_bwd_dev(lg, lb, lse, acc, dloss_dev, eps)
    dlogits_host = ext.ce_bwd(lg, lb, lse, acc, sr.CE_DLOSS, eps)
    acc2, lse2 = ext.ce_fwd(lg, lb, eps)
    dlogits2 = ext.ce_bwd_dev(lg, lb, lse2, acc2, dloss_dev, eps)

    assert float(acc[1]) == t["n_valid"]
    loss = (acc[0] / acc[1].clamp(min=1.0)).reshape(1)
    _assert_fp32(f"ce lse {what}", lse.view(B, S_), t["lse"], t["tol_lse"])
    _assert_fp32(f"ce loss {what}", loss, t["loss"].reshape(1), t["tol_loss"])
    _assert_half_ulp(f"ce dlogits {what}", dlogits, t["dlogits"],
                     t["dlogits_floor"])
    # ignored tokens and each sequence's last position
    dead = (sr.ce_shift(labels) < 0)
    assert dead[:, -1].all()
    assert not lse.view(B, S_).cpu()[dead].any()
    assert not dlogits.cpu()[dead].any()
    assert not torch.isnan(dlogits).any() and not torch.isnan(lse).any()
    if t["n_valid"] == 0:
        assert float(loss) == 0.0 and not dlogits.any()
    # only the loss goes through atomics; host and device dloss agree
    assert torch.equal(lse, lse2) and torch.equal(dlogits, dlogits2)
    assert torch.equal(dlogits_host, dlogits)


@pytest.mark.parametrize("V", [72, 2057])
def test_ce_out_of_range_label_is_ignored(V):
    """A label outside [0, V) is an ignored token, as -100 is: lse 0, a zero
    dlogits row, not counted, and never used as an index."""
    eps = 0.1
    g = sr.case_generator("ce_bad_label_%d" % V)
    logits = (torch.randn(1, 5, V, generator=g) * 2.0).bfloat16().cuda()
    valid = int(torch.randint(0, V, (1,), generator=g))
    bad = torch.tensor([[0, V, 2 ** 40, -(2 ** 40), valid]]).cuda()
    ignored = torch.tensor([[0, -100, -100, -100, valid]]).cuda()
    ext = _ext()
    dloss_dev = torch.tensor([sr.CE_DLOSS], device="cuda")

    def run(labels):
        acc, lse = ext.ce_fwd(logits, labels, eps)
        return lse, acc[1], ext.ce_bwd_dev(logits, labels, lse, acc,
                                           dloss_dev, eps)

    lse, n_valid, dlogits = run(bad)
    for got, want in zip((lse, n_valid, dlogits), run(ignored)):
        assert torch.equal(got, want)
    assert float(n_valid) == 1.0
    assert not lse[:3].any() and not dlogits[0, :3].any()
    assert float(lse[3]) != 0.0 and dlogits[0, 3].any()


def test_causal_lm_loss_takes_logits_off_16_bytes():
    """ops.causal_lm_loss on a contiguous view that starts one bf16 element
    into its buffer (the bindings reject it, the autograd function copies
    it): the gradient of its aligned clone bit for bit; the loss, summed
    with atomics, within tol_loss of the clone's."""
    from acco_amd import ops
    B, S_, V = 2, 5, 72
    logits, labels = sr.ce_inputs((B, S_, V), 0.0, "n2")
    tol = sr.ce_tolerances(logits, labels, 0.0)["tol_loss"]
    buf = torch.zeros(B * S_ * V + 1, device="cuda", dtype=torch.bfloat16)
    buf[1:] = logits.flatten().cuda()
    off = buf[1:].view(B, S_, V).requires_grad_(True)
    aligned = off.detach().clone().requires_grad_(True)
    assert off.is_contiguous() and off.data_ptr() % 16 == 2
    assert aligned.data_ptr() % 16 == 0
    lb = labels.cuda()
    loss_off = ops.causal_lm_loss(off, lb)
    loss_off.backward()
    loss = ops.causal_lm_loss(aligned, lb)
    loss.backward()
    assert off.grad.any() and torch.equal(off.grad, aligned.grad)
    assert abs(float(loss_off.detach()) - float(loss.detach())) <= tol


# ---------------------------------------------------------------- AdamW
_ADAMW_CASES = sr.adamw_cases()
_DT = {"bf16": torch.bfloat16, "fp32": torch.float32}


@functools.lru_cache(maxsize=2)
def _adamw_pool(n, gdt):
    return sr.adamw_pool(n, _DT[gdt])


@pytest.mark.parametrize(
    "n,bufs,prm", _ADAMW_CASES,
    ids=["%d_%s_%s_%s_step%d_wd%g" % (n, *b, *p) for n, b, p in _ADAMW_CASES])
def test_fused_adamw(n, bufs, prm):
    """n = 6 291 859 = 4·(3·524288 + 100) + 3: two two-chunk trips for 100
    threads, the single-chunk loop for the rest, a 3-element tail."""
    from acco_amd import ops
    (gdt, odt), (kind, step, wd) = bufs, prm
    pool = _adamw_pool(n, gdt)
    hyper = sr.ADAMW_HYPER
    scale32 = float(torch.tensor(sr.ADAMW_SCALE, dtype=torch.float32))
    ref = sr.adamw64(*pool, scale32, step, wd, **hyper)
    tols = [sr.fp32_tol(a, b) for a, b in
            zip(sr.adamw32(*pool, sr.ADAMW_SCALE, step, wd, **hyper), ref)]
    scale = (torch.tensor([sr.ADAMW_SCALE], device="cuda") if kind == "dev"
             else sr.ADAMW_SCALE)

    def state():
        return [t[:n].clone().cuda() for t in pool]

    def step_(p, m, v, g, out, commit):
        ops.fused_adamw_step(p, g, m, v, step, hyper["lr"], hyper["beta1"],
                             hyper["beta2"], hyper["eps"], wd,
                             grad_scale=scale, out_bf16=out, commit=commit)

    p, m, v, g = state()
    out = None if odt == "none" else torch.empty(n, device="cuda",
                                                 dtype=_DT[odt])
    step_(p, m, v, g, out, True)
    what = f"adamw n={n} {gdt}/{odt} {kind} step={step} wd={wd}"
    for name, got, r, tol in zip("pmv", (p, m, v), ref, tols):
        _assert_fp32(f"{what} {name}", got, r[:n], tol)
    if out is None:
        return
    assert torch.equal(out, p.to(out.dtype))
    # the tentative step from the same state: same out, state untouched
    p2, m2, v2, g2 = state()
    out_t = torch.empty_like(out)
    step_(p2, m2, v2, g2, out_t, False)
    assert torch.equal(out_t, out)
    for got, t0 in zip((p2, m2, v2), pool):
        assert torch.equal(got.cpu(), t0[:n])


# --------------------------------------------------------------- colsum
@pytest.mark.parametrize("P,D,dt", sr.COLSUM_CASES)
def test_colsum(P, D, dt):
    x = sr.colsum_input(P, D, dt)
    got = _ext().colsum(x.cuda())
    ref = sr.colsum64(x)
    assert got.shape == (D,)
    _assert_fp32(f"colsum {P}x{D} {dt}", got, ref,
                 sr.fp32_tol(sr.colsum32(x), ref))
    if P == 0:
        assert not got.any()
        _still_alive()


# -------------------------------------------------------------- gemm_nt
@pytest.mark.parametrize("M,N,K", sr.GEMM_SHAPES)
def test_gemm_nt(M, N, K):
    """(256, 384, 192): 6 tiles, so the XCD remap has a remainder, and 3
    k-steps, so the double buffer wraps; (1024, 1152, 128): 72 tiles."""
    A, B = sr.gemm_inputs(M, N, K)
    C = _ext().gemm_nt(A.cuda(), B.cuda())
    assert C.shape == (M, N)
    _assert_half_ulp(f"gemm {M}x{N}x{K}", C, sr.gemm64(A, B),
                     sr.gemm_floor(A, B))


# --------------------------------------------------------- empty inputs
def _bf16(*shape):
    return torch.zeros(*shape, device="cuda", dtype=torch.bfloat16)


def _f32(*shape):
    return torch.zeros(*shape, device="cuda")


def _empty_gelu(ext):
    x = _bf16(0, 512)
    return [ext.gelu_fwd(x), ext.gelu_bwd(x, x)]


def _empty_swiglu(ext):
    g, gu = _bf16(3, 0, 64), _bf16(0, 16)
    return [ext.swiglu_fwd(g, g), *ext.swiglu_bwd(g, g, g),
            ext.swiglu_packed_fwd(gu), ext.swiglu_packed_bwd(_bf16(0, 8), gu)]


def _empty_rope(ext):
    outs = []
    for shape in [(0, 7, 1, 8), (2, 0, 3, 64)]:
        outs.append(ext.rope_fwd(_bf16(*shape), _f32(12, shape[3]),
                                 _f32(12, shape[3]), False))
    qkv = _bf16(0, 7, 64)
    ext.rope_packed(qkv, qkv, _f32(7, 16), _f32(7, 16), 16, 2, 16, True)
    return outs


def _empty_adamw(ext):
    from acco_amd import ops
    p = _f32(0)
    ops.fused_adamw_step(p, _bf16(0), p.clone(), p.clone(), 0, 1e-3, 0.9,
                         0.95, 1e-8, 0.1)
    return [p]


def _empty_ce(ext):
    logits = _bf16(0, 5, 8)
    labels = torch.zeros(0, 5, device="cuda", dtype=torch.long)
    acc, lse = ext.ce_fwd(logits, labels, 0.1)
    assert acc.shape == (2,) and not acc.any()
    assert float(acc[0] / acc[1].clamp(min=1.0)) == 0.0
    one = torch.ones(1, device="cuda")
    return [lse, ext.ce_bwd(logits, labels, lse, acc, 1.0, 0.1),
            ext.ce_bwd_dev(logits, labels, lse, acc, one, 0.1)]


def _empty_gemm(ext):
    c = ext.gemm_nt(_bf16(0, 64), _bf16(128, 64))
    z = ext.gemm_nt(_bf16(128, 0), _bf16(128, 0))
    assert c.shape == (0, 128) and z.shape == (128, 128) and not z.any()
    return [c]


EMPTY = {"gelu": _empty_gelu, "swiglu": _empty_swiglu, "rope": _empty_rope,
         "adamw": _empty_adamw, "ce": _empty_ce, "gemm": _empty_gemm}


@pytest.mark.parametrize("name", list(EMPTY))
def test_empty_input(name):
    for out in EMPTY[name](_ext()):
        assert out.numel() == 0
    _still_alive()


# ------------------------------------------------------------ rejection
def _adamw(**kw):
    """fused_adamw with valid arguments except those given."""
    def call(ext):
        n = 8
        a = dict(p=_f32(n), g=_bf16(n), m=_f32(n), v=_f32(n), step=0,
                 scale_dev=_f32(0), out=_bf16(n))
        a.update({k: f() for k, f in kw.items()})
        return ext.fused_adamw(a["p"], a["g"], a["m"], a["v"], a["step"],
                               1e-3, 0.9, 0.95, 1e-8, 0.1, 1.0,
                               a["scale_dev"], a["out"], True)
    return call


def _ce_call(entry="ce_bwd", V=16, **kw):
    def call(ext):
        B, S_ = 2, 4
        a = dict(logits=_bf16(B, S_, V),
                 labels=torch.zeros(B, S_, device="cuda", dtype=torch.long),
                 lse=_f32(B * S_), acc=torch.ones(2, device="cuda"))
        a.update({k: f() for k, f in kw.items()})
        if entry == "ce_fwd":
            return ext.ce_fwd(a["logits"], a["labels"], 0.0)
        if entry == "ce_bwd":
            return ext.ce_bwd(a["logits"], a["labels"], a["lse"], a["acc"],
                              1.0, 0.0)
        return ext.ce_bwd_dev(a["logits"], a["labels"], a["lse"], a["acc"],
                              kw.get("dloss", lambda: _f32(1))(), 0.0)
    return call


def _rope_call(cos=(9, 16), sin=(9, 16), table_dev="cuda",
               table_dtype=torch.float32):
    def call(ext):
        c = torch.zeros(*cos, device=table_dev, dtype=table_dtype)
        s = torch.zeros(*sin, device=table_dev, dtype=table_dtype)
        return ext.rope_fwd(_bf16(1, 8, 2, 16), c, s, False)
    return call


def _rope_packed(dst=(1, 8, 64), off=16, Hsec=2, D=16, cos=(8, 16),
                 table_dev="cuda"):
    def call(ext):
        c = torch.zeros(*cos, device=table_dev)
        return ext.rope_packed(_bf16(1, 8, 64), _bf16(*dst), c, c.clone(),
                               off, Hsec, D, False)
    return call


_labels32 = lambda: torch.zeros(2, 4, device="cuda", dtype=torch.int32)
_labels = lambda *shape: torch.zeros(*shape, device="cuda", dtype=torch.long)
# contiguous [2, 4, 16] starting one bf16 element into its buffer
_logits_off_one = lambda: _bf16(2 * 4 * 16 + 1)[1:].view(2, 4, 16)

REJECTED = {
    "adamw_m_fp64": _adamw(m=lambda: _f32(8).double()),
    "adamw_v_short": _adamw(v=lambda: _f32(7)),
    "adamw_m_on_cpu": _adamw(m=lambda: torch.zeros(8)),
    "adamw_v_strided": _adamw(v=lambda: _f32(16)[::2]),
    "adamw_g_on_cpu": _adamw(g=lambda: torch.zeros(8).bfloat16()),
    "adamw_out_on_cpu": _adamw(out=lambda: torch.zeros(8).bfloat16()),
    "adamw_scale_dev_two": _adamw(scale_dev=lambda: _f32(2)),
    "adamw_scale_dev_on_cpu": _adamw(scale_dev=lambda: torch.ones(1)),
    "adamw_step_negative": _adamw(step=lambda: -1),
    "adamw_p_off_16_bytes": _adamw(p=lambda: _f32(9)[1:]),
    "adamw_m_off_16_bytes": _adamw(m=lambda: _f32(9)[1:]),
    "adamw_g_off_8_bytes": _adamw(g=lambda: _bf16(9)[1:]),
    "adamw_g_fp32_off_16_bytes": _adamw(g=lambda: _f32(10)[2:],
                                        out=lambda: _f32(8)),
    "adamw_out_off_8_bytes": _adamw(out=lambda: _bf16(10)[2:]),
    "swiglu_fwd_u_other_sizes":
        lambda ext: ext.swiglu_fwd(_bf16(8, 8), _bf16(4, 16)),
    "swiglu_fwd_u_on_cpu":
        lambda ext: ext.swiglu_fwd(_bf16(8, 8), _bf16(8, 8).cpu()),
    "swiglu_fwd_last_dim_12":
        lambda ext: ext.swiglu_fwd(_bf16(2, 12), _bf16(2, 12)),
    "swiglu_bwd_dout_other_sizes":
        lambda ext: ext.swiglu_bwd(_bf16(4, 16), _bf16(8, 8), _bf16(8, 8)),
    "swiglu_bwd_dout_short":
        lambda ext: ext.swiglu_bwd(_bf16(7, 8), _bf16(8, 8), _bf16(8, 8)),
    "swiglu_bwd_last_dim_12":
        lambda ext: ext.swiglu_bwd(_bf16(2, 12), _bf16(2, 12), _bf16(2, 12)),
    "swiglu_packed_fwd_last_dim_24":
        lambda ext: ext.swiglu_packed_fwd(_bf16(2, 24)),
    "swiglu_packed_bwd_dout_like_gu":
        lambda ext: ext.swiglu_packed_bwd(_bf16(4, 32), _bf16(4, 32)),
    "swiglu_packed_bwd_last_dim_24":
        lambda ext: ext.swiglu_packed_bwd(_bf16(2, 12), _bf16(2, 24)),
    "gelu_fwd_scalar":
        lambda ext: ext.gelu_fwd(_bf16(())),
    "gelu_fwd_12_elements":
        lambda ext: ext.gelu_fwd(_bf16(12)),
    "gelu_bwd_dout_short":
        lambda ext: ext.gelu_bwd(_bf16(1, 8), _bf16(2, 8)),
    "gelu_bwd_dout_other_sizes":
        lambda ext: ext.gelu_bwd(_bf16(16), _bf16(2, 8)),
    "gelu_bwd_dout_on_cpu":
        lambda ext: ext.gelu_bwd(_bf16(2, 8).cpu(), _bf16(2, 8)),
    "rope_fwd_tables_on_cpu": _rope_call(table_dev="cpu"),
    "rope_fwd_tables_fp64": _rope_call(table_dtype=torch.float64),
    "rope_fwd_cos_short": _rope_call(cos=(7, 16), sin=(7, 16)),
    "rope_fwd_sin_other_sizes": _rope_call(sin=(8, 16)),
    "rope_fwd_tables_flat": _rope_call(cos=(144,), sin=(144,)),
    "rope_packed_dst_other_sizes": _rope_packed(dst=(1, 8, 32)),
    "rope_packed_off_negative": _rope_packed(off=-16),
    "rope_packed_off_2": _rope_packed(off=2),
    "rope_packed_section_past_W": _rope_packed(off=48),
    "rope_packed_D_12": _rope_packed(D=12, Hsec=1, cos=(8, 12)),
    "rope_packed_Hsec_0": _rope_packed(Hsec=0),
    "rope_packed_cos_short": _rope_packed(cos=(7, 16)),
    "rope_packed_tables_on_cpu": _rope_packed(table_dev="cpu"),
    "ce_fwd_labels_int32": _ce_call("ce_fwd", labels=_labels32),
    "ce_fwd_labels_other_S": _ce_call("ce_fwd", labels=lambda: _labels(2, 5)),
    "ce_fwd_labels_flat": _ce_call("ce_fwd", labels=lambda: _labels(8)),
    "ce_fwd_labels_on_cpu":
        _ce_call("ce_fwd", labels=lambda: _labels(2, 4).cpu()),
    "ce_fwd_labels_transposed":
        _ce_call("ce_fwd", labels=lambda: _labels(4, 2).t()),
    "ce_fwd_V_0": _ce_call("ce_fwd", V=0),
    "ce_fwd_logits_off_16_bytes": _ce_call("ce_fwd", logits=_logits_off_one),
    "ce_bwd_logits_off_16_bytes": _ce_call("ce_bwd", logits=_logits_off_one),
    "ce_bwd_dev_logits_off_16_bytes":
        _ce_call("ce_bwd_dev", logits=_logits_off_one),
    "ce_bwd_labels_other_S": _ce_call("ce_bwd", labels=lambda: _labels(2, 3)),
    "ce_bwd_labels_int32": _ce_call("ce_bwd", labels=_labels32),
    "ce_bwd_lse_short": _ce_call("ce_bwd", lse=lambda: _f32(7)),
    "ce_bwd_lse_fp64": _ce_call("ce_bwd", lse=lambda: _f32(8).double()),
    "ce_bwd_lse_on_cpu": _ce_call("ce_bwd", lse=lambda: torch.zeros(8)),
    "ce_bwd_acc_one_element": _ce_call("ce_bwd", acc=lambda: _f32(1)),
    "ce_bwd_acc_on_cpu": _ce_call("ce_bwd", acc=lambda: torch.ones(2)),
    "ce_bwd_acc_fp64": _ce_call("ce_bwd", acc=lambda: _f32(2).double()),
    "ce_bwd_dev_labels_flat":
        _ce_call("ce_bwd_dev", labels=lambda: _labels(8)),
    "ce_bwd_dev_lse_short": _ce_call("ce_bwd_dev", lse=lambda: _f32(7)),
    "ce_bwd_dev_acc_one_element": _ce_call("ce_bwd_dev", acc=lambda: _f32(1)),
    "ce_bwd_dev_dloss_on_cpu":
        _ce_call("ce_bwd_dev", dloss=lambda: torch.ones(1)),
    "gemm_nt_A_3d":
        lambda ext: ext.gemm_nt(_bf16(128, 64, 1), _bf16(128, 64)),
    "gemm_nt_B_3d":
        lambda ext: ext.gemm_nt(_bf16(128, 64), _bf16(128, 64, 1)),
}


@pytest.mark.parametrize("name", list(REJECTED))
def test_streaming_binding_rejects(name):
    with pytest.raises(RuntimeError):
        REJECTED[name](_ext())
    torch.cuda.synchronize()        # nothing was launched, nothing faulted
