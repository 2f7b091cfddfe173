"""The acceptance criterion of the streaming-kernel tests, checked without a
GPU: every fp32 torch formula, rounded to bf16, must pass
`within_half_ulp` against the fp64 reference with the recorded slack
S_FP32 and the recorded floors, over the case lists the GPU tests use.
Loosening the slack, a floor or a reference makes one of these fail or
stops them from biting (test_criterion_rejects_*).

Shrunk against the GPU lists (same data distribution, fewer elements, the
sizes only matter to the kernels' grid-stride loops): the elementwise
stride shape [9, 1024, 512] -> [1, 1024, 512], packed SwiGLU
[2304, 4096] -> [256, 4096], RoPE (2, 2048, 17, 64) -> (2, 256, 17, 64).
"""

import math

import pytest
import torch

from tests import streaming_ref as sr


def _check(got_bf16, ref64, floor=0.0, what=""):
    ratio, idx = sr.within_half_ulp(got_bf16, ref64, floor, s=sr.S_FP32)
    print(f"RATIO32 {what} {ratio:.4f}")
    assert ratio <= 1.0, (what, ratio, idx)


def test_slack_is_four_times_measured_and_capped():
    assert sr.S == 4 * sr.S_FP32 and sr.S <= 2.0 ** -6


def test_ulp_bf16():
    r = torch.tensor([1.0, 1.99, 2.0, -3.0, 0.0, 2.0 ** -130, 0.75],
                     dtype=torch.float64)
    want = torch.tensor([2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -6,
                         2.0 ** -133, 2.0 ** -133, 2.0 ** -8],
                        dtype=torch.float64)
    assert torch.equal(sr.ulp_bf16(r), want)


def test_criterion_rejects_wrong_neighbour_nan_and_tiny():
    ref = torch.tensor([1.0 + 2.0 ** -10, 3.0, 2.0 ** -125],
                       dtype=torch.float64)
    good = torch.tensor([1.0, 3.0, 0.0]).bfloat16()
    assert sr.within_half_ulp(good, ref)[0] <= 1.0
    # the bf16 neighbour on the far side of the reference
    bad = good.clone()
    bad[0] = 1.0 + 2.0 ** -7
    ratio, idx = sr.within_half_ulp(bad, ref)
    assert ratio > 1.0 and idx == 0
    nan = good.clone()
    nan[1] = math.nan
    ratio, idx = sr.within_half_ulp(nan, ref)
    assert ratio > 1.0 and idx == 1
    big = good.clone()
    big[2] = 2.0 ** -100
    ratio, idx = sr.within_half_ulp(big, ref)
    assert ratio > 1.0 and idx == 2


def test_criterion_rejects_half_wrong_probabilities():
    """What the old atol=1e-3 let through: every non-label CE gradient
    entry wrong by 50 %, or the smoothing term dropped."""
    shape, eps = (2, 33, 1031), 0.1
    logits, labels = sr.ce_inputs(shape, eps, "n2")
    t = sr.ce_tolerances(logits, labels, eps)
    lab = sr.ce_shift(labels).clamp(min=0)[..., None]
    half = t["dlogits"] * 0.5
    half.scatter_(2, lab, t["dlogits"].gather(2, lab))
    assert sr.within_half_ulp(half.bfloat16(), t["dlogits"],
                              t["dlogits_floor"])[0] > 1.0
    scale = sr.CE_DLOSS / t["n_valid"]
    valid = (sr.ce_shift(labels) >= 0)[..., None]
    no_uni = t["dlogits"] + valid * scale * eps / shape[2]
    assert sr.within_half_ulp(no_uni.bfloat16(), t["dlogits"],
                              t["dlogits_floor"])[0] > 1.0
    assert torch.allclose(no_uni.float(), t["dlogits"].float(), atol=1e-3)


def _gelu_inputs():
    x = sr.all_bf16_patterns()
    yield "sweep", x[torch.isfinite(x)]
    g = sr.case_generator("gelu_stride")
    yield "stride", (torch.randn(1, 1024, 512, generator=g) * 3).bfloat16()


@pytest.mark.parametrize("dout", sr.GELU_DOUT)
def test_gelu_fp32_formula_meets_criterion(dout):
    for name, x in _gelu_inputs():
        f_fwd, f_bwd = sr.gelu_floors(x)
        print(f"FLOOR gelu {name} fwd {f_fwd:.3e} bwd {f_bwd:.3e}")
        # the floors are the fp32 cancellation of 1 + tanh(u): about
        # |x|·2^-24 at x ~ -5, and never more than a few of those
        assert f_fwd <= 4 * 8 * 2.0 ** -24 and f_bwd <= 4 * 32 * 2.0 ** -24
        _check(sr.gelu32(x).bfloat16(), sr.gelu64(x), f_fwd, f"gelu fwd {name}")
        xb = x[x.float().abs() <= sr.GELU_BWD_MAX]
        d = torch.full_like(xb, dout)
        got = (d.float() * sr.gelu_grad32(xb)).bfloat16()
        _check(got, d.double() * sr.gelu_grad64(xb), f_bwd * abs(float(d[0])),
               f"gelu bwd {name}")


def _swiglu_inputs():
    x = sr.all_bf16_patterns()
    x = x[torch.isfinite(x) & (x.float().abs() <= sr.SWIGLU_G_MAX)]
    for u in sr.SWIGLU_U:
        for dout in sr.SWIGLU_DOUT:
            yield f"sweep u={u} dout={dout}", x, torch.full_like(x, u), \
                torch.full_like(x, dout)
    g = sr.case_generator("swiglu_stride")
    r = [(torch.randn(1, 1024, 512, generator=g) * 3).bfloat16()
         for _ in range(3)]
    yield "stride", r[0], r[1], r[2]
    for rows, two_i in [(5, 16), (37, 528), (256, 4096)]:
        g = sr.case_generator(f"swiglu_packed_{rows}_{two_i}")
        gu = (torch.randn(rows, two_i, generator=g) * 3).bfloat16()
        d = (torch.randn(rows, two_i // 2, generator=g) * 3).bfloat16()
        yield f"packed {rows}x{two_i}", gu[:, :two_i // 2], \
            gu[:, two_i // 2:], d


def test_swiglu_fp32_formula_meets_criterion():
    for name, g, u, dout in _swiglu_inputs():
        _check(sr.swiglu32(g, u).bfloat16(), sr.swiglu64(g, u),
               sr.swiglu_flush_floor(g, u), f"swiglu out {name}")
        dg32, du32 = sr.swiglu32(g, u, dout)
        dg64, du64 = sr.swiglu64(g, u, dout)
        _check(dg32.bfloat16(), dg64, sr.swiglu_dg_floor(dout, u),
               f"swiglu dg {name}")
        _check(du32.bfloat16(), du64, sr.swiglu_flush_floor(g, dout),
               f"swiglu du {name}")


@pytest.mark.parametrize("shape", sr.ROPE_SHAPES[:3] + [(2, 256, 17, 64)])
@pytest.mark.parametrize("bwd", [False, True])
def test_rope_fp32_formula_meets_criterion(shape, bwd):
    from acco_amd.ops import torch_ref
    B, S_, H, D = shape
    g = sr.case_generator("rope_%d_%d_%d_%d" % shape)
    x = torch.randn(B, S_, H, D, generator=g).bfloat16()
    cos, sin = torch_ref.rope_cos_sin(S_ + sr.ROPE_TABLE_EXTRA, D, 10000.0,
                                      "cpu")
    _check(sr.rope32(x, cos, sin, bwd).bfloat16(), sr.rope64(x, cos, sin, bwd),
           sr.rope_floor(x), f"rope {shape} bwd={bwd}")


@pytest.mark.parametrize("shape,eps,var", sr.ce_cases(),
                         ids=[sr.ce_case_name(*c) for c in sr.ce_cases()])
def test_ce_fp32_formula_meets_criterion(shape, eps, var):
    logits, labels = sr.ce_inputs(shape, eps, var)
    t = sr.ce_tolerances(logits, labels, eps)
    print(f"TOL ce {shape} eps={eps} {var} lse {t['tol_lse']:.3e} "
          f"loss {t['tol_loss']:.3e} "
          f"largest floor {float(t['dlogits_floor'].max()):.3e}")
    # the fp32 reference is itself accurate: a few ulp of |lse|
    lse_mag = max(float(t["lse"].abs().max()), 1.0)
    assert t["tol_lse"] <= sr.FP32_MARGIN * 4 * 2.0 ** -24 * lse_mag
    _check(t["dlogits32"], t["dlogits"], t["dlogits_floor"],
           f"ce dlogits {shape} eps={eps} {var}")
    # the forced labels of ce_inputs are where the issue wants them
    B, S_, V = shape
    if shape != sr.CE_ALL_IGNORED and S_ >= 5:
        forced = set(labels[0, 1:5].tolist())
        assert {0, V - 1} <= forced
        assert V < 8 or 8 * (V // 8) - 1 in forced
        assert V % 8 == 0 or 8 * (V // 8) in forced
    assert int(labels.max()) < V
    if S_ == 1 or shape == sr.CE_ALL_IGNORED:
        assert t["n_valid"] == 0 and float(t["loss"]) == 0.0
        assert not t["dlogits"].any()
    if var == "neginf":
        assert torch.isinf(logits).any()
        assert torch.isfinite(t["lse"]).all()
        assert torch.isfinite(t["dlogits"]).all()


@pytest.mark.parametrize("n", sr.ADAMW_N)
def test_adamw_fp32_reference_error(n):
    """The fp32 reference against fp64: the tolerances the GPU test derives
    stay at a few fp32 ulp of the values."""
    for gdt in (torch.bfloat16, torch.float32):
        p, m, v, g = sr.adamw_pool(n, gdt)
        assert p.numel() == max(n, sr.ADAMW_POOL)
        for kind, step, wd in sr.ADAMW_PARAMS:
            ref = sr.adamw64(p, m, v, g, float(torch.tensor(sr.ADAMW_SCALE)),
                             step, wd, **sr.ADAMW_HYPER)
            got = sr.adamw32(p, m, v, g, sr.ADAMW_SCALE, step, wd,
                             **sr.ADAMW_HYPER)
            tols = [sr.fp32_tol(a, b) for a, b in zip(got, ref)]
            print(f"TOL adamw n={n} step={step} wd={wd} p {tols[0]:.3e} "
                  f"m {tols[1]:.3e} v {tols[2]:.3e}")
            for tol, r in zip(tols, ref):
                assert tol <= sr.FP32_MARGIN * 4 * 2.0 ** -24 * \
                    max(float(r.abs().max()), 2.0 ** -20)


@pytest.mark.parametrize("P,D,dt", sr.COLSUM_CASES)
def test_colsum_fp32_reference_error(P, D, dt):
    x = sr.colsum_input(P, D, dt)
    ref = sr.colsum64(x)
    tol = sr.fp32_tol(sr.colsum32(x), ref)
    print(f"TOL colsum {P}x{D} {dt} {tol:.3e}")
    assert ref.shape == (D,)
    assert tol <= sr.FP32_MARGIN * max(P, 1) * 2.0 ** -24 * \
        max(float(x.double().abs().sum(0).max()) if P else 0.0, 1.0)


@pytest.mark.parametrize("M,N,K", sr.GEMM_SHAPES)
def test_gemm_fp32_formula_meets_criterion(M, N, K):
    A, B = sr.gemm_inputs(M, N, K)
    _check(sr.gemm32(A, B).bfloat16(), sr.gemm64(A, B), sr.gemm_floor(A, B),
           f"gemm {M}x{N}x{K}")
