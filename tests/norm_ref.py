"""fp64 references, fp32 formulas, case lists and the acceptance criterion of
the RMSNorm / LayerNorm kernels (norms.hip), shared by
test_gpu_norm_kernels.py (the kernels) and test_norm_ref.py (the criterion
itself, on the CPU). The half-ulp rule, its slack S_FP32 / S, `fp32_tol` and
the case generator are those of streaming_ref.py.

Every reference is computed from the kernel's own inputs upcast to float64:
    fwd  s = bf16(x + res) when fused; the statistics and y come from the
         ROUNDED s, as in the kernels. Outputs y, mean, rstd.
    bwd  takes mean and rstd as fp32 inputs (the tests pass the fp64
         statistics rounded to fp32, so the backward is pinned without the
         forward) and upcasts those same values. Outputs dx (+ dadd), dw, db.
`norm32_*` are the same quantities in fp32 torch ops, written in the
decomposition of the comment above `bwd_sums` in norms.hip; they carry the
criterion on the CPU and take a `mutant` that test_norm_ref.py uses to show
what the criterion rejects.

Floors are absolute error terms of fp32 cancellation: a coefficient times
2^-24 times the sum of the absolute values of the terms that are added
(`fwd_terms`, `bwd_terms`), with xhat = (s - mean)·r (Rms: s·r), r = rstd:
    y    |xhat·w| + |b|, and for LayerNorm r·|w|·mean|s|: the row mean is
         itself a sum, off by a few 2^-24·mean|s|, and that error reaches
         every y of the row whatever its xhat (a row at 64 +- 4 has
         r·mean|s| = 16; without the term the fp32 formula needs a
         coefficient of 11141 there, where xhat·w + b cancels, and 2.03 on
         randn; with it, 0.957)
    dx   r·(|dy·w| + |m1| + |xhat·m2|) + r·(mean|dy·w| + |xhat|·mean|dy·w·xhat|)
         + |dadd|; m1 = mean(dy·w) (LayerNorm only), m2 = mean(dy·w·xhat),
         the second bracket being the error of the two row means
    dw   sum over rows of |dy·xhat|;   db   sum over rows of |dy|
The coefficients are measured on the fp32 formulas: the smallest power of two
with which every case below passes `within_half_ulp(..., s=S_FP32)` on the
CPU (test_norm_ref.py prints the largest coefficient any element needs as
COEF lines); the kernels get 4x that, the rule of the slack.
    largest coefficient needed: y rms 0 (three roundings, no sum), ln 0.957
    (offset rows); dx rms 1.231, ln 1.131 (outlier rows); dw rms 0.828,
    ln 0.775 (zero / constant rows); db 0, so it takes dw's, the same sum
    -> Y_COEF = 1, DX_COEF = 2, DW_COEF = 1 (kernels 4, 8, 4)
    worst err/limit at S_FP32 with these: y 0.9981, dx 0.9980, dw 0.9981,
    db 0.9980; mean and rstd at most 0.125 of their tolerance
On every randn case the kernel floor stays below one bf16 ulp of the
reference on at least 99 % of the elements (asserted on the CPU), so a floor
cannot swallow a wrong result.

fp32 outputs (mean, rstd): tolerance = 8x the larger of the fp32 formula's
largest error against fp64 on the same inputs and one fp32 ulp of the largest
|reference| (a constant row makes the former exactly zero by accident).

Domain: the sum of x^2 over a row must stay below 2^127 (it is an fp32
accumulator in the kernels and in the fp32 formulas alike); the `large` kind
uses |x| ~ 2^40, not more.
"""

import math

import torch

from tests.streaming_ref import (FP32_MARGIN, S, S_FP32,  # noqa: F401
                                 case_generator, fp32_tol, ulp_bf16,
                                 within_half_ulp)

# measured coefficients of the fp32 formulas (see the docstring); the
# kernels get KERNEL_FLOOR times these
Y_COEF = 1.0
DX_COEF = 2.0
DW_COEF = 1.0        # dw and db: the same column sum over rows
KERNEL_FLOOR = 4.0

# D -> what it selects (fwd grouping G / chunk count CH; bwd kernel and CH)
#   8     G=4, one vector per row (63 idle lanes); wave-per-row bwd CH=1
#   264   G=4, 33 vectors, D % 32 = 8 (ragged last finalize block); wr CH=1
#   512   G=4 full (64 vectors); last wr CH=1
#   520   G=2, first past G=4; wr CH=2 with one live vector in chunk 2
#   1024  G=2 full (128 vectors); last wave-per-row width
#   1032  G=1 CH=1, first past G=2; first block-per-row bwd (CH=1)
#   2048  G=1 CH=1 full (256 vectors)
#   2056  CH=2 with one live vector in the last chunk, fwd and bwd
#   4104  CH=4 with one live vector in the last chunk
#   8200  CH=8 with one live vector in the last chunk
#   16384 CH=8 full, the widest the bindings accept
DIMS = [8, 264, 512, 520, 1024, 1032, 2048, 2056, 4104, 8200, 16384]
WR_MAX_D = 1024
EXCLUDED_GOLDEN = [("rms", 2048, 8195), ("ln", 256, 4099), ("ln", 768, 8195),
                   ("ln", 2048, 8195)]
EDGE_DIMS = [264, 520, 1032, 2056]       # one per backward instantiation
EDGE_ROWS = 37
KINDS = ["offset", "outlier", "tiny", "large", "rows", "w_signed"]
CPU_MAX_ROWS = 515


def rows_for(D):
    # 1, 3, 5: row groups / waves without a live row
    rows = [1, 3, 5]
    if D <= WR_MAX_D:
        # 98 and 128 partial rows: the finalize's unrolled trip taken by some
        # row slots only, and by all; 4099: three waves take a second row
        rows += [389, 509, 4099]
    else:
        # 101 partial rows; 1027: three blocks take a second row
        rows += [101, 1027]
    if D in (8, 520, 1032):
        rows.append(8195)       # past the forward grid cap under G=4, 2, 1
    return rows


def case_name(family, D, R, fused, kind="randn", eps=1e-5):
    return "%s_%d_%d_%s_%s_eps%g" % (family, D, R, "add" if fused else "plain",
                                     kind, eps)


def cases():
    """(family, D, R, fused, kind, eps) of every case."""
    out = []
    for fam in ("rms", "ln"):
        for D in DIMS:
            for R in rows_for(D):
                for fused in (False, True):
                    out.append((fam, D, R, fused, "randn", 1e-5))
        # the shapes test_gpu_norm_golden.py leaves out, fused
        for f2, D, R in EXCLUDED_GOLDEN:
            if f2 == fam:
                out.append((fam, D, R, True, "randn", 1e-5))
        for kind in KINDS:
            for D in EDGE_DIMS:
                for fused in (False, True):
                    for eps in (1e-5, 1e-6):
                        out.append((fam, D, EDGE_ROWS, fused, kind, eps))
    return out


def cpu_cases():
    """cases() with 8195 and 4099 rows shrunk to 515 (same distribution;
    the row count past the grid caps only matters to the kernels' loops)."""
    seen, out = set(), []
    for fam, D, R, fused, kind, eps in cases():
        c = (fam, D, min(R, CPU_MAX_ROWS), fused, kind, eps)
        if c not in seen:
            seen.add(c)
            out.append(c)
    return out


def norm_inputs(family, D, R, fused, kind="randn", eps=1e-5):
    """dict of bf16 CPU tensors x, dy [R, D], w, b [D], res, dadd ([R, D], or
    None when not fused)."""
    g = case_generator(case_name(family, D, R, fused, kind, eps))

    def rn(*shape):
        return torch.randn(*shape, generator=g)

    x, dy, res, dadd = rn(R, D), rn(R, D), rn(R, D), rn(R, D)
    w, b = 1.0 + 0.1 * rn(D), 0.1 * rn(D)
    if kind == "offset":
        x = 64.0 + 4.0 * x
    elif kind == "outlier":
        x[:, (5 * D) // 8 + 3] = 3e4
    elif kind == "tiny":
        x, res = x * 1e-12, res * 1e-12
    elif kind == "large":
        x, res = x * 2.0 ** 40, res * 2.0 ** 40
    elif kind == "rows":
        x[0], x[1] = 0.0, 3.0
        res[:2] = 0.0
    elif kind == "w_signed":
        w = rn(D)
        w[::7] = 0.0
        assert (w < 0).any()
    else:
        assert kind == "randn", kind
    t = dict(x=x, dy=dy, w=w, b=b, res=res if fused else None,
             dadd=dadd if fused else None)
    return {k: None if v is None else v.bfloat16() for k, v in t.items()}


# ----------------------------------------------------------- the formulas
MUTANTS = ["var_over_d_minus_1", "no_eps", "no_mean_dyw", "no_bias_at_col",
           "dw_without_last_row", "stats_of_unrounded_sum"]
MUTANT_BIAS = 0.02      # the bias is dropped at the column nearest to this


def _fwd(dt, family, x, res, w, b, eps, mutant=None):
    """s (bf16, None when res is None), y, mean (None for rms), rstd, and
    what was normalised, all but s in dtype dt."""
    D = x.shape[-1]
    s, sf = None, x.to(dt)
    if res is not None:
        exact = sf + res.to(dt)
        s = exact.float().bfloat16()
        sf = exact if mutant == "stats_of_unrounded_sum" else s.to(dt)
    n = D - 1 if mutant == "var_over_d_minus_1" else D
    e = 0.0 if mutant == "no_eps" else eps
    w = w.to(dt)
    if family == "ln":
        mean = sf.sum(-1) / D
        d = sf - mean[:, None]
        rstd = torch.rsqrt((d * d).sum(-1) / n + e)
        bias = b.to(dt).clone()
        if mutant == "no_bias_at_col":
            bias[(bias.abs() - MUTANT_BIAS).abs().argmin()] = 0.0
        y = d * rstd[:, None] * w + bias
    else:
        mean = None
        rstd = torch.rsqrt((sf * sf).sum(-1) / n + e)
        y = sf * rstd[:, None] * w
    return dict(s=s, y=y, mean=mean, rstd=rstd, sf=sf)


def _bwd(dt, family, dy, x, w, mean, rstd, dadd, mutant=None):
    """dx, dw, db (None for rms) in dtype dt; mean / rstd as the kernels get
    them (fp32 [R])."""
    D = x.shape[-1]
    dy, x, w = dy.to(dt), x.to(dt), w.to(dt)
    r = rstd.to(dt)[:, None]
    db = None
    if family == "ln":
        xhat = (x - mean.to(dt)[:, None]) * r
        dyw = dy * w
        m1 = dyw.sum(-1, keepdim=True) / D
        if mutant == "no_mean_dyw":
            m1 = torch.zeros_like(m1)
        m2 = (dyw * xhat).sum(-1, keepdim=True) / D
        dx = r * (dyw - m1 - xhat * m2)
        g = dy * xhat
        db = dy.sum(0)
    else:
        coef = r * r * r * (dy * w * x).sum(-1, keepdim=True) / D
        dx = r * dy * w - x * coef
        g = dy * x * r
    if dadd is not None:
        dx = dx + dadd.to(dt)
    if mutant == "dw_without_last_row":
        g = g[:-1]
    return dict(dx=dx, dw=g.sum(0), db=db)


def norm64_fwd(family, x, res, w, b, eps):
    return _fwd(torch.float64, family, x, res, w, b, eps)


def norm32_fwd(family, x, res, w, b, eps, mutant=None):
    return _fwd(torch.float32, family, x, res, w, b, eps, mutant)


def norm64_bwd(family, dy, x, w, mean, rstd, dadd):
    return _bwd(torch.float64, family, dy, x, w, mean, rstd, dadd)


def norm32_bwd(family, dy, x, w, mean, rstd, dadd, mutant=None):
    return _bwd(torch.float32, family, dy, x, w, mean, rstd, dadd, mutant)


# ------------------------------------------------------------- the floors
def fwd_terms(family, ref, w, b):
    """2^-24 · the y terms of the docstring, from norm64_fwd's result."""
    sf, r = ref["sf"], ref["rstd"][:, None]
    wa = w.double().abs()
    if family == "ln":
        t = ((sf - ref["mean"][:, None]) * r).abs() * wa + b.double().abs() \
            + r * wa * sf.abs().mean(-1, keepdim=True)
    else:
        t = (sf * r).abs() * wa
    return 2.0 ** -24 * t


def bwd_terms(family, dy, x, w, mean, rstd, dadd):
    """2^-24 · the (dx, dw, db) terms of the docstring; db is None for rms."""
    dy, x, w = dy.double(), x.double(), w.double()
    r = rstd.double()[:, None]
    if family == "ln":
        xhat = (x - mean.double()[:, None]) * r
    else:
        xhat = x * r
    dyw = dy * w
    t2 = dyw * xhat
    t = dyw.abs() + (xhat * t2.mean(-1, keepdim=True)).abs() \
        + xhat.abs() * t2.abs().mean(-1, keepdim=True)
    db = None
    if family == "ln":
        t = t + dyw.mean(-1, keepdim=True).abs() \
            + dyw.abs().mean(-1, keepdim=True)
        db = 2.0 ** -24 * dy.abs().sum(0)
    t = r * t
    if dadd is not None:
        t = t + dadd.double().abs()
    return 2.0 ** -24 * t, 2.0 ** -24 * (dy * xhat).abs().sum(0), db


def needed_coefficient(got, ref64, terms, s=S_FP32):
    """The largest coefficient any element needs to pass with floor
    coefficient·terms (0 when every element passes without a floor)."""
    if ref64.numel() == 0:
        return 0.0
    over = (got.double() - ref64).abs() - (0.5 + s) * ulp_bf16(ref64)
    need = torch.where(over > 0, over / terms.clamp(min=2.0 ** -1000),
                       torch.zeros_like(over))
    return float(need.max())


def floor_below_one_ulp(floor, ref64):
    """Fraction of elements whose floor is under one bf16 ulp of ref."""
    if ref64.numel() == 0:
        return 1.0
    return float((floor < ulp_bf16(ref64)).double().mean())


# ---------------------------------------------------------- fp32 outputs
def stat_tol(val32, ref64):
    """Tolerance of mean / rstd: 8x the larger of the fp32 formula's own
    largest error and one fp32 ulp of the largest |reference|."""
    if ref64.numel() == 0:
        return 0.0
    big = float(ref64.abs().max())
    ulp = 2.0 ** (math.frexp(big)[1] - 24) if big > 0.0 else 0.0
    return max(fp32_tol(val32, ref64), FP32_MARGIN * ulp)


# ------------------------------------------------- everything of one case
def expectation(family, t, eps, formulas32=False):
    """What a case's outputs are held to, from `t` = norm_inputs(...):
    ref (fp64 y, mean, rstd, dx, dw, db and the bf16 s), terms (the floor
    terms of y, dx, dw, db), tol (mean, rstd), the backward's inputs xin,
    mean_in, rstd_in, and with formulas32 the fp32 formulas' outputs."""
    ln = family == "ln"
    f64 = norm64_fwd(family, t["x"], t["res"], t["w"], t["b"], eps)
    f32 = norm32_fwd(family, t["x"], t["res"], t["w"], t["b"], eps)
    xin = t["x"] if t["res"] is None else f64["s"]
    mean_in = f64["mean"].float() if ln else None
    rstd_in = f64["rstd"].float()
    bwd_in = (family, t["dy"], xin, t["w"], mean_in, rstd_in, t["dadd"])
    b64 = norm64_bwd(*bwd_in)
    tdx, tdw, tdb = bwd_terms(*bwd_in)
    keys = ("y", "mean", "rstd", "dx", "dw", "db")
    both = {**f64, **b64}
    out = dict(ref={k: both[k] for k in keys + ("s",)},
               terms=dict(y=fwd_terms(family, f64, t["w"], t["b"]), dx=tdx,
                          dw=tdw, db=tdb),
               tol={k: stat_tol(f32[k], f64[k]) for k in ("mean", "rstd")
                    if f64[k] is not None},
               xin=xin, mean_in=mean_in, rstd_in=rstd_in)
    if formulas32:
        out["got32"] = {**f32, **norm32_bwd(*bwd_in)}
    return out


COEF = dict(y=Y_COEF, dx=DX_COEF, dw=DW_COEF, db=DW_COEF)
