"""The RMSNorm / LayerNorm kernels against fp64 references at every dispatch
edge: the first width past each G / CH / backward-kernel threshold (one live
vector in the last chunk), one vector per row, widths that are no multiple
of the finalize's 32 columns, partial-row counts on both sides of its
unrolled trip, rows past every grid cap, empty inputs, rows with an offset,
an outlier, tiny and large magnitudes, zero and constant rows, signed and
zero weights, two eps; and every argument check of the bindings.

bf16 outputs must lie within (0.5 + S) ulp (+ a derived cancellation floor)
of the fp64 reference, mean and rstd within the fp32 rule; the rules, the
floors, the references and the case lists live in norm_ref.py, and
test_norm_ref.py holds the fp32 torch formulas to the same criterion on the
CPU. Inputs come from a CPU generator seeded from the case name; the
extension entry points are called directly. The backward gets the fp64
statistics rounded to fp32, not the forward kernel's, so each direction is
pinned alone. References are evaluated on the CPU."""

import pytest
import torch

from tests import norm_ref as nr
from tests.test_gpu_streaming_kernels import (_assert_fp32, _assert_half_ulp,
                                              _ext, _still_alive)

pytestmark = pytest.mark.gpu

CASES = nr.cases()


def _cuda(t):
    return None if t is None else t.cuda()


@pytest.mark.parametrize("case", CASES, ids=[nr.case_name(*c) for c in CASES])
def test_norm_kernels(case):
    family, D, R, fused, kind, eps = case
    name = nr.case_name(*case)
    ext = _ext()
    t = nr.norm_inputs(*case)
    exp = nr.expectation(family, t, eps)
    ref = exp["ref"]
    x, dy, w, b = (t[k].cuda() for k in ("x", "dy", "w", "b"))
    res, dadd = _cuda(t["res"]), _cuda(t["dadd"])

    got = {}
    if family == "rms":
        if fused:
            got["y"], got["s"], got["rstd"] = ext.add_rmsnorm_fwd(x, res, w,
                                                                  eps)
        else:
            got["y"], got["rstd"] = ext.rmsnorm_fwd(x, w, eps)
        got["dx"], got["dw"] = ext.rmsnorm_bwd(
            dy, exp["xin"].cuda(), w, exp["rstd_in"].cuda(), dadd)
    else:
        if fused:
            (got["y"], got["s"], got["mean"],
             got["rstd"]) = ext.add_layernorm_fwd(x, res, w, b, eps)
        else:
            got["y"], got["mean"], got["rstd"] = ext.layernorm_fwd(x, w, b,
                                                                   eps)
        got["dx"], got["dw"], got["db"] = ext.layernorm_bwd(
            dy, exp["xin"].cuda(), w, exp["mean_in"].cuda(),
            exp["rstd_in"].cuda(), dadd)
    got = {k: v.cpu() for k, v in got.items()}

    if fused:
        assert torch.equal(got["s"], ref["s"]), "s is not bf16(x + res)"
    for k in ("y", "dx", "dw", "db"):
        if ref[k] is None:
            continue
        assert got[k].dtype == torch.bfloat16
        assert got[k].shape == ((D,) if k in ("dw", "db") else (R, D))
        _assert_half_ulp(f"{k} {name}", got[k], ref[k],
                         nr.KERNEL_FLOOR * nr.COEF[k] * exp["terms"][k])
    for k, tol in exp["tol"].items():
        assert got[k].shape == (R,)
        _assert_fp32(f"{k} {name}", got[k], ref[k], tol)
    if kind == "rows":
        for v in got.values():
            assert torch.isfinite(v.float()).all()
        if family == "ln":      # zero row and constant row: y is the bias
            assert torch.equal(got["y"][:2], t["b"].expand(2, D))
        else:
            assert not got["y"][0].any()


# ---------------------------------------------------------- empty input
@pytest.mark.parametrize("D", [264, 2056])     # one per backward kernel
@pytest.mark.parametrize("fused", [False, True])
def test_norm_empty_input(D, fused):
    """R = 0: nothing to normalise, dW and dB are sums over no rows."""
    ext = _ext()
    x = torch.empty(0, D, device="cuda", dtype=torch.bfloat16)
    w = torch.ones(D, device="cuda", dtype=torch.bfloat16)
    st = torch.empty(0, device="cuda")
    extra = x.clone() if fused else None
    if fused:
        outs = ext.add_rmsnorm_fwd(x, extra, w, 1e-5)
        outs += ext.add_layernorm_fwd(x, extra, w, w, 1e-5)
        shapes = [(0, D), (0, D), (0,), (0, D), (0, D), (0,), (0,)]
    else:
        outs = ext.rmsnorm_fwd(x, w, 1e-5) + ext.layernorm_fwd(x, w, w, 1e-5)
        shapes = [(0, D), (0,), (0, D), (0,), (0,)]
    assert [tuple(o.shape) for o in outs] == shapes
    _still_alive()
    dx, dw = ext.rmsnorm_bwd(x, x, w, st, extra)
    dx2, dw2, db2 = ext.layernorm_bwd(x, x, w, st, st, extra)
    _still_alive()
    assert dx.shape == dx2.shape == (0, D)
    for d in (dw, dw2, db2):
        assert d.shape == (D,) and d.dtype == torch.bfloat16
        assert not d.any()


# ------------------------------------------------------------ rejection
RJ_R, RJ_D = 5, 16


def _bf16(*shape, device="cuda"):
    return torch.ones(*shape, device=device, dtype=torch.bfloat16)


def _f32(*shape, device="cuda"):
    return torch.ones(*shape, device=device)


ENTRY_ARGS = {
    "rmsnorm_fwd": ("x", "w", "eps"),
    "add_rmsnorm_fwd": ("x", "res", "w", "eps"),
    "rmsnorm_bwd": ("dy", "x", "w", "rstd", "dadd"),
    "layernorm_fwd": ("x", "w", "b", "eps"),
    "add_layernorm_fwd": ("x", "res", "w", "b", "eps"),
    "layernorm_bwd": ("dy", "x", "w", "mean", "rstd", "dadd"),
}
ROW_ARGS = ("x", "res", "dy", "dadd")        # [R, D] bf16
COL_ARGS = ("w", "b")                        # [D] bf16
STAT_ARGS = ("mean", "rstd")                 # [R] fp32


def _norm(entry, **kw):
    """`entry` with valid arguments except those given (as factories)."""
    def call(ext):
        a = {k: _bf16(RJ_R, RJ_D) for k in ROW_ARGS}
        a.update({k: _bf16(RJ_D) for k in COL_ARGS})
        a.update({k: _f32(RJ_R) for k in STAT_ARGS})
        a["eps"] = 1e-5
        a.update({k: f() for k, f in kw.items()})
        return getattr(ext, entry)(*[a[k] for k in ENTRY_ARGS[entry]])
    return call


def _rejected():
    out = {}
    for entry, args in ENTRY_ARGS.items():
        def add(what, **kw):
            out[f"{entry}_{what}"] = _norm(entry, **kw)

        def shaped(D, xD=None, R=RJ_R):
            # every tensor of the call at width D, x at width xD
            kw = {k: (lambda: _bf16(R, D)) for k in ROW_ARGS}
            kw.update({k: (lambda: _bf16(D)) for k in COL_ARGS})
            if xD is not None:
                kw["x"] = lambda: _bf16(R, xD)
            return kw

        add("width_12", **shaped(12))
        add("width_16392", **shaped(16392, R=1))
        add("x_numel_not_rows_of_w", **shaped(24, xD=16))
        add("x_on_cpu", x=lambda: _bf16(RJ_R, RJ_D, device="cpu"))
        add("x_fp32", x=lambda: _f32(RJ_R, RJ_D))
        add("x_not_contiguous", x=lambda: _bf16(RJ_R, 2 * RJ_D)[:, ::2])
        for k in args:
            if k in ROW_ARGS[1:]:
                add(f"{k}_on_cpu", **{k: lambda: _bf16(RJ_R, RJ_D,
                                                       device="cpu")})
                add(f"{k}_fp32", **{k: lambda: _f32(RJ_R, RJ_D)})
                add(f"{k}_not_contiguous",
                    **{k: lambda: _bf16(RJ_R, 2 * RJ_D)[:, ::2]})
                add(f"{k}_short", **{k: lambda: _bf16(RJ_R - 1, RJ_D)})
            elif k in COL_ARGS:
                add(f"{k}_on_cpu", **{k: lambda: _bf16(RJ_D, device="cpu")})
                add(f"{k}_fp32", **{k: lambda: _f32(RJ_D)})
                add(f"{k}_not_contiguous",
                    **{k: lambda: _bf16(2 * RJ_D)[::2]})
                # 8 divides x.numel() too: half rows, were it let through
                add(f"{k}_half_width", **{k: lambda: _bf16(RJ_D // 2)})
                add(f"{k}_too_wide", **{k: lambda: _bf16(RJ_D + 8)})
            elif k in STAT_ARGS:
                add(f"{k}_fp64", **{k: lambda: _f32(RJ_R).double()})
                add(f"{k}_short", **{k: lambda: _f32(RJ_R - 1)})
                add(f"{k}_strided", **{k: lambda: _f32(2 * RJ_R)[::2]})
                add(f"{k}_on_cpu", **{k: lambda: _f32(RJ_R, device="cpu")})
    return out


REJECTED = _rejected()


@pytest.mark.parametrize("entry", list(ENTRY_ARGS))
def test_norm_rejection_baseline_is_accepted(entry):
    """The arguments the rejection cases start from are valid."""
    _norm(entry)(_ext())
    _still_alive()


@pytest.mark.parametrize("name", list(REJECTED))
def test_norm_binding_rejects(name):
    with pytest.raises(RuntimeError):
        REJECTED[name](_ext())
    torch.cuda.synchronize()        # nothing was launched, nothing faulted
