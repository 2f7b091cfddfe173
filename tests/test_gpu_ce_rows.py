"""The row-wise CE kernels of the chunked lm_head + loss (ce.hip, Rows
policy: ce_rows_fwd, ce_rows_bwd_) against the fp64 references, tolerances
and case list of streaming_ref.py: every case of ce_cases() (odd V with a
different scalar head per row, more rows than the 8192-block grid, all rows
ignored, large and -inf logits, label smoothing), V around the vector and block
strides with targets on every segment boundary of a misaligned row,
out-of-range targets, bitwise reproducibility, the empty input and every
argument check of both bindings.

The entry points are called directly on [T, V] rows with targets shifted by
sr.ce_shift, so a case pins the kernels and not the dispatch. lse and the
per-token loss are fp32 outputs (tol_lse, tol_loss); the in-place dlogits go
through within_half_ulp with the CE floor at the module's S."""

import functools

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


def _run(rows, targets, eps, scale):
    """(lse, tok_loss, dlogits) of bf16 rows [T, V] and int64 targets [T] on
    the CPU; the rows are copied, the kernel overwrites its own buffer."""
    ext = _ext()
    T = rows.shape[0]
    buf = rows.cuda().contiguous()
    tg = targets.cuda()
    lse = torch.full((T,), float("nan"), device="cuda")
    tok = torch.full((T,), float("nan"), device="cuda")
    ext.ce_rows_fwd(buf, tg, lse, tok, eps)
    assert torch.equal(buf.cpu(), rows)          # the forward only reads
    scale_dev = torch.tensor([scale], device="cuda", dtype=torch.float32)
    ext.ce_rows_bwd_(buf, tg, lse, scale_dev, eps)
    return lse, tok, buf


def _check(what, logits, labels, eps, rows=None):
    """logits [B, S, V], labels [B, S] as streaming_ref builds them; the
    kernels get the first `rows` rows (default all) and their targets."""
    B, S_, V = logits.shape
    t = sr.ce_tolerances(logits, labels, eps)
    tok64 = sr.ce64(logits, labels, eps)[1].reshape(-1)
    targets = sr.ce_shift(labels).reshape(-1)
    n = B * S_ if rows is None else rows
    assert not (targets[n:] >= 0).any()          # only ignored rows dropped
    flat = logits.reshape(-1, V)[:n]
    scale = sr.CE_DLOSS / max(t["n_valid"], 1)
    lse, tok, dlogits = _run(flat, targets[:n], eps, scale)
    lse2, tok2, dlogits2 = _run(flat, targets[:n], eps, scale)

    _assert_fp32(f"ce_rows lse {what}", lse, t["lse"].reshape(-1)[:n],
                 t["tol_lse"])
    _assert_fp32(f"ce_rows tok_loss {what}", tok, tok64[:n], t["tol_loss"])
    _assert_half_ulp(f"ce_rows dlogits {what}", dlogits,
                     t["dlogits"].reshape(-1, V)[:n],
                     t["dlogits_floor"].reshape(-1, V)[:n])
    dead = targets[:n] < 0
    assert not lse.cpu()[dead].any() and not tok.cpu()[dead].any()
    assert not dlogits.cpu()[dead].any()
    assert not torch.isnan(dlogits).any() and not torch.isnan(lse).any()
    assert not torch.isnan(tok).any()
    # no atomics anywhere: the same bits twice
    assert torch.equal(lse, lse2) and torch.equal(tok, tok2)
    assert torch.equal(dlogits, dlogits2)
    return lse, tok, dlogits


_CE_CASES = sr.ce_cases()


@pytest.mark.parametrize("shape,eps,var", _CE_CASES,
                         ids=[sr.ce_case_name(*c) for c in _CE_CASES])
def test_ce_rows(shape, eps, var):
    logits, labels = sr.ce_inputs(shape, eps, var)
    lse, tok, dlogits = _check(sr.ce_case_name(shape, eps, var), logits,
                               labels, eps)
    if shape == sr.CE_ALL_IGNORED or shape[1] == 1:
        assert not lse.any() and not tok.any() and not dlogits.any()


# ---------------------------------------------------- V around the strides
def _peel(t, V):
    return min((-(t * V)) % 8, V)


ALIGN_V = [1, 7, 9, 2055, 2057]
ALIGN_T = 5


def alignment_inputs(V, eps):
    """(logits [1, T + 1, V], labels [1, T + 1]) on the CPU, T = 5 rows of
    odd V: rows 1 to 4 start at four different offsets from a 16-byte
    boundary. Targets on column 0, the last column of the scalar head, the
    first vector column and V - 1, each in a misaligned row. A sixth, ignored
    row carries the shift of streaming_ref's labels and is not passed on."""
    T = ALIGN_T
    g = sr.case_generator("ce_rows_align_%d_%g" % (V, eps))
    logits = (torch.randn(1, T + 1, V, generator=g) * 2.0).bfloat16()
    assert len({(-(t * V)) % 8 for t in range(1, T)}) == 4
    targets = [int(torch.randint(0, V, (1,), generator=g)),
               0,
               max(_peel(2, V) - 1, 0),
               min(_peel(3, V), V - 1),
               V - 1]
    labels = torch.full((1, T + 1), -100)
    labels[0, 1:] = torch.tensor(targets)
    assert sr.ce_shift(labels).reshape(-1).tolist() == targets + [-100]
    return logits, labels


@pytest.mark.parametrize("eps", sr.CE_EPS)
@pytest.mark.parametrize("V", ALIGN_V)
def test_ce_rows_alignment(V, eps):
    logits, labels = alignment_inputs(V, eps)
    _check("align_V%d_eps%g" % (V, eps), logits, labels, eps, rows=ALIGN_T)


# ------------------------------------------------------ out-of-range targets
@pytest.mark.parametrize("bad", ["V", 2 ** 40, -1, -(2 ** 40)])
def test_ce_rows_out_of_range_target_is_ignored(bad):
    V, T = 2057, 4
    bad = V if bad == "V" else bad
    g = sr.case_generator("ce_rows_bad_target")
    rows = (torch.randn(T, V, generator=g) * 2.0).bfloat16()
    targets = torch.tensor([3, bad, V - 1, 0])
    ignored = torch.tensor([3, -100, V - 1, 0])
    got = _run(rows, targets, 0.1, 0.25)
    want = _run(rows, ignored, 0.1, 0.25)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    lse, tok, dlogits = got
    assert float(lse[1]) == 0.0 and float(tok[1]) == 0.0
    assert not dlogits[1].any()
    assert dlogits[0].any() and dlogits[2].any() and dlogits[3].any()


# ---------------------------------------------------------------- empty input
def test_ce_rows_empty():
    ext = _ext()
    buf = torch.empty(0, 72, device="cuda", dtype=torch.bfloat16)
    tg = torch.empty(0, device="cuda", dtype=torch.int64)
    lse = torch.empty(0, device="cuda")
    tok = torch.empty(0, device="cuda")
    ext.ce_rows_fwd(buf, tg, lse, tok, 0.0)
    ext.ce_rows_bwd_(buf, tg, lse, torch.ones(1, device="cuda"), 0.0)
    torch.cuda.synchronize()
    assert float((torch.ones(4, device="cuda") + 1).sum()) == 8.0


# ------------------------------------------------------------ argument checks
_T, _V = 4, 16


def _good():
    return dict(
        logits=torch.zeros(_T, _V, device="cuda", dtype=torch.bfloat16),
        targets=torch.zeros(_T, device="cuda", dtype=torch.int64),
        lse=torch.zeros(_T, device="cuda"),
        tok_loss=torch.zeros(_T, device="cuda"),
        scale_dev=torch.ones(1, device="cuda"))


def _call(entry, **kw):
    a = _good()
    a.update({k: v(a) for k, v in kw.items()})
    ext = _ext()
    if entry == "fwd":
        return ext.ce_rows_fwd(a["logits"], a["targets"], a["lse"],
                               a["tok_loss"], 0.0)
    return ext.ce_rows_bwd_(a["logits"], a["targets"], a["lse"],
                            a["scale_dev"], 0.0)


def _misaligned(a):
    base = torch.zeros(_T * _V + 8, device="cuda", dtype=torch.bfloat16)
    return base[1:1 + _T * _V].view(_T, _V)


_LOGITS_BAD = {
    "logits_fp32": lambda a: a["logits"].float(),
    "logits_on_cpu": lambda a: a["logits"].cpu(),
    "logits_3d": lambda a: a["logits"].view(2, 2, _V),
    "logits_transposed":
        lambda a: torch.zeros(_V, _T, device="cuda",
                              dtype=torch.bfloat16).t(),
    "logits_misaligned": _misaligned,
    "logits_V_0": lambda a: a["logits"][:, :0].contiguous(),
    # 4 GiB of address space, never touched: the check comes before a launch
    "logits_V_2_31":
        lambda a: torch.empty(1, 2 ** 31, device="cuda",
                              dtype=torch.bfloat16),
}
_TARGETS_BAD = {
    "targets_int32": lambda a: a["targets"].int(),
    "targets_short": lambda a: a["targets"][:-1],
    "targets_long": lambda a: torch.zeros(_T + 1, device="cuda",
                                          dtype=torch.int64),
    "targets_on_cpu": lambda a: a["targets"].cpu(),
    "targets_strided":
        lambda a: torch.zeros(2 * _T, device="cuda", dtype=torch.int64)[::2],
}


def _rowvec_bad(name):
    return {
        f"{name}_short": lambda a: a[name][:-1],
        f"{name}_fp64": lambda a: a[name].double(),
        f"{name}_on_cpu": lambda a: a[name].cpu(),
        f"{name}_strided": lambda a: torch.zeros(2 * _T, device="cuda")[::2],
    }


_SCALE_BAD = {
    "scale_dev_on_cpu": lambda a: torch.ones(1),
    "scale_dev_two_elements": lambda a: torch.ones(2, device="cuda"),
    "scale_dev_empty": lambda a: torch.ones(0, device="cuda"),
    "scale_dev_fp64": lambda a: torch.ones(1, device="cuda").double(),
}


def _bad_calls():
    out = {}
    for entry, groups in (
            ("fwd", [("logits", _LOGITS_BAD), ("targets", _TARGETS_BAD),
                     ("lse", _rowvec_bad("lse")),
                     ("tok_loss", _rowvec_bad("tok_loss"))]),
            ("bwd", [("logits", _LOGITS_BAD), ("targets", _TARGETS_BAD),
                     ("lse", _rowvec_bad("lse")),
                     ("scale_dev", _SCALE_BAD)])):
        for arg, bad in groups:
            for name, make in bad.items():
                out[f"ce_rows_{entry}_{name}"] = functools.partial(
                    _call, entry, **{arg: make})
    return out


_BAD = _bad_calls()


@pytest.mark.parametrize("name", list(_BAD))
def test_ce_rows_argument_checks(name):
    _call("fwd")
    _call("bwd")                                  # the good call passes
    with pytest.raises(RuntimeError):
        _BAD[name]()
    torch.cuda.synchronize()
