"""The CE kernels of ce.hip bit for bit against sha256 prefixes recorded from
the build named in golden/ce_parent.json, i.e. ce.hip and ce_rows.hip before
they were folded onto one row skeleton with two policies.

Inputs come from streaming_ref.ce_inputs and the alignment cases of
test_gpu_ce_rows.py (CPU generators seeded from the case name), so the hashes
do not depend on the device RNG. What is pinned:

  rows      ce_rows_fwd / ce_rows_bwd_ (no atomics): lse, tok_loss and the
            in-place dlogits of every case of ce_cases() and of every
            alignment case.
  shifted   ce_fwd / ce_bwd_dev at V % 8 == 0: lse, dlogits and n_valid.
  shifted, V % 8 != 0: per-row hashes of lse[t] and dlogits[t] are recorded
            for every row and pinned for exactly the rows with
            (t·V) % 8 == 0. The parent read every row as V / 8 vectors from
            the row start plus a tail; the skeleton peels a scalar head of
            (-(t·V)) mod 8 elements first, which is empty on those rows and
            regroups the same elements per thread on every other row. The
            other rows are held by the fp64 limits of test_ce.

The loss sum acc[0] goes through float atomics and is pinned nowhere; test_ce
bounds it. test_shifted_and_rows_agree holds the two policies to each other:
the same rows and targets give the same lse bits through either entry."""

import hashlib
import json
import os

import pytest
import torch

from tests import streaming_ref as sr
from tests.test_gpu_ce_rows import ALIGN_T, ALIGN_V, alignment_inputs

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "ce_parent.json")


def _sha(t):
    raw = t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()
    return hashlib.sha256(raw).hexdigest()[:16]


def _ext():
    from acco_amd import ops
    return ops.hip_ext()


# name -> (inputs, eps, rows passed to the row kernels or None for all)
ROWS_CASES = {sr.ce_case_name(*c): (lambda c=c: sr.ce_inputs(*c), c[1], None)
              for c in sr.ce_cases()}
ROWS_CASES.update({
    "align_V%d_eps%g" % (V, eps):
        (lambda V=V, eps=eps: alignment_inputs(V, eps), eps, ALIGN_T)
    for V in ALIGN_V for eps in sr.CE_EPS})
SHIFTED_WHOLE = {sr.ce_case_name(*c): c for c in sr.ce_cases()
                 if c[0][2] % 8 == 0}
SHIFTED_PER_ROW = {sr.ce_case_name(*c): c for c in sr.ce_cases()
                   if c[0][2] % 8 != 0}


def run_rows(name):
    """lse, tok_loss and in-place dlogits of one ROWS_CASES entry."""
    make, eps, rows = ROWS_CASES[name]
    logits, labels = make()
    V = logits.shape[-1]
    targets = sr.ce_shift(labels).reshape(-1)
    n = targets.numel() if rows is None else rows
    buf = logits.reshape(-1, V)[:n].cuda().contiguous()
    tg = targets[:n].cuda()
    lse = torch.full((n,), float("nan"), device="cuda")
    tok = torch.full((n,), float("nan"), device="cuda")
    scale = torch.tensor([sr.CE_DLOSS / max(int((targets >= 0).sum()), 1)],
                         dtype=torch.float32).cuda()
    _ext().ce_rows_fwd(buf, tg, lse, tok, eps)
    _ext().ce_rows_bwd_(buf, tg, lse, scale, eps)
    return {"lse": lse, "tok_loss": tok, "dlogits": buf}


def run_shifted(case):
    """lse [T], dlogits [T, V] and n_valid of ce_fwd / ce_bwd_dev."""
    shape, eps, var = case
    logits, labels = sr.ce_inputs(shape, eps, var)
    lg, lb = logits.cuda(), labels.cuda()
    acc, lse = _ext().ce_fwd(lg, lb, eps)
    dloss_dev = torch.tensor([sr.CE_DLOSS], device="cuda")
    dlogits = _ext().ce_bwd_dev(lg, lb, lse, acc, dloss_dev, eps)
    return lse, dlogits.view(-1, shape[2]), float(acc[1])


def _per_row(lse, dlogits):
    T = lse.numel()
    return {"lse": [_sha(lse[t:t + 1]) for t in range(T)],
            "dlogits": [_sha(dlogits[t]) for t in range(T)]}


def collect():
    """The content of golden/ce_parent.json's "cases" from the loaded build."""
    out = {"rows": {}, "shifted": {}, "shifted_per_row": {}}
    for name in ROWS_CASES:
        out["rows"][name] = {k: _sha(v) for k, v in run_rows(name).items()}
    for name, case in SHIFTED_WHOLE.items():
        lse, dlogits, n_valid = run_shifted(case)
        out["shifted"][name] = {"lse": _sha(lse), "dlogits": _sha(dlogits),
                                "n_valid": n_valid}
    for name, case in SHIFTED_PER_ROW.items():
        lse, dlogits, n_valid = run_shifted(case)
        out["shifted_per_row"][name] = dict(_per_row(lse, dlogits),
                                            n_valid=n_valid)
    return out


def _gold(section, name):
    with open(GOLDEN) as f:
        return json.load(f)["cases"][section][name]


@pytest.mark.parametrize("name", list(ROWS_CASES))
def test_rows_match_parent(name):
    got = {k: _sha(v) for k, v in run_rows(name).items()}
    assert got == _gold("rows", name)


@pytest.mark.parametrize("name", list(SHIFTED_WHOLE))
def test_shifted_matches_parent(name):
    lse, dlogits, n_valid = run_shifted(SHIFTED_WHOLE[name])
    assert {"lse": _sha(lse), "dlogits": _sha(dlogits),
            "n_valid": n_valid} == _gold("shifted", name)


@pytest.mark.parametrize("name", list(SHIFTED_PER_ROW))
def test_shifted_odd_V_matches_parent_on_aligned_rows(name):
    case = SHIFTED_PER_ROW[name]
    B, S_, V = case[0]
    lse, dlogits, n_valid = run_shifted(case)
    gold = _gold("shifted_per_row", name)
    got = _per_row(lse, dlogits)
    pinned = [t for t in range(B * S_) if (t * V) % 8 == 0]
    assert pinned and len(gold["lse"]) == len(gold["dlogits"]) == B * S_
    assert n_valid == gold["n_valid"]
    for key in ("lse", "dlogits"):
        assert ([got[key][t] for t in pinned]
                == [gold[key][t] for t in pinned]), key


@pytest.mark.parametrize("case", [((3, 2741, 72), 0.1, "n2"),
                                  ((2, 33, 1031), 0.1, "n2")],
                         ids=lambda c: sr.ce_case_name(*c))
def test_shifted_and_rows_agree(case):
    """One skeleton: ce_fwd and ce_rows_fwd give the same lse bits."""
    shape, eps, var = case
    logits, labels = sr.ce_inputs(shape, eps, var)
    T, V = shape[0] * shape[1], shape[2]
    lg = logits.cuda()
    _, lse = _ext().ce_fwd(lg, labels.cuda(), eps)
    lse_rows = torch.full((T,), float("nan"), device="cuda")
    tok = torch.empty(T, device="cuda")
    _ext().ce_rows_fwd(lg.view(T, V), sr.ce_shift(labels).reshape(-1).cuda(),
                       lse_rows, tok, eps)
    assert lse.any()
    assert torch.equal(lse, lse_rows)
