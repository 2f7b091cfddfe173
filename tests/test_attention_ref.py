"""The acceptance criterion of the attention-kernel tests, checked without a
GPU: the fp32 emulation of attention_ref.py (tile-wise online softmax with the
deferred max, P and dS rounded to bf16) must pass the criterion against the
fp64 reference with the slack S_FP32 and the recorded floor coefficients over
every case the GPU tests use; lse must pass the fp32 rule. On the randn cases
the kernels' limit must stay under a quarter of the older tests' tolerance on
99 % of the elements. The census cases are checked against closed forms, and
ten wrong kernels (MUTANTS) go through the older tolerances and through the
new criterion: every mask and every delta mutant must fail the new criterion
on every case where it changes the mask or the row; the table the run prints
(MUTANT lines) is the one in RESULTS.md.
"""

import functools

import pytest
import torch

from tests import attention_ref as ar

CPU_CASES = ar.cpu_cases()
IDS = [ar.case_name(c) for c in CPU_CASES]


@functools.lru_cache(maxsize=None)
def _inputs(c):
    return ar.attn_inputs(c)


@functools.lru_cache(maxsize=None)
def _expect(c):
    return ar.expectation(c, _inputs(c), formulas32=True)


def _ratios(exp, got, s, mult):
    """err/limit of every output of `got` under the criterion."""
    out = {}
    for k in ar.BF16_OUT:
        ref = exp["ref"][k]
        floor = ar.floor_of(exp["terms"][k], k, ref, mult, s)
        out[k] = ar.within(got[k], ref, floor, s=s)[0]
    err = float((got["lse"].double() - exp["ref"]["lse"]).abs().max())
    out["lse"] = err / exp["tol"]["lse"] if err == err else float("inf")
    return out


def _needed(got, ref, terms, s):
    """Largest coefficient of the fp32 term that any element needs."""
    bf, fp = terms
    over = (got.double() - ref).abs() - bf \
        - (0.5 + s) * ar.ulp_bf16(ref.abs() + bf)
    # below 2^-100 both are noise of underflowing P, not a coefficient
    live = (over > 2.0 ** -100) & (fp > 2.0 ** -100)
    need = torch.where(live, over / fp.clamp(min=2.0 ** -100),
                       torch.zeros_like(over))
    return float(need.max())


def test_case_lists():
    names = [ar.case_name(c) for c in ar.cases()]
    assert len(set(names)) == len(names)
    assert ar.KERNEL_FLOOR == 4.0 and ar.BF16_U == 2.0 ** -8
    for c in ar.COEF.values():                # powers of two
        assert torch.frexp(torch.tensor(c))[0] == 0.5
    for sh in ar.SHAPES + ar.WINDOW_SHAPES + ar.KIND_SHAPES:
        assert sh[0] * sh[2] <= 8 and sh[1] <= 1024 and sh[1] % 64 == 0
    for sh, _, _, _ in ar.DOC_BUILDS:
        assert sh[1] % 256 == 0


@pytest.mark.parametrize("case", CPU_CASES, ids=IDS)
def test_attention_fp32_emulation_meets_criterion(case):
    (B, S_, H, Hkv, D), window, scale, kind, starts = case
    t, exp = _inputs(case), _expect(case)
    got, name = exp["got32"], ar.case_name(case)
    for k in ar.BF16_OUT:
        need = _needed(got[k], exp["ref"][k], exp["terms"][k], ar.S_FP32)
        print(f"COEF {k} {name} {need:.4f}")
    ratios = _ratios(exp, got, ar.S_FP32, 1.0)
    for k, r in ratios.items():
        print(f"RATIO32 {k} {name} {r:.4f}")
    assert all(r <= 1.0 for r in ratios.values()), ratios
    if kind == "randn":
        # the cap that keeps the floor honest
        for k in ar.BF16_OUT:
            ref = exp["ref"][k]
            floor = ar.floor_of(exp["terms"][k], k, ref, ar.KERNEL_FLOOR)
            frac = ar.limit_below_quarter_old(k, floor, ref)
            print(f"CAP {k} {name} {frac:.5f}")
            assert frac >= 0.99, (k, frac)
    if kind == "census":
        # closed forms: lse = log(count), o·count = attended keys of class d
        n = ar.census_count(S_, window, t["doc_start"])          # [B|1, S]
        lse = exp["ref"]["lse"]
        assert (lse - n.log()[:, None, :]).abs().max() < 1e-12
        oc = exp["ref"]["o"] * n[:, :, None, None]
        assert (oc - oc.round()).abs().max() < 1e-9
        assert (oc.sum(-1) - n[:, :, None]).abs().max() < 1e-9
    if kind == "do_zero":
        for k in ("dq", "dk", "dv"):
            assert not exp["ref"][k].any() and not got[k].any()
    if window == 1:
        rep = H // Hkv
        v = t["v"].repeat_interleave(rep, dim=2)
        assert torch.equal(exp["ref"]["o"], v.double())


# ------------------------------------------------------------------ mutants
def _mutant_applies(mutant, case, t, exp):
    """Does the mutant change the mask (or the row) of this case?"""
    (B, S_, H, Hkv, D), window, scale, kind, starts = case
    if mutant in ar.MASK_MUTANTS:
        a = ar.attend_mask(S_, window, t["doc_start"], mutant=mutant)
        return not torch.equal(a.expand_as(exp["allow"] | a),
                               exp["allow"].expand_as(exp["allow"] | a))
    if kind == "do_zero":
        return False
    if mutant == "delta_unscaled":
        return scale != 1.0
    return True


def _old_passes(exp, got):
    return all(torch.allclose(got[k].double(), exp["ref"][k],
                              atol=ar.OLD_ATOL[k], rtol=ar.OLD_RTOL)
               for k in ar.BF16_OUT)


@pytest.mark.parametrize("mutant", ar.MUTANTS)
def test_mutants(mutant):
    """MUTANT lines: per mutant, on how many of the cases it applies to the
    older tolerances pass it and the new criterion (the kernels' slack and
    floors) rejects it. Mask and delta mutants must be rejected everywhere."""
    applies = old_pass = new_fail = 0
    missed = []
    for case in CPU_CASES:
        t, exp = _inputs(case), _expect(case)
        if not _mutant_applies(mutant, case, t, exp):
            continue
        applies += 1
        (B, S_, H, Hkv, D), window, scale, kind, starts = case
        q, k, v, ds = t["q"], t["k"], t["v"], t["doc_start"]
        o, lse = ar.attn32_fwd(q, k, v, scale, window, ds, mutant)
        dq, dk, dv = ar.attn32_bwd(q, k, v, t["dO"], exp["lse_in"],
                                   exp["delta_in"], scale, window, ds, mutant)
        got = dict(o=o, lse=lse, dq=dq, dk=dk, dv=dv)
        old_pass += _old_passes(exp, got)
        ratios = _ratios(exp, got, ar.S, ar.KERNEL_FLOOR)
        worst = max(r if r == r else float("inf") for r in ratios.values())
        if worst > 1.0:
            new_fail += 1
        else:
            missed.append((ar.case_name(case), round(worst, 3)))
    print(f"MUTANT {mutant}: applies to {applies} cases, old tolerances pass "
          f"{old_pass}, new criterion rejects {new_fail}; not caught: "
          f"{missed}")
    assert applies > 0
    if mutant in ar.MASK_MUTANTS + ar.DELTA_MUTANTS:
        assert not missed, missed
