"""The acceptance criterion of the norm-kernel tests, checked without a GPU:
every fp32 torch formula of norm_ref.py, rounded to bf16, must pass
`within_half_ulp` against the fp64 reference with the slack S_FP32 and the
recorded floor coefficients, over the case lists the GPU tests use; mean and
rstd must pass the fp32 rule. On the randn cases the KERNEL floor (4x) must
stay under one bf16 ulp of the reference on 99 % of the elements, and six
wrong formulas that the old allclose tolerances accept must be rejected.

Shrunk against the GPU lists: 8195 and 4099 rows become 515 (same data
distribution; the row counts past the grid caps only matter to the kernels'
grid-stride loops).
"""

import pytest
import torch

from tests import norm_ref as nr
from tests.test_gpu_norm_golden import _tol as old_tol

BF16_KEYS = ("y", "dx", "dw", "db")


def _ratios(exp, got, s, floor_scale):
    """err/limit of every output of `got` under the criterion."""
    out = {}
    for k in BF16_KEYS:
        if exp["ref"][k] is not None:
            floor = floor_scale * nr.COEF[k] * exp["terms"][k]
            out[k] = nr.within_half_ulp(got[k].bfloat16(), exp["ref"][k],
                                        floor, s=s)[0]
    for k, tol in exp["tol"].items():
        err = float((got[k].double() - exp["ref"][k]).abs().max())
        out[k] = err / tol if tol > 0 else (0.0 if err == 0 else float("inf"))
    return out


CPU_CASES = nr.cpu_cases()


def test_case_lists():
    names = [nr.case_name(*c) for c in nr.cases()]
    assert len(set(names)) == len(names)
    for fam, D, R in nr.EXCLUDED_GOLDEN:
        assert (fam, D, R, True, "randn", 1e-5) in nr.cases()
    assert nr.KERNEL_FLOOR == 4.0
    for c in nr.COEF.values():                # powers of two
        assert torch.frexp(torch.tensor(c))[0] == 0.5


@pytest.mark.parametrize("case", CPU_CASES,
                         ids=[nr.case_name(*c) for c in CPU_CASES])
def test_norm_fp32_formulas_meet_criterion(case):
    family, D, R, fused, kind, eps = case
    t = nr.norm_inputs(*case)
    exp = nr.expectation(family, t, eps, formulas32=True)
    got = exp["got32"]
    name = nr.case_name(*case)
    if fused:
        assert torch.equal(got["s"], exp["ref"]["s"])
    for k in BF16_KEYS:
        if exp["ref"][k] is not None:
            need = nr.needed_coefficient(got[k].bfloat16(), exp["ref"][k],
                                         exp["terms"][k])
            print(f"COEF {k} {name} {need:.4f}")
    ratios = _ratios(exp, got, nr.S_FP32, 1.0)
    for k, r in ratios.items():
        print(f"RATIO32 {k} {name} {r:.4f}")
    assert all(r <= 1.0 for r in ratios.values()), ratios
    if kind == "randn":
        for k in BF16_KEYS:
            if exp["ref"][k] is not None:
                floor = nr.KERNEL_FLOOR * nr.COEF[k] * exp["terms"][k]
                frac = nr.floor_below_one_ulp(floor, exp["ref"][k])
                assert frac >= 0.99, (k, frac)
    if kind == "rows":
        assert (exp["ref"]["rstd"][0] - eps ** -0.5).abs() < 1e-9 * eps ** -0.5
        if family == "ln":
            assert torch.equal(exp["ref"]["y"][:2],
                               t["b"].double().expand(2, D))
    if kind == "offset":                     # the rows did not collapse
        assert (exp["xin"].float().std(-1) > 2.0).all()


# (mutant, case, the outputs it must spoil)
MUTANT_CASES = [
    ("var_over_d_minus_1", ("ln", 264, 389, False, "randn", 1e-5), "y rstd"),
    ("var_over_d_minus_1", ("rms", 264, 389, False, "randn", 1e-5), "y rstd"),
    ("no_eps", ("ln", 264, 389, False, "randn", 1e-5), "rstd"),
    ("no_eps", ("rms", 264, 389, False, "randn", 1e-5), "rstd"),
    ("no_mean_dyw", ("ln", 8200, 5, False, "randn", 1e-5), "dx"),
    ("no_bias_at_col", ("ln", 264, 389, False, "randn", 1e-5), "y"),
    # a row's terms are O(1) against atol 0.3 + 5 % of |dW| ~ sqrt(R): the old
    # bound is blind to them only at thousands of rows, and of the D = 8
    # cases only here in every column
    ("dw_without_last_row", ("ln", 8, 8195, True, "randn", 1e-5), "dw"),
    ("stats_of_unrounded_sum", ("ln", 264, 389, True, "randn", 1e-5), "y"),
    ("stats_of_unrounded_sum", ("rms", 264, 389, True, "randn", 1e-5), "y"),
]


@pytest.mark.parametrize("mutant,case,spoils", MUTANT_CASES)
def test_criterion_rejects_what_the_old_tolerances_accept(mutant, case,
                                                          spoils):
    """Each wrong formula passes atol / rtol of test_gpu_norm_golden.py
    against the fp64 reference and fails the new criterion, even with the
    kernels' slack and floors."""
    family, D, R, fused, kind, eps = case
    assert case in nr.cases() and mutant in nr.MUTANTS
    t = nr.norm_inputs(*case)
    exp = nr.expectation(family, t, eps)
    got = nr.norm32_fwd(family, t["x"], t["res"], t["w"], t["b"], eps, mutant)
    got.update(nr.norm32_bwd(family, t["dy"], exp["xin"], t["w"],
                             exp["mean_in"], exp["rstd_in"], t["dadd"],
                             mutant))
    # the old fp32 rtol = 1e-4 on mean / rstd does see a variance over D - 1
    # (0.2 % of rstd) and the statistics of the unrounded sum; what it passed
    # were those mutants' y, dx and dw
    stats = () if mutant in ("var_over_d_minus_1", "stats_of_unrounded_sum") \
        else ("mean", "rstd")
    for k in BF16_KEYS + stats:
        if exp["ref"][k] is not None:
            atol, rtol = old_tol(k, fused)
            g = got[k].bfloat16() if k in BF16_KEYS else got[k]
            assert torch.allclose(g.double(), exp["ref"][k], atol=atol,
                                  rtol=rtol), (k, "old tolerance rejects it")
    ratios = _ratios(exp, got, nr.S, nr.KERNEL_FLOOR)
    print(f"MUTANT {mutant} {nr.case_name(*case)} {ratios}")
    for k in spoils.split():
        assert ratios[k] > 1.0, (k, ratios[k])
