"""Every norm entry point over every kernel instantiation and row-loop edge:
each output against the fp32 torch reference (tolerances of the norm tests
in test_gpu_kernels.py and test_gpu_fused_glue.py) AND bit for bit against
sha256 prefixes recorded from the build named in golden/norms_parent.json,
i.e. the norm kernels before they were folded into shared templates.

Inputs come from a CPU generator seeded from the case name, so the hashes
do not depend on the device RNG; the norm paths hold no atomics, so the
outputs are run-to-run deterministic."""

import hashlib
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "norms_parent.json")
EPS = 1e-5

# D -> what it selects (fwd grouping G / chunk count CH; bwd kernel)
#   256  G=4; wave-per-row bwd CH=1
#   768  G=2 with 96 of 128 lanes live; wave-per-row CH=2, half-empty chunk
#   1024 G=2 full; last wave-per-row width
#   2048 CH=1 full; first block-per-row bwd
#   2560 CH=2 with a partly empty second chunk
#   4096 CH=2 full;  8192 CH=4;  16384 CH=8
DIMS = [256, 768, 1024, 2048, 2560, 4096, 8192, 16384]

# Cases whose dW missed the reference tolerance on the recording build
# itself, so no hash is pinned for them (max abs error against atol 0.3).
# All four are residual-fused cases with thousands of rows: the reference
# normalizes the unrounded fp32 x + res while the kernels (by design) read
# the stored bf16 sum, and that rounding noise grows with sqrt(R); the add
# tolerance was set at 132 rows. The plain cases at the same shapes run the
# same dW code and pass the tighter plain tolerance.
# test_gpu_norm_kernels.py runs these four against a reference of the bf16 sum.
PARENT_MISSES_REFERENCE = {
    "rms_2048_8195_add": 1.118,
    "ln_256_4099_add": 0.4662,
    "ln_768_8195_add": 0.8310,
    "ln_2048_8195_add": 0.8873,
}


def _rows(D):
    # 1 and 5 leave row groups / waves without a live row; 1027 passes the
    # 1024-block bwd cap so three blocks take a second row
    rows = [1, 5, 1027]
    if D <= 1024:
        rows.append(4099)     # > 4·1024: wave-per-row waves take a 2nd row
    if D in (256, 768, 2048):
        rows.append(8195)     # > the 8192-row fwd grid: fwd blocks stride
    return rows


CASES = [name
         for fam in ("rms", "ln") for D in DIMS
         for R in _rows(D) for fused in ("plain", "add")
         for name in [f"{fam}_{D}_{R}_{fused}"]
         if name not in PARENT_MISSES_REFERENCE]


def _sha(t):
    raw = t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()
    return hashlib.sha256(raw).hexdigest()[:16]


def _ref(family, x32, w32, b32):
    from acco_amd.ops import torch_ref
    if family == "rms":
        return torch_ref.rms_norm(x32, w32, EPS)
    return torch_ref.layer_norm(x32, w32, b32, EPS)


def norm_case(name):
    """Run one case through the extension; returns (outs, refs): dicts of
    the kernel outputs and of their fp32 references under the same keys
    (y, s, mean, rstd, dx, dw, db as applicable). Module-level so the
    hashes can be recorded with the same inputs from any build."""
    from acco_amd import ops
    ext = ops.hip_ext()
    family, D, R, fused = name.split("_")
    D, R, add = int(D), int(R), fused == "add"
    seed = int.from_bytes(hashlib.sha256(name.encode()).digest()[:4], "big")
    g = torch.Generator().manual_seed(seed)

    def rand(*shape, scale=1.0, shift=0.0):
        return (torch.randn(*shape, generator=g) * scale + shift
                ).bfloat16().cuda()

    x = rand(R, D)
    dy = rand(R, D)
    w = rand(D, scale=0.1, shift=1.0)
    b = rand(D, scale=0.1)
    res = rand(R, D) if add else None
    dadd = rand(R, D) if add else None

    outs, refs = {}, {}
    if family == "rms":
        if add:
            outs["y"], outs["s"], outs["rstd"] = ext.add_rmsnorm_fwd(
                x, res, w, EPS)
        else:
            outs["y"], outs["rstd"] = ext.rmsnorm_fwd(x, w, EPS)
    else:
        if add:
            (outs["y"], outs["s"], outs["mean"],
             outs["rstd"]) = ext.add_layernorm_fwd(x, res, w, b, EPS)
        else:
            outs["y"], outs["mean"], outs["rstd"] = ext.layernorm_fwd(
                x, w, b, EPS)
    xin = outs["s"] if add else x            # what the statistics saw
    if family == "rms":
        outs["dx"], outs["dw"] = ext.rmsnorm_bwd(dy, xin, w, outs["rstd"],
                                                 dadd)
    else:
        outs["dx"], outs["dw"], outs["db"] = ext.layernorm_bwd(
            dy, xin, w, outs["mean"], outs["rstd"], dadd)

    # fp32 reference, residual sum left unrounded as in the add-norm tests
    x32 = x.float().requires_grad_(True)
    w32 = w.float().requires_grad_(True)
    b32 = b.float().requires_grad_(True)
    s32 = x32 + res.float() if add else x32
    y32 = _ref(family, s32, w32, b32)
    loss = (y32 * dy.float()).sum()
    if add:
        loss = loss + (s32 * dadd.float()).sum()
        refs["s"] = s32.detach()
    loss.backward()
    refs["y"], refs["dx"], refs["dw"] = y32.detach(), x32.grad, w32.grad
    # the row statistics are those of the stored bf16 sum
    xs = xin.float()
    if family == "rms":
        refs["rstd"] = torch.rsqrt(xs.pow(2).mean(-1) + EPS)
    else:
        refs["db"] = b32.grad
        refs["mean"] = xs.mean(-1)
        refs["rstd"] = torch.rsqrt(xs.var(-1, unbiased=False) + EPS)
    return outs, refs


def _tol(key, add):
    """(atol, rtol) of the existing norm tests for this output."""
    if key == "y":
        return 3e-2, 3e-2
    if key == "s":
        return 1e-2, 1e-2
    if key in ("mean", "rstd"):       # fp32 both sides, summation order only
        return 1e-5, 1e-4
    if key == "dx":
        return (3e-2, 5e-2) if add else (3e-2, 3e-2)
    return (0.3, 5e-2) if add else (0.1, 0.05)     # dw, db


def check_against_reference(name, outs, refs):
    """Names of the outputs that miss their reference tolerance."""
    add = name.endswith("_add")
    bad = []
    for key, got in outs.items():
        atol, rtol = _tol(key, add)
        if not torch.allclose(got.float(), refs[key].float(), atol=atol,
                              rtol=rtol):
            err = (got.float() - refs[key].float()).abs().max().item()
            bad.append(f"{key} (max abs err {err:.3e})")
    if add and not torch.equal(outs["s"], refs["s"].bfloat16()):
        bad.append("s is not bf16(x + res)")
    return bad


@pytest.mark.parametrize("name", CASES)
def test_norm_matches_reference_and_parent(name):
    outs, refs = norm_case(name)
    assert set(outs) == set(refs)
    assert not check_against_reference(name, outs, refs)
    with open(GOLDEN) as f:
        gold = json.load(f)["cases"][name]
    assert {k: _sha(v) for k, v in outs.items()} == gold


# ---------------------------------------------------------------- rejection
def _bwd_args(R=5, D=256):
    x = torch.randn(R, D, device="cuda").bfloat16()
    w = torch.ones(D, device="cuda").bfloat16()
    rstd = torch.ones(R, device="cuda")
    return x.clone(), x, w, rstd


def test_rmsnorm_bwd_rejects_short_rstd():
    from acco_amd import ops
    dy, x, w, rstd = _bwd_args()
    with pytest.raises(RuntimeError):
        ops.hip_ext().rmsnorm_bwd(dy, x, w, rstd[:-1].contiguous())


def test_rmsnorm_bwd_rejects_wrong_dadd_numel():
    from acco_amd import ops
    dy, x, w, rstd = _bwd_args()
    with pytest.raises(RuntimeError):
        ops.hip_ext().rmsnorm_bwd(dy, x, w, rstd, x[:-1].contiguous())


def test_rmsnorm_bwd_rejects_width_not_multiple_of_8():
    from acco_amd import ops
    dy, x, w, rstd = _bwd_args(R=5, D=252)
    with pytest.raises(RuntimeError):
        ops.hip_ext().rmsnorm_bwd(dy, x, w, rstd)
