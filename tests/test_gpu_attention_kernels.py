"""The attention kernels against fp64 references under the half-ulp criterion
of attention_ref.py, called straight through ops.hip_ext(): both kernel
generations at every dispatch edge (QW16 / QW32 / the wide() edge / 32x32,
D = 64 and 128), every window that moves a tile bound, data that forces late
rescales, near one-hot rows and exact counts, document bounds, the packed
entry points, attn_delta and the GQA reduce past their grid caps, and windows
up to 2^32 + 64. The backward gets lse and delta from the fp64 reference
(rounded to fp32), so it is pinned without the forward. RATIO lines are the
numbers of RESULTS.md.
"""

import pytest
import torch

from tests import attention_ref as ar

pytestmark = pytest.mark.gpu

CASES = ar.cases()
IDS = [ar.case_name(c) for c in CASES]
# run twice, bit for bit: one case per kernel build
TWICE = {ar.make_case(sh) for sh in ar.SHAPES} | {
    ar.make_case(sh, w, sc, "randn", st) for sh, w, sc, st in ar.DOC_BUILDS}


def _ext():
    from acco_amd import ops
    return ops.hip_ext()


def _cuda(t):
    return {k: None if v is None else v.cuda() for k, v in t.items()}


def _run(ext, t, c, lse_in, delta_in):
    """o, lse, dq, dk, dv of the unpacked entry points."""
    _, window, scale, _, _ = c
    doc = () if t["doc_start"] is None else (t["doc_start"],)
    o, lse = ext.attn_fwd(t["q"], t["k"], t["v"], scale, window, *doc)
    if doc:
        doc = (t["doc_start"], t["doc_end"])
    dq, dk, dv = ext.attn_bwd(t["q"], t["k"], t["v"], t["dO"], lse_in,
                              delta_in, scale, window, *doc)
    torch.cuda.synchronize()
    return dict(o=o, lse=lse, dq=dq, dk=dk, dv=dv)


def _check(name, exp, got):
    """Every output under the criterion; prints RATIO lines."""
    bad = {}
    for k in ar.BF16_OUT:
        ref = exp["ref"][k]
        assert got[k].dtype == torch.bfloat16 and got[k].shape == ref.shape
        floor = ar.floor_of(exp["terms"][k], k, ref, ar.KERNEL_FLOOR)
        r, idx = ar.within(got[k], ref, floor)
        print(f"RATIO {k} {name} {r:.4f}")
        if not r <= 1.0:
            pos = [int(x) for x in torch.unravel_index(
                torch.tensor(idx), ref.shape)]
            bad[k] = (r, pos, float(got[k].flatten()[idx]),
                      float(ref.flatten()[idx]))
    err = float((got["lse"].double() - exp["ref"]["lse"]).abs().max())
    tol = exp["tol"]["lse"]
    print(f"RATIO lse {name} {err / tol:.4f} (err {err:.3e} tol {tol:.3e})")
    if not err <= tol:
        bad["lse"] = (err, tol)
    assert not bad, bad


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_attention_kernels(case):
    (B, S_, H, Hkv, D), window, scale, kind, starts = case
    ext = _ext()
    t = _cuda(ar.attn_inputs(case))
    exp = ar.expectation(case, t)
    got = _run(ext, t, case, exp["lse_in"], exp["delta_in"])
    assert got["lse"].shape == (B, H, S_) and got["lse"].dtype == torch.float32
    _check(ar.case_name(case), exp, got)
    if window == 1:
        # one key per query: o is v of the query's kv head, bit for bit, and
        # lse the one score (the criterion above has held it to scale·q·k)
        v = t["v"].repeat_interleave(H // Hkv, dim=2)
        assert torch.equal(got["o"], v)
    if kind == "census":
        n = ar.census_count(S_, window, t["doc_start"]).cuda()
        err = (got["lse"].double() - n.log()[:, None, :]).abs().max()
        assert float(err) <= exp["tol"]["lse"], float(err)
    if kind == "do_zero":
        for k in ("dq", "dk", "dv"):
            assert not got[k].any(), k
    if case in TWICE:
        again = _run(ext, t, case, exp["lse_in"], exp["delta_in"])
        for k, x in got.items():
            assert torch.equal(x, again[k]), k


@pytest.mark.parametrize("shape", ar.BIG_WINDOW_SHAPES,
                         ids=["16x16", "32x32"])
def test_window_at_least_S_bounds_nothing(shape):
    """Windows S, S + 1, 2^31 - 1, 2^31 and 2^32 + 64 give the bits of window
    0 (the bindings clamp to S before the cast to int; unclamped, 2^31 - 1
    overflowed q_tile_hi and zeroed dK / dV, and 2^32 + 64 ran as 64), through
    the unpacked entry points and, on the 32x32 shape, the packed ones."""
    ext = _ext()
    B, S_, H, Hkv, D = shape
    c0 = ar.make_case(shape)
    t = _cuda(ar.attn_inputs(c0))
    exp = ar.expectation(c0, t)
    want = _run(ext, t, c0, exp["lse_in"], exp["delta_in"])
    _check(ar.case_name(c0), exp, want)
    assert want["dk"].any() and want["dv"].any()
    packed = S_ % 256 == 0
    if packed:
        qkv = torch.cat([t[k].reshape(B, S_, -1) for k in "qkv"], -1)
        offs = (0, H * D, (H + Hkv) * D)
        dO = t["dO"].reshape(B, S_, H * D)

        def run_packed(w):
            o, lse = ext.attn_fwd_packed(qkv, H, Hkv, D, c0[2], w, *offs)
            dqkv = torch.zeros_like(qkv)
            dkq, dvq = ext.attn_bwd_packed(qkv, dO, exp["lse_in"],
                                           exp["delta_in"], dqkv, H, Hkv, D,
                                           c0[2], w, *offs)
            return o, lse, dqkv, dkq, dvq
        want_p = run_packed(0)
        assert torch.equal(want_p[0].view(B, S_, H, D), want["o"])
    for w in ar.big_windows(S_):
        got = _run(ext, t, (shape, w) + c0[2:], exp["lse_in"],
                   exp["delta_in"])
        for k, x in want.items():
            assert torch.equal(x, got[k]), (w, k)
        if packed:
            for a, b in zip(want_p, run_packed(w)):
                assert torch.equal(a, b), w
    for call in (
            lambda: ext.attn_fwd(t["q"], t["k"], t["v"], c0[2], -1),
            lambda: ext.attn_bwd(t["q"], t["k"], t["v"], t["dO"],
                                 exp["lse_in"], exp["delta_in"], c0[2], -1)):
        with pytest.raises(RuntimeError, match="window"):
            call()


# ------------------------------------------------------ packed entry points
SENTINEL = -1.2578125        # 0xBFA1


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("order", ["qkv", "kvq"])
def test_packed_entry_points(order, D):
    ext = _ext()
    B, S_, H, Hkv = 2, 256, 4, 2
    c = ar.make_case((B, S_, H, Hkv, D))
    name = "packed_%s_%s" % (order, ar.case_name(c))
    cpu = ar.attn_inputs(c)
    W, q_off, k_off, v_off = ar.gqa_layout(Hkv, D, H // Hkv, order)
    g = ar.case_generator(name)
    qkv = (0.5 * torch.randn(B, S_, W, generator=g)).bfloat16()
    for key, off in (("q", q_off), ("k", k_off), ("v", v_off)):
        sec = cpu[key].reshape(B, S_, -1)
        qkv[..., off:off + sec.shape[-1]] = sec
    t, qkv = _cuda(cpu), qkv.cuda()
    exp = ar.expectation(c, t)
    offs = (q_off, k_off, v_off)
    dO = t["dO"].reshape(B, S_, H * D)

    def run(cos=None, sin=None):
        o, lse = ext.attn_fwd_packed(qkv, H, Hkv, D, c[2], 0, *offs)
        dqkv = torch.full_like(qkv, SENTINEL)
        dkq, dvq = ext.attn_bwd_packed(qkv, dO, exp["lse_in"],
                                       exp["delta_in"], dqkv, H, Hkv, D,
                                       c[2], 0, *offs, cos, sin)
        torch.cuda.synchronize()
        return o, lse, dqkv, dkq, dvq

    o, lse, dqkv, dkq, dvq = run()
    qsec = slice(q_off, q_off + H * D)
    dq = dqkv[..., qsec].reshape(B, S_, H, D)
    _check(name, exp, dict(o=o.view(B, S_, H, D), lse=lse, dq=dq, dk=dkq,
                           dv=dvq))
    outside = torch.ones(W, dtype=torch.bool, device="cuda")
    outside[qsec] = False
    assert (dqkv[..., outside] == SENTINEL).all()
    for a, b in zip((o, lse, dqkv, dkq, dvq), run()):
        assert torch.equal(a, b)

    # the inverse RoPE in the dq epilogue, against rope64 of the kernel's
    # own un-roped dq
    cos, sin = ar.rope_tables(S_, D, "cuda")
    o2, lse2, dqkv2, dkq2, dvq2 = run(cos, sin)
    assert torch.equal(o2, o) and torch.equal(lse2, lse)
    assert torch.equal(dkq2, dkq) and torch.equal(dvq2, dvq)
    assert (dqkv2[..., outside] == SENTINEL).all()
    want = ar.rope64(dq, cos, sin, bwd=True)
    r, _ = ar.within_half_ulp(dqkv2[..., qsec].reshape(B, S_, H, D), want,
                              ar.rope_floor(dq))
    print(f"RATIO dq_rope {name} {r:.4f}")
    assert r <= 1.0, r


# --------------------------------------------------------------- attn_delta
@pytest.mark.parametrize("kind", ar.DELTA_KINDS)
@pytest.mark.parametrize("case", ar.DELTA_CASES,
                         ids=["D%d_%dx%dx%d" % c for c in ar.DELTA_CASES])
def test_attn_delta(case, kind):
    ext = _ext()
    D, B, S_, H = case
    dO, o = (x.cuda() for x in ar.delta_inputs(D, B, S_, H, kind))
    got = ext.attn_delta(dO, o)
    torch.cuda.synchronize()
    assert got.shape == (B, H, S_) and got.dtype == torch.float32
    ref = ar.delta64(dO, o)
    err = float((got.double() - ref).abs().max())
    if kind == "ints":
        assert torch.equal(ref, ref.round()) and err == 0.0, err
    # the tolerance comes from at least 1031 rows of the same distribution:
    # the largest fp32 error of three rows is no maximum
    pool = [x.cuda() for x in ar.delta_inputs(D, 1, 1031, 1, kind)]
    tol = max(ar.stat_tol(ar.delta32(dO, o), ref),
              ar.stat_tol(ar.delta32(*pool), ar.delta64(*pool)))
    print(f"RATIO delta D{D}_{B}x{S_}x{H}_{kind} "
          f"{err / tol if tol else 0.0:.4f} (err {err:.3e} tol {tol:.3e})")
    assert err <= tol, (err, tol)
    if kind == "cancel":
        assert float(ref.abs().max()) < 0.05 * float(
            (dO.double() * o.double()).abs().sum(-1).max())
    assert torch.equal(got, ext.attn_delta(dO, o))


# --------------------------------------------------------------- GQA reduce
GQA = ar.gqa_cases()


@pytest.mark.parametrize(
    "case", GQA, ids=["T%dx%d_Hkv%d_D%d_rep%d_%s" % (*c[0], *c[1:])
                      for c in GQA])
def test_attn_gqa_reduce(case):
    ext = _ext()
    (B, S_), Hkv, D, rep, order = case
    dkq, dvq = (x.cuda() for x in ar.gqa_inputs(*case))
    W, q_off, k_off, v_off = ar.gqa_layout(Hkv, D, rep, order)
    dqkv = torch.full((B, S_, W), SENTINEL, device="cuda",
                      dtype=torch.bfloat16)
    ext.attn_gqa_reduce(dkq, dvq, dqkv, Hkv, rep, D, k_off, v_off)
    torch.cuda.synchronize()
    ksec = slice(k_off, k_off + Hkv * D)
    vsec = slice(v_off, v_off + Hkv * D)
    worst = 0.0
    for x, sec in ((dkq, ksec), (dvq, vsec)):
        ref, floor = ar.gqa64(x, Hkv, rep)
        r, _ = ar.within_half_ulp(dqkv[..., sec], ref, floor)
        worst = max(worst, r)
    print(f"RATIO gqa_reduce {case} {worst:.4f}")
    assert worst <= 1.0, worst
    outside = torch.ones(W, dtype=torch.bool, device="cuda")
    outside[ksec] = False
    outside[vsec] = False
    assert (dqkv[..., outside] == SENTINEL).all()
    again = torch.full_like(dqkv, SENTINEL)
    ext.attn_gqa_reduce(dkq, dvq, again, Hkv, rep, D, k_off, v_off)
    assert torch.equal(again, dqkv)

    # the rotating variant: bit-equal to the plain reduce followed by the
    # stand-alone inverse rope of the k section
    cos, sin = ar.rope_tables(S_, D, "cuda")
    want = dqkv.clone()
    ext.rope_packed(want, want, cos, sin, k_off, Hkv, D, True)
    got = torch.full_like(dqkv, SENTINEL)
    ext.attn_gqa_reduce_rope(dkq, dvq, got, cos, sin, Hkv, rep, D, k_off,
                             v_off)
    torch.cuda.synchronize()
    assert torch.equal(got, want), \
        float((got.float() - want.float()).abs().max())
