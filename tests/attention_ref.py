"""fp64 references, an fp32 emulation, case lists and the acceptance criterion
of the attention kernels (attention_fwd*.hip, attention_bwd*.hip, delta.hip),
shared by test_gpu_attention_kernels.py (the kernels) and
test_attention_ref.py (the criterion itself, on the CPU). The half-ulp rule,
its slack S_FP32 / S, `fp32_tol`, `stat_tol` and the case generator are those
of streaming_ref.py and norm_ref.py.

Every reference is computed from the kernel's own bf16 / fp32 / int32 inputs
upcast to float64, on whatever device they are on. For q [B,S,H,D], k and v
[B,S,Hkv,D] (query head h reads kv head h // (H/Hkv)), scale, window and an
optional doc_start [B,S]:
    mask   query i attends key j iff j <= i, j > i - window (window > 0) and
           j >= doc_start[i]
    fwd    P = softmax(scale·QK^T + mask), o = P·V, lse = logsumexp in natural
           units [B,H,S]
    delta  sum_d dO·o [B,H,S]
    bwd    takes lse and delta as fp32 inputs (the tests pass the fp64 values
           rounded to fp32, so dq and dkv are pinned without the forward) and
           upcasts those same values: P = exp(s - lse),
           dS = P·(dO·V^T - delta)·scale, dq = dS·K, and per QUERY head
           [B,S,H,D], as attn_bwd emits them, dk = dS^T·Q, dv = P^T·dO.

bf16 outputs (o, dq, dk, dv): `within_half_ulp(got, ref64, floor, s=S)` with
floor = bf16 term + fp32 term.
  bf16 term, derived, coefficient 1: P (in the backward also dS) is rounded
  once to bf16 by RNE before the second MFMA, unit roundoff 2^-8, so
      o   2^-8·sum_j P_ij·|v_jd|        dv  2^-8·sum_i P_ij·|dO_id|
      dq  2^-8·sum_j |dS_ij|·|k_jd|     dk  2^-8·sum_i |dS_ij|·|q_id|
  whatever the tiling; the deferred max scales P by at most e^8 before the
  rounding, which leaves the relative error alone.
  fp32 term: fp32 accumulation, the dP - delta cancellation and the error of
  exp(s - lse): COEF·(attended keys or queries + D)·2^-24·(|A|·|B|), the
  shape of gemm_floor, where for dq and dk
      T_ij = scale·P_ij·(sum_d |dO_id|·|v_jd| + |delta_i|)·(1 + |s_ij| + |lse_i|)
  stands in for |dS_ij| (row 0 has dS = 0 exactly, and its floor must not be
  0). COEF is measured on the fp32 emulation below: the smallest power of two
  with which every case passes at s = S_FP32 on the CPU (test_attention_ref.py
  prints the largest coefficient any element needs as COEF lines); the
  kernels get KERNEL_FLOOR = 4x that.

Two places where the rule of streaming_ref.py is completed, not loosened
(RESULTS.md, "Deviations"):
  rounding term: the kernel rounds ref + e, |e| <= floor, to bf16. Where that
  sum crosses into the next binade the half ulp of the rounding is that of
  |ref| + floor, so `floor_of` adds (0.5 + s)·(ulp(|ref| + floor) - ulp(ref)),
  zero everywhere else. (dv of the census case with documents: ref
  -0.0078100 just under 2^-7, two terms P = 1/255 and 1/256 whose bf16
  roundings move the sum by 1.16 ulp to -0.0078453, which rounds to
  -0.0078735: 2.08 ulp(ref) off with a floor of 1.34 ulp.)
  exact zeros: row 0 of dq has dS = 0 exactly while fp32 leaves rounding
  noise there;
  `within` holds a zero reference that has a floor to that floor, where
  within_half_ulp alone would ask |got| <= 2^-119.

MEASURED (CPU, fp32 emulation, the 99 cases of cpu_cases(), slack S_FP32):
    largest fp32-term coefficient needed: dq 0.0113, dk 0.0113 (window 1 at
    S = 768: one key per row, dS = P·(dP - delta) cancels to rounding noise);
    o 0 and dv 0 (the bf16 term covers them), so they take the backward's
    -> COEF = 2^-6 for o, dq, dk, dv (kernels 2^-4)
    worst err/limit with these: o 0.9282, dq 0.9953, dk 0.9782, dv 0.9832;
    lse err/tol 0.125 (= 1 / FP32_MARGIN, it sets its own tolerance)
    the cap: 100 % of the elements of every randn case
MEASURED (MI355X, kernels, slack S, floors 4x): worst err/limit
                o       dq      dk      dv      lse err/tol
    16x16 D64   0.8498  0.9814  0.9615  0.9694  0.151
    16x16 D128  0.8622  0.9597  0.9439  0.9448  0.155
    32x32 D64   0.9077  0.9673  0.9372  0.9733  0.148
    32x32 D128  0.9262  0.9913  0.9743  0.9805  0.155
    packed      0.6839  0.8051  0.9338  0.8687  0.134   dq after rope 0.9922
    attn_delta err/tol 0.128; GQA reduce 0.9922 (= 0.5 / (0.5 + 2^-8))
Mutants (cases they change / older tolerances pass / criterion rejects):
    window one key too wide 61 / 24 / 61, too narrow 65 / 27 / 65,
    causal admits i + 1 99 / 0 / 99, doc_start - 1 8 / 0 / 8, first kv tile
    of a windowed block dropped 72 / 0 / 72, delta of the neighbouring row
    97 / 0 / 97, -delta unscaled 89 / 0 / 89, lse from a stale max
    97 / 97 / 97 (lse alone sees it), P truncated to bf16 97 / 97 / 92,
    rescale threshold 800 97 / 96 / 1: NOT caught, and not an error of the
    result: P/l is the same quotient whatever max P was scaled by, until
    exp overflows (the sharp case at S = 768 is the one rejection).

fp32 outputs (lse, delta): tolerance = FP32_MARGIN x the larger of the fp32
formula's own largest error against fp64 on the same inputs and one fp32 ulp
of the largest |reference| (`stat_tol` of norm_ref.py).

`attn32_fwd` / `attn32_bwd` are torch fp32 functions that work tile-wise, 64
keys per tile, with an online softmax whose running max is deferred while no
row of a 32-row group grows by more than 8 natural units (attention_fwd32.hip)
and that round P and dS to bf16 where the kernels do. They carry the criterion
on the CPU and take a `mutant` (MUTANTS) that test_attention_ref.py uses to
show what the criterion rejects.

The cap that keeps the floor honest, asserted on the CPU: on every randn case
the limit (half-ulp + kernel floor) lies below a quarter of the tolerance the
older tests use, atol + 4e-2·|ref| with atol = 4e-2 (o) / 8e-2 (gradients), on
at least 99 % of the elements.
"""

import math

import torch

from tests.norm_ref import needed_coefficient, stat_tol  # noqa: F401
from tests.streaming_ref import (FP32_MARGIN, S, S_FP32,  # noqa: F401
                                 case_generator, fp32_tol, rope64, rope_floor,
                                 ulp_bf16, within_half_ulp)

# measured coefficients of the fp32 term (see the docstring); the kernels get
# KERNEL_FLOOR times these
COEF = dict(o=2.0 ** -6, dv=2.0 ** -6, dq=2.0 ** -6, dk=2.0 ** -6)
KERNEL_FLOOR = 4.0
BF16_U = 2.0 ** -8
OLD_ATOL = dict(o=4e-2, dq=8e-2, dk=8e-2, dv=8e-2)
OLD_RTOL = 4e-2
TILE = 64

# (B, S, H, Hkv, D) -> the kernels it reaches; each the smallest that does
SHAPES = [
    (2, 64, 2, 1, 64), (1, 192, 3, 1, 64),          # 16x16 QW16, D64
    (1, 128, 2, 2, 64), (1, 384, 4, 1, 64),         # 16x16 QW32, D64
    (1, 64, 2, 1, 128), (1, 128, 2, 2, 128),        # 16x16 QW16, D128; the
    (1, 192, 2, 1, 128),                            # second is the wide() edge
    (2, 256, 2, 1, 64), (1, 768, 3, 3, 64),         # 32x32, D64
    (1, 256, 2, 1, 128), (1, 512, 4, 1, 128),       # 32x32, D128
]
# one shape per generation and D for the windows
WINDOW_SHAPES = [(1, 384, 4, 1, 64), (1, 192, 2, 1, 128),
                 (1, 768, 3, 3, 64), (1, 512, 4, 1, 128)]
# one shape per generation for the data kinds
KIND_SHAPES = [(1, 192, 3, 1, 64), (1, 768, 3, 3, 64)]
KINDS = ["spike", "stairs", "sharp", "census", "do_zero"]
CENSUS_WINDOWS = [31, 33, 96]
# the start lists of test_gpu_doc_mask.py: (shape, window, scale, starts)
MIXED = [[0, 1, 64, 128, 198], [0]]
DOC_BUILDS = [
    ((2, 256, 2, 1, 64), 0, None, MIXED),
    ((1, 768, 4, 2, 64), 0, None, [[0, 300, 512, 700]]),
    ((1, 512, 2, 2, 64), 96, 1.0, [[0, 200, 260]]),
    ((1, 512, 2, 1, 128), 0, None, [[0, 70, 330]]),
]
# exactness and overflow of the window: one 16x16 and one 32x32 shape
BIG_WINDOW_SHAPES = [(1, 192, 3, 1, 64), (2, 256, 2, 1, 64)]


def windows_for(S_):
    return [1, 2, 31, 32, 33, 63, 64, 65, 96, 255, 256, 257, S_ - 1, S_,
            S_ + 1]


def big_windows(S_):
    return [S_, S_ + 1, 2 ** 31 - 1, 2 ** 31, 2 ** 32 + 64]


def make_case(shape, window=0, scale=None, kind="randn", starts=None):
    """A case: (shape, window, scale, kind, starts); scale None = D^-0.5."""
    scale = shape[4] ** -0.5 if scale is None else float(scale)
    starts = None if starts is None else tuple(tuple(r) for r in starts)
    return (tuple(shape), int(window), scale, kind, starts)


def case_name(c):
    shape, window, scale, kind, starts = c
    doc = "" if starts is None else "_doc" + "-".join(
        ".".join(map(str, r)) for r in starts)
    return "attn_%dx%dx%dx%dx%d_w%d_s%g_%s%s" % (*shape, window, scale, kind,
                                                 doc)


def cases():
    out = [make_case(sh) for sh in SHAPES]
    for sh in WINDOW_SHAPES:
        out += [make_case(sh, w) for w in windows_for(sh[1])]
        out.append(make_case(sh, 64, 1.0))
    for sh in KIND_SHAPES:
        for kind in KINDS:
            # sharp: |lse| ~ 100 needs the unscaled scores
            out.append(make_case(sh, 0, 1.0 if kind == "sharp" else None,
                                 kind))
        out += [make_case(sh, w, None, "census") for w in CENSUS_WINDOWS]
    for sh, w, sc, starts in DOC_BUILDS:
        out.append(make_case(sh, w, sc, "randn", starts))
        out.append(make_case(sh, w, sc, "census", starts))
    seen, uniq = set(), []
    for c in out:
        if c not in seen:
            seen.add(c)
            uniq.append(c)
    return uniq


def cpu_cases():
    """What test_attention_ref.py runs: every case (the largest is S = 768)."""
    return cases()


def doc_arrays(starts, S_):
    """int32 [B, S] doc_start and (exclusive) doc_end from start lists."""
    ds = torch.zeros(len(starts), S_, dtype=torch.int32)
    de = torch.full((len(starts), S_), S_, dtype=torch.int32)
    for b, row in enumerate(starts):
        row = sorted(row)
        for n, s0 in enumerate(row):
            ds[b, s0:] = s0
            end = row[n + 1] if n + 1 < len(row) else S_
            de[b, s0:end] = end
    return ds, de


def attn_inputs(c):
    """dict of CPU tensors: q, dO [B,S,H,D], k, v [B,S,Hkv,D] bf16, and
    doc_start / doc_end int32 [B,S] (None without documents)."""
    (B, S_, H, Hkv, D), window, scale, kind, starts = c
    g = case_generator(case_name(c))

    def rn(*shape):
        return torch.randn(*shape, generator=g)

    # randn·0.5, the data of the older attention tests
    q, k, v, dO = (0.5 * x for x in (rn(B, S_, H, D), rn(B, S_, Hkv, D),
                                     rn(B, S_, Hkv, D), rn(B, S_, H, D)))
    if kind == "spike":
        # K rows off the 32-multiples, in the third tile or later of a block:
        # a late rescale that one half of a wave does not see coming
        for pos in range(2 * TILE + 13, S_, 3 * TILE + 24):
            assert pos % 32 != 0
            k[:, pos] = 8.0
    elif kind == "stairs":
        # scores rise ~5 natural units per 64-key tile: deferred and rescaled
        # tiles alternate and P reaches e^8 before it is rounded
        q, k = 0.5 * q, 0.5 * k
        q[..., 0] = 4.0
        step = 5.0 / (scale * 4.0)
        k[..., 0] = (torch.arange(S_) // TILE).float()[None, :, None] * step
    elif kind == "sharp":
        q, k = 4.0 * q, 4.0 * k          # randn·2
    elif kind == "census":
        q = torch.zeros_like(q)
        v = (torch.arange(S_)[:, None] % D == torch.arange(D)[None, :]) \
            .float()[None, :, None, :].expand(B, S_, Hkv, D).clone()
    elif kind == "do_zero":
        dO = torch.zeros_like(dO)
    else:
        assert kind == "randn", kind
    t = dict(q=q.bfloat16(), k=k.bfloat16(), v=v.bfloat16(),
             dO=dO.bfloat16(), doc_start=None, doc_end=None)
    if starts is not None:
        t["doc_start"], t["doc_end"] = doc_arrays(starts, S_)
    return t


# ------------------------------------------------------------------ the mask
MASK_MUTANTS = ["window_wide", "window_narrow", "causal_plus_one",
                "doc_start_minus_one", "first_tile_dropped"]
SOFTMAX_MUTANTS = ["rescale_800", "lse_stale_max", "p_truncated"]
DELTA_MUTANTS = ["delta_neighbour", "delta_unscaled"]
MUTANTS = MASK_MUTANTS + SOFTMAX_MUTANTS + DELTA_MUTANTS


def attend_mask(S_, window, doc_start=None, device="cpu", mutant=None):
    """bool [B or 1, 1, S, S]: [.., i, j] = query i attends key j."""
    i = torch.arange(S_, device=device)[:, None]
    j = torch.arange(S_, device=device)[None, :]
    m = j <= (i + 1 if mutant == "causal_plus_one" else i)
    if window > 0:
        w = window + (mutant == "window_wide") - (mutant == "window_narrow")
        m = m & (j > i - w)
        if mutant == "first_tile_dropped":
            # the first kv tile of each row block (256 rows under the 32x32
            # kernels, else 64)
            rows = 256 if S_ % 256 == 0 else TILE
            blk0 = (i // rows) * rows
            j_lo = (blk0 - window + 1).clamp(min=0) // TILE
            m = m & (j // TILE != j_lo)
    m = m[None, None]
    if doc_start is not None:
        ds = doc_start.to(device).long()
        if mutant == "doc_start_minus_one":
            ds = ds - 1
        m = m & (j[None, None] >= ds[:, None, :, None])
    return m


def _heads(t, H, dt):
    """[B,S,h,D] -> [B,H,S,D] in dtype dt, kv heads repeated per group."""
    t = t.to(dt).permute(0, 2, 1, 3)
    rep = H // t.shape[1]
    return t.repeat_interleave(rep, dim=1) if rep > 1 else t


def _bshd(t):
    return t.permute(0, 2, 1, 3).contiguous()


# ---------------------------------------------------------- fp64 references
def attn64_fwd(q, k, v, scale, window=0, doc_start=None):
    """o [B,S,H,D], lse [B,H,S], and P, s (scaled scores, 0 where masked),
    allow for the floors; all fp64."""
    H, S_ = q.shape[2], q.shape[1]
    dt = torch.float64
    qh, kh, vh = _heads(q, H, dt), _heads(k, H, dt), _heads(v, H, dt)
    allow = attend_mask(S_, window, doc_start, q.device)
    s = (qh @ kh.transpose(-1, -2)) * scale
    sm = s.masked_fill(~allow, -math.inf)
    lse = torch.logsumexp(sm, dim=-1)
    P = torch.exp(sm - lse[..., None])
    return dict(o=_bshd(P @ vh), lse=lse, P=P,
                s=s.masked_fill(~allow, 0.0), allow=allow, vh=vh, qh=qh, kh=kh)


def delta64(dO, o):
    """[B,H,S] from dO, o [B,S,H,D]."""
    return (dO.double() * o.double()).sum(-1).permute(0, 2, 1).contiguous()


def delta32(dO, o):
    return (dO.float() * o.float()).sum(-1).permute(0, 2, 1).contiguous()


def attn64_bwd(q, k, v, dO, lse, delta, scale, window=0, doc_start=None):
    """dq, dk, dv [B,S,H,D] (dk, dv per query head) in fp64 from the fp32
    lse / delta the kernels are given, and P, dS, T for the floors."""
    H, S_ = q.shape[2], q.shape[1]
    dt = torch.float64
    qh, kh, vh = _heads(q, H, dt), _heads(k, H, dt), _heads(v, H, dt)
    doh = _heads(dO, H, dt)
    allow = attend_mask(S_, window, doc_start, q.device)
    s = (qh @ kh.transpose(-1, -2)) * scale
    lse, delta = lse.double(), delta.double()
    zero = torch.zeros_like(s)
    P = torch.where(allow, torch.exp(s - lse[..., None]), zero)
    dP = doh @ vh.transpose(-1, -2)
    dS = P * (dP - delta[..., None]) * scale
    T = scale * P * (doh.abs() @ vh.abs().transpose(-1, -2)
                     + delta.abs()[..., None]) \
        * (1.0 + torch.where(allow, s, zero).abs() + lse.abs()[..., None])
    return dict(dq=_bshd(dS @ kh), dk=_bshd(dS.transpose(-1, -2) @ qh),
                dv=_bshd(P.transpose(-1, -2) @ doh), P=P, dS=dS, T=T,
                allow=allow, qh=qh, kh=kh, doh=doh)


# ------------------------------------------------------------- the floors
def fwd_floor_terms(f):
    """(bf16 term, 2^-24 fp32 term) of o from attn64_fwd's result."""
    pv = _bshd(f["P"] @ f["vh"].abs())
    n = f["allow"].sum(-1).double() + f["vh"].shape[-1]     # [Bm,1,S]
    n = n.expand(f["P"].shape[:3]).permute(0, 2, 1)[..., None]
    return BF16_U * pv, 2.0 ** -24 * n * pv


def bwd_floor_terms(b):
    """{dq, dk, dv: (bf16 term, 2^-24 fp32 term)} from attn64_bwd's result."""
    D = b["qh"].shape[-1]
    P, dS, T, allow = b["P"], b["dS"].abs(), b["T"], b["allow"]
    nq = (allow.sum(-1).double() + D).expand(P.shape[:3])   # per query
    nk = (allow.sum(-2).double() + D).expand(P.shape[:3])   # per key
    nq = nq.permute(0, 2, 1)[..., None]
    nk = nk.permute(0, 2, 1)[..., None]
    qa, ka, da = b["qh"].abs(), b["kh"].abs(), b["doh"].abs()
    pt, dst, tt = (x.transpose(-1, -2) for x in (P, dS, T))
    return dict(
        dq=(BF16_U * _bshd(dS @ ka), 2.0 ** -24 * nq * _bshd(T @ ka)),
        dk=(BF16_U * _bshd(dst @ qa), 2.0 ** -24 * nk * _bshd(tt @ qa)),
        dv=(BF16_U * _bshd(pt @ da), 2.0 ** -24 * nk * _bshd(pt @ da)))


def floor_of(terms, key, ref64, mult=1.0, s=S):
    """bf16 term + mult·COEF·fp32 term + the rounding term: the kernel rounds
    ref + e with |e| <= floor, and where that crosses into the next binade the
    half ulp of the rounding is that of |ref| + floor, not of |ref|."""
    bf, fp = terms
    floor = bf + mult * COEF[key] * fp
    return floor + (0.5 + s) * (ulp_bf16(ref64.abs() + floor)
                                - ulp_bf16(ref64))


def within(got, ref64, floor, s=S):
    """within_half_ulp, except that an exactly zero reference with a floor
    (row 0 of dq: dS = 0) is held to its floor, not to |got| <= 2^-119."""
    tiny = (ref64.abs() < 2.0 ** -120) & (floor > 2.0 ** -119)
    zero = torch.zeros_like(ref64)
    r, idx = within_half_ulp(torch.where(tiny, zero, got.double()),
                             torch.where(tiny, zero, ref64), floor, s)
    if bool(tiny.any()):
        rt = (got.double() - ref64).abs() / floor.clamp(min=2.0 ** -119)
        rt = torch.where(tiny, rt, zero).flatten()
        if float(rt.max()) > r:
            return float(rt.max()), int(rt.argmax())
    return r, idx


def old_tolerance(key, ref64):
    return OLD_ATOL[key] + OLD_RTOL * ref64.abs()


def limit_below_quarter_old(key, floor, ref64, s=S):
    """Fraction of elements whose limit is under a quarter of the older
    tests' tolerance."""
    limit = (0.5 + s) * ulp_bf16(ref64) + floor
    return float((limit < 0.25 * old_tolerance(key, ref64)).double().mean())


# --------------------------------------------------------- fp32 emulation
def _to_bf16(x, trunc):
    if trunc:
        return (x.contiguous().view(torch.int32) & -65536).view(torch.float32)
    return x.bfloat16().float()


def attn32_fwd(q, k, v, scale, window=0, doc_start=None, mutant=None):
    """o [B,S,H,D] bf16 and lse [B,H,S] fp32 by the kernels' algorithm in
    torch fp32 ops."""
    B, S_, H, D = q.shape
    dt = torch.float32
    qh, kh, vh = _heads(q, H, dt), _heads(k, H, dt), _heads(v, H, dt)
    allow = attend_mask(S_, window, doc_start, q.device, mutant)
    thr = 800.0 if mutant == "rescale_800" else 8.0
    m = torch.full((B, H, S_), -1e30, dtype=dt, device=q.device)
    m_stale = m.clone()
    l = torch.zeros_like(m)
    acc = torch.zeros(B, H, S_, D, dtype=dt, device=q.device)
    for j in range(S_ // TILE):
        sl = slice(j * TILE, (j + 1) * TILE)
        a = allow[..., sl]
        if not bool(a.any()):
            continue
        s = (qh @ kh[:, :, sl].transpose(-1, -2)) * scale
        s = torch.where(a, s, torch.full_like(s, -1e30))
        tmax = s.amax(-1)
        # one decision per 32 rows (a wave of the 32x32 kernels)
        grow = (tmax > m + thr).view(B, H, S_ // 32, 32).any(-1, keepdim=True)
        grow = grow.expand(B, H, S_ // 32, 32).reshape(B, H, S_)
        m_new = torch.where(grow, torch.maximum(m, tmax), m)
        alpha = torch.exp(m - m_new)
        l = l * alpha
        acc = acc * alpha[..., None]
        m_stale = torch.where(m_new != m, m, m_stale)
        m = m_new
        p = torch.where(a, torch.exp(s - m[..., None]), torch.zeros_like(s))
        l = l + p.sum(-1)
        acc = acc + _to_bf16(p, mutant == "p_truncated") @ vh[:, :, sl]
    o = acc / l[..., None]
    lse = (m_stale if mutant == "lse_stale_max" else m) + torch.log(l)
    return _bshd(o).bfloat16(), lse


def attn32_bwd(q, k, v, dO, lse, delta, scale, window=0, doc_start=None,
               mutant=None):
    """dq, dk, dv [B,S,H,D] bf16 by the kernels' algorithm in fp32."""
    B, S_, H, D = q.shape
    dt = torch.float32
    qh, kh, vh = _heads(q, H, dt), _heads(k, H, dt), _heads(v, H, dt)
    doh = _heads(dO, H, dt)
    allow = attend_mask(S_, window, doc_start, q.device, mutant)
    lse, dl = lse.float()[..., None], delta.float()
    if mutant == "delta_neighbour":
        dl = torch.roll(dl, 1, dims=-1)
    dl = dl[..., None]
    trunc = mutant == "p_truncated"
    dq = torch.zeros(B, H, S_, D, dtype=dt, device=q.device)
    dk, dv = torch.zeros_like(dq), torch.zeros_like(dq)
    for j in range(S_ // TILE):
        sl = slice(j * TILE, (j + 1) * TILE)
        a = allow[..., sl]
        if not bool(a.any()):
            continue
        s = (qh @ kh[:, :, sl].transpose(-1, -2)) * scale
        p = torch.where(a, torch.exp(s - lse), torch.zeros_like(s))
        dp = doh @ vh[:, :, sl].transpose(-1, -2)
        if mutant == "delta_unscaled":
            ds = p * (dp * scale - dl)
        else:
            ds = p * (dp - dl) * scale
        pb, dsb = _to_bf16(p, trunc), _to_bf16(ds, trunc)
        dv[:, :, sl] = pb.transpose(-1, -2) @ doh
        dk[:, :, sl] = dsb.transpose(-1, -2) @ qh
        dq = dq + dsb @ kh[:, :, sl]
    return tuple(_bshd(x).bfloat16() for x in (dq, dk, dv))


# ------------------------------------------------- everything of one case
BF16_OUT = ("o", "dq", "dk", "dv")


def expectation(c, t, formulas32=False, mutant=None):
    """What a case's outputs are held to, from `t` = attn_inputs(c), on the
    device `t` is on: ref (fp64 o, lse, dq, dk, dv), terms (the two floor
    terms of each bf16 output), tol (lse), the backward's inputs lse_in and
    delta_in (fp32), and with formulas32 the emulation's outputs got32."""
    _, window, scale, _, _ = c
    ds = t["doc_start"]
    f = attn64_fwd(t["q"], t["k"], t["v"], scale, window, ds)
    lse_in = f["lse"].float()
    delta_in = delta64(t["dO"], f["o"]).float()
    b = attn64_bwd(t["q"], t["k"], t["v"], t["dO"], lse_in, delta_in, scale,
                   window, ds)
    terms = dict(o=fwd_floor_terms(f), **bwd_floor_terms(b))
    o32, lse32 = attn32_fwd(t["q"], t["k"], t["v"], scale, window, ds)
    out = dict(ref=dict(o=f["o"], lse=f["lse"], dq=b["dq"], dk=b["dk"],
                        dv=b["dv"]),
               terms=terms, tol=dict(lse=stat_tol(lse32, f["lse"])),
               lse_in=lse_in, delta_in=delta_in, allow=f["allow"])
    if formulas32:
        if mutant is not None:
            o32, lse32 = attn32_fwd(t["q"], t["k"], t["v"], scale, window, ds,
                                    mutant)
        dq, dk, dv = attn32_bwd(t["q"], t["k"], t["v"], t["dO"], lse_in,
                                delta_in, scale, window, ds, mutant)
        out["got32"] = dict(o=o32, lse=lse32, dq=dq, dk=dk, dv=dv)
    return out


def census_count(S_, window, doc_start=None):
    """Attended keys of each query: min(i + 1, window, i - doc_start + 1);
    float64 [B or 1, S]."""
    i = torch.arange(S_, dtype=torch.float64)[None]
    n = i + 1
    if window > 0:
        n = torch.minimum(n, torch.full_like(n, float(window)))
    if doc_start is not None:
        n = torch.minimum(n, i - doc_start.double().cpu() + 1)
    return n


# -------------------------------------------------- attn_delta, gqa reduce
# (D, B, S, H) and what it reaches
DELTA_CASES = [
    (64, 1, 1, 3),          # rows not a multiple of 8
    (64, 1, 1031, 130),     # 134030 rows: second grid trip
    (64, 2, 5, 3),          # the [B,H,S] layout
    (128, 1, 1, 3),         # rows not a multiple of 4
    (128, 1, 1031, 65),     # 67015 rows: second grid trip
    (128, 2, 5, 3),
    (8, 1, 1, 1), (72, 1, 5, 1), (520, 1, 1, 1), (520, 2, 5, 3),
    (8, 1, 5463, 3),        # 16389 rows: past the generic kernel's grid cap
]
DELTA_KINDS = ["randn", "cancel", "ints"]


def delta_inputs(D, B, S_, H, kind):
    g = case_generator("delta_%d_%d_%d_%d_%s" % (D, B, S_, H, kind))
    dO = torch.randn(B, S_, H, D, generator=g)
    o = torch.randn(B, S_, H, D, generator=g)
    if kind == "cancel":
        # the second half repeats the first with the sign of o flipped, up
        # to 1 %: the sum is about 0, not exactly (an exact 0 would leave the
        # tolerance rule nothing to measure)
        h = D // 2
        dO[..., h:] = dO[..., :h].clone()
        o[..., h:] = -(o[..., :h] + 0.01 * torch.randn(B, S_, H, h,
                                                       generator=g))
    elif kind == "ints":
        dO = torch.randint(-8, 9, (B, S_, H, D), generator=g).float()
        o = torch.randint(-8, 9, (B, S_, H, D), generator=g).float()
    else:
        assert kind == "randn", kind
    return dO.bfloat16(), o.bfloat16()


# (T = B·S as (B, S), Hkv, D, rep, order)
def gqa_cases():
    out = [((2, 37), Hkv, D, rep, order)
           for rep in (1, 2, 4, 8) for Hkv in (1, 3) for D in (64, 128)
           for order in ("qkv", "kvq")]
    out.append(((2, 4100), 4, 128, 2, "qkv"))    # 524800 items > 2048·256
    return out


def gqa_layout(Hkv, D, rep, order):
    """(W, q_off, k_off, v_off) of the packed grad, with 8 spare columns
    between and after the sections (they must keep their sentinel)."""
    H = Hkv * rep
    if order == "qkv":
        q_off, k_off = 0, H * D + 8
        v_off = k_off + Hkv * D + 8
        W = v_off + Hkv * D + 8
    else:
        k_off, v_off = 0, Hkv * D + 8
        q_off = v_off + Hkv * D + 8
        W = q_off + H * D + 8
    return W, q_off, k_off, v_off


def gqa_inputs(BS, Hkv, D, rep, order):
    g = case_generator("gqa_%d_%d_%d_%d_%d_%s" % (*BS, Hkv, D, rep, order))
    shape = (*BS, Hkv * rep, D)
    return (torch.randn(*shape, generator=g).bfloat16(),
            torch.randn(*shape, generator=g).bfloat16())


def gqa64(x, Hkv, rep):
    """fp64 group sum [B,S,Hkv·D] and its floor rep·2^-24·sum|terms|."""
    B, S_, H, D = x.shape
    x = x.double().view(B, S_, Hkv, rep, D)
    return (x.sum(3).reshape(B, S_, Hkv * D),
            rep * 2.0 ** -24 * x.abs().sum(3).reshape(B, S_, Hkv * D))


def rope_tables(S_, D, device="cpu"):
    inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2).float() / D))
    ang = torch.arange(S_).float()[:, None] * inv[None, :]
    ang = torch.cat((ang, ang), -1)
    return ang.cos().to(device), ang.sin().to(device)
