"""fp64 references, case lists and the acceptance criterion of the streaming
kernels (gelu_new, SwiGLU, RoPE, shifted CE, fused AdamW, colsum, gemm_nt),
shared by test_gpu_streaming_kernels.py (the kernels) and
test_streaming_ref.py (the criterion itself, on the CPU).

Every reference is computed from the kernel's own bf16 / fp32 inputs upcast
to float64, on whatever device the inputs are on.

bf16 outputs: `within_half_ulp(got, ref64, floor, s)`. With
ulp(r) = 2^(floor(log2 max(|r|, 2^-126)) - 7), an element passes iff
|got - ref| <= (0.5 + s)·ulp(ref) + floor; where |ref| < 2^-120 only
|got| <= 2^-119 is asked (hardware exp flushes denormals). No element is
left out. A result on the wrong bf16 neighbour is off by >= 0.5 ulp, so it
fails unless the true value lies within s ulp of a rounding midpoint.

The slack s is measured on the reference, not on the kernels: the same
formulas evaluated with fp32 torch ops, rounded to bf16, go through the
criterion against fp64 (test_streaming_ref.py). Over every case list below
the fp32 formulas pass with S_FP32 = 2^-10; the worst err/limit ratios at
S_FP32 on the CPU were
    gelu fwd 0.9974 (floor 3.03e-07), gelu bwd 0.9970 (floor 2.14e-06 per
    unit |dout|), swiglu out 0.9981, dg 0.9982, du 0.9981, rope 0.9980,
    CE dlogits 0.9980, gemm 0.9952.
The kernels get S = 4·S_FP32 = 2^-8 (hardware exp / rcp are ~1-ulp fp32
approximations chained over about four roundings where libm is correctly
rounded); the hard ceiling is 2^-6.

Floors are absolute error terms of fp32 cancellation:
    gelu fwd   4x the fp32 formula's own largest excess over the half-ulp
               limit on the same inputs (1 + tanh(u) cancels for x < -4.5,
               about |x|·2^-24)
    gelu bwd   the same rule at dout = 1, scaled by |dout|
    swiglu     dg: 2^-22·|dout·u|               (1 - sigmoid cancels)
               out, du: 2^-126·|g·u|, 2^-126·|g·dout|: zero for every
               purpose except g in [-91.3, -88.7] with |u| > 1, where fp32
               has no sigmoid (exp(-g) overflows) and the true product
               still exceeds the 2^-120 threshold above
    rope       2^-23·(|x1| + |x2|)              (a·c - b·s cancels)
    CE dlogits 2·tol_lse·scale·p, scale = dloss / max(n_valid, 1)
               (dp = p·d(lse); p is the entry's own probability)
    gemm       K·2^-24·(|A|·|B|^T)              (fp32 accumulation)

fp32 outputs (CE lse and loss, AdamW p/m/v, colsum): tolerance = 8x the
largest absolute error of the fp32 torch computation of the same quantity
against fp64 on the same inputs (`fp32_tol`); the margin covers __expf
scaling its argument by log2(e) before the hardware exp, and reduction order.
The loss is one scalar, so its single fp32 error is one draw of rounding
noise, not a maximum; its tolerance takes the larger of that error and the
largest per-token loss error of the same fp32 computation (the loss is the
mean of those terms, so its error is bounded by theirs).
"""

import hashlib
import math

import torch
import torch.nn.functional as F

S_FP32 = 2.0 ** -10          # what the fp32 formulas need (measured)
S = 4 * S_FP32               # what the kernels get
assert S <= 2.0 ** -6
FP32_MARGIN = 8.0

GELU_C = math.sqrt(2.0 / math.pi)
GELU_A = 0.044715


# ------------------------------------------------------------- criterion
def ulp_bf16(ref64):
    """2^(floor(log2 max(|r|, 2^-126)) - 7) of each element."""
    a = ref64.abs().clamp(min=2.0 ** -126)
    _, e = torch.frexp(a)                    # a = m·2^e, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(a), e - 8)


def within_half_ulp(got, ref64, floor=0.0, s=S):
    """(worst err/limit, its flat index) over every element; <= 1 passes."""
    got64 = got.double()
    ref64 = ref64.double()
    assert got64.shape == ref64.shape, (got64.shape, ref64.shape)
    if ref64.numel() == 0:
        return 0.0, -1
    if not torch.is_tensor(floor):
        floor = torch.full_like(ref64, float(floor))
    err = (got64 - ref64).abs()
    limit = (0.5 + s) * ulp_bf16(ref64) + floor.double().expand_as(ref64)
    tiny = ref64.abs() < 2.0 ** -120
    err = torch.where(tiny, got64.abs(), err)
    limit = torch.where(tiny, torch.full_like(limit, 2.0 ** -119), limit)
    ratio = err / limit
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, math.inf),
                        ratio).flatten()
    idx = int(ratio.argmax())
    return float(ratio[idx]), idx


def excess_over_half_ulp(got, ref64, s=S_FP32):
    """Largest amount by which an element misses the floor-less limit."""
    err = (got.double() - ref64).abs()
    over = err - (0.5 + s) * ulp_bf16(ref64)
    return float(over.clamp(min=0).max()) if over.numel() else 0.0


def fp32_tol(val32, ref64):
    """Tolerance of an fp32 output from the fp32 reference's own error."""
    if ref64.numel() == 0:
        return 0.0
    return FP32_MARGIN * float((val32.double() - ref64).abs().max())


def case_generator(name):
    seed = int.from_bytes(hashlib.sha256(name.encode()).digest()[:4], "big")
    return torch.Generator().manual_seed(seed)


def all_bf16_patterns():
    """Every bf16 bit pattern once, [128, 512]."""
    bits = torch.arange(65536, dtype=torch.int32).to(torch.int16)
    return bits.view(torch.bfloat16).reshape(128, 512).clone()


# ------------------------------------------------------------- gelu_new
GELU_DOUT = [1.0, -0.371, 5.25]
GELU_BWD_MAX = 2.0 ** 60
STRIDE_SHAPE = (9, 1024, 512)       # 589 824 vec8 items > 2048·256


def gelu64(x):
    x = x.double()
    return 0.5 * x * (1.0 + torch.tanh(GELU_C * (x + GELU_A * x * x * x)))


def gelu_grad64(x):
    x = x.double()
    t = torch.tanh(GELU_C * (x + GELU_A * x * x * x))
    du = GELU_C * (1.0 + 3.0 * GELU_A * x * x)
    return 0.5 * (1.0 + t) + 0.5 * x * (1.0 - t * t) * du


def gelu32(x):
    from acco_amd.ops import torch_ref
    return torch_ref.gelu_new(x.float())


def gelu_grad32(x):
    x = x.float()
    x2 = x * x
    t = torch.tanh(GELU_C * (x + GELU_A * x * x2))
    du = GELU_C * (1.0 + 3.0 * GELU_A * x2)
    return 0.5 * (1.0 + t) + 0.5 * x * (1.0 - t * t) * du


def gelu_floors(x):
    """(fwd floor, bwd floor per unit |dout|) for the finite inputs `x`:
    4x the excess of the fp32 formulas themselves. The backward is asked
    for |x| <= 2^60 only: beyond it x^2 overflows fp32 and 0·inf follows,
    in the kernel and in the fp32 formula alike."""
    fwd = 4 * excess_over_half_ulp(gelu32(x).bfloat16(), gelu64(x))
    xb = x[x.float().abs() <= GELU_BWD_MAX]
    bwd = 4 * excess_over_half_ulp(gelu_grad32(xb).bfloat16(),
                                   gelu_grad64(xb))
    return fwd, bwd


# --------------------------------------------------------------- SwiGLU
SWIGLU_U = [1.0, -0.371, 37.5, 1e-30]
SWIGLU_DOUT = [0.75, -0.371]
SWIGLU_G_MAX = 2.0 ** 100
SWIGLU_PACKED_SHAPES = [(5, 16), (37, 528), (2304, 4096)]


def swiglu64(g, u, dout=None):
    """out, or (dg, du) when dout is given."""
    g, u = g.double(), u.double()
    s = torch.sigmoid(g)
    if dout is None:
        return g * s * u
    dout = dout.double()
    return dout * u * s * (1.0 + g * (1.0 - s)), dout * g * s


def swiglu32(g, u, dout=None):
    g, u = g.float(), u.float()
    if dout is None:
        return F.silu(g) * u
    s = torch.sigmoid(g)
    dout = dout.float()
    return dout * u * s * (1.0 + g * (1.0 - s)), dout * g * s


def swiglu_dg_floor(dout, u):
    return 2.0 ** -22 * (dout.double() * u.double()).abs()


def swiglu_flush_floor(g, mul):
    """out = g·sigmoid(g)·u and du = g·sigmoid(g)·dout: fp32 holds no
    sigmoid below 2^-126 (exp(-g) overflows at g < -88.7 and the quotient
    is 0), so the product is off by up to 2^-126·|g·mul| there. Anywhere
    else this is far below one ulp of the result."""
    return 2.0 ** -126 * (g.double() * mul.double()).abs()


# ----------------------------------------------------------------- RoPE
ROPE_SHAPES = [(2, 96, 3, 64), (1, 7, 1, 8), (2, 40, 2, 128),
               (2, 2048, 17, 64)]      # the last: 557 056 items > the cap
ROPE_TABLE_EXTRA = 5


def _rotate_half(x):
    half = x.shape[-1] // 2
    return torch.cat((-x[..., half:], x[..., :half]), dim=-1)


def _rope(x, cos, sin, bwd):
    S_ = x.shape[1]
    c = cos[:S_].to(x.dtype)[None, :, None, :]
    s = sin[:S_].to(x.dtype)[None, :, None, :]
    if bwd:
        return x * c - _rotate_half(x) * s
    return x * c + _rotate_half(x) * s


def rope64(x, cos, sin, bwd):
    """x [B, S, H, D]; fp32 tables [>= S, D] upcast to fp64."""
    return _rope(x.double(), cos, sin, bwd)


def rope32(x, cos, sin, bwd):
    return _rope(x.float(), cos, sin, bwd)


def rope_floor(x):
    x = x.double().abs()
    half = x.shape[-1] // 2
    return 2.0 ** -23 * (x + torch.cat((x[..., half:], x[..., :half]), -1))


# ------------------------------------------------------------------- CE
CE_SHAPES = [(2, 33, 1031), (2, 5, 7), (2, 5, 8), (1, 9, 4099),
             (1, 4, 50257), (3, 2741, 72), (4, 1, 64), (2, 9, 72)]
CE_ALL_IGNORED = (2, 9, 72)
CE_EPS = [0.0, 0.1]
CE_VARIANTS = ["n2", "n30", "neginf"]     # neginf with eps = 0 only
CE_DLOSS = 0.37


def ce_cases():
    return [(shape, eps, var) for shape in CE_SHAPES for eps in CE_EPS
            for var in CE_VARIANTS if not (var == "neginf" and eps != 0.0)]


def ce_case_name(shape, eps, var):
    return "ce_%dx%dx%d_eps%g_%s" % (*shape, eps, var)


def ce_shift(labels):
    """Label of each token: labels[b, s + 1], -100 at the last position."""
    out = torch.full_like(labels, -100)
    out[:, :-1] = labels[:, 1:]
    return out


def ce_inputs(shape, eps, var):
    """(logits bf16 [B, S, V], labels int64 [B, S]) on the CPU."""
    B, S_, V = shape
    g = case_generator(ce_case_name(shape, eps, var))
    mag = 30.0 if var == "n30" else 2.0
    logits = (torch.randn(B, S_, V, generator=g) * mag).bfloat16()
    labels = torch.randint(0, V, (B, S_), generator=g)
    labels[torch.rand(B, S_, generator=g) < 0.2] = -100
    if shape == CE_ALL_IGNORED:
        labels[:] = -100
    else:
        # labels on the first and last column, the last vector column and,
        # where the row has one, the first tail column
        forced = [0, V - 1]
        if V >= 8:
            forced.append(8 * (V // 8) - 1)
        if V % 8:
            forced.append(8 * (V // 8))
        for i, lab in enumerate(forced):
            if 1 + i < S_:
                labels[0, 1 + i] = lab
    if var == "neginf":
        drop = torch.rand(B, S_, V, generator=g) < 0.1
        lab = ce_shift(labels).clamp(min=0)
        drop.scatter_(2, lab[..., None], False)     # never the label
        logits[drop] = -math.inf
    return logits, labels


def _ce(x, labels, eps, dloss):
    """Shifted CE in x's dtype: lse [B, S] (0 at ignored tokens), per-token
    loss [B, S], loss, dlogits [B, S, V], n_valid."""
    V = x.shape[-1]
    lab = ce_shift(labels)
    valid = lab >= 0
    lse = torch.logsumexp(x, dim=-1)
    gold = x.gather(2, lab.clamp(min=0)[..., None]).squeeze(2)
    tok = lse - gold
    if eps != 0.0:
        tok = (1.0 - eps) * tok + eps * (lse - x.sum(-1) / V)
    zero = torch.zeros_like(lse)
    tok = torch.where(valid, tok, zero)
    n = int(valid.sum())
    loss = tok.sum() / max(n, 1)
    scale = dloss / max(n, 1)
    p = torch.exp(x - lse[..., None]) - eps / V
    onehot = torch.zeros_like(x).scatter_(2, lab.clamp(min=0)[..., None],
                                          1.0 - eps)
    dlogits = torch.where(valid[..., None], (p - onehot) * scale,
                          torch.zeros_like(x))
    return torch.where(valid, lse, zero), tok, loss, dlogits, n


def ce64(logits, labels, eps, dloss=CE_DLOSS):
    return _ce(logits.double(), labels, eps, dloss)


def ce32(logits, labels, eps, dloss=CE_DLOSS):
    return _ce(logits.float(), labels, eps, dloss)


def ce_tolerances(logits, labels, eps, dloss=CE_DLOSS):
    """fp64 reference and what it allows: dict with lse, loss, dlogits
    (fp64), tol_lse, tol_loss, dlogits_floor, n_valid, and the fp32
    formula's bf16 dlogits (for the CPU self-test)."""
    lse64, tok64, loss64, d64, n = ce64(logits, labels, eps, dloss)
    lse32, tok32, loss32, d32, _ = ce32(logits, labels, eps, dloss)
    tol_lse = fp32_tol(lse32, lse64)
    tol_loss = max(fp32_tol(loss32.reshape(1), loss64.reshape(1)),
                   fp32_tol(tok32, tok64))
    # dp = p·d(lse): the floor 2·tol_lse·scale, times the probability itself
    # (under the bare bound a dropped eps/V term passed wherever few tokens
    # are valid, scale being large there and p small)
    p64 = torch.exp(logits.double() - torch.logsumexp(logits.double(), -1,
                                                      keepdim=True))
    floor = 2.0 * tol_lse * abs(dloss) / max(n, 1) * p64
    return dict(lse=lse64, loss=loss64, dlogits=d64, n_valid=n,
                tol_lse=tol_lse, tol_loss=tol_loss, dlogits_floor=floor,
                dlogits32=d32.bfloat16())


# ---------------------------------------------------------------- AdamW
ADAMW_N = [1, 3, 4, 1027, 4352, 6291859]   # last: 4·(3·524288 + 100) + 3
ADAMW_BUFS = [("bf16", "bf16"), ("fp32", "fp32"), ("bf16", "none")]
# (grad_scale kind, step, weight_decay): every value of each, mixed
ADAMW_PARAMS = [("float", 0, 0.0), ("dev", 7, 0.1), ("float", 100000, 0.1),
                ("dev", 100000, 0.0)]
ADAMW_HYPER = dict(lr=6e-4, beta1=0.9, beta2=0.95, eps=1e-8)
ADAMW_SCALE = 1.0 / 3.0


def adamw_cases():
    return [(n, bufs, prm) for n in ADAMW_N for bufs in ADAMW_BUFS
            for prm in ADAMW_PARAMS
            if n < 1 << 20 or bufs == ("bf16", "bf16")]


ADAMW_POOL = 1027


def adamw_pool(n, grad_dtype):
    """p, m, v fp32 and g on the CPU, max(n, ADAMW_POOL) elements each. A
    case of n elements runs the first n; its fp32 tolerances come from the
    whole pool, because the largest error of one to four draws is no
    maximum: in half the draws it is under a quarter of an fp32 ulp, which
    no fp32 computation with another (equally valid) rounding order meets."""
    N = max(n, ADAMW_POOL)
    g_ = case_generator("adamw_%d" % n)
    p = torch.randn(N, generator=g_)
    m = (torch.rand(N, generator=g_) - 0.5) * 0.02
    v = torch.rand(N, generator=g_) * 0.001
    g = torch.randn(N, generator=g_).to(grad_dtype)
    return p, m, v, g


def _adamw(p, m, v, g, scale, step, wd, lr, beta1, beta2, eps):
    t = step + 1
    gf = g * scale
    m2 = beta1 * m + (1.0 - beta1) * gf
    v2 = beta2 * v + (1.0 - beta2) * gf * gf
    denom = v2.sqrt() / math.sqrt(1.0 - beta2 ** t) + eps
    p2 = p * (1.0 - lr * wd) - (lr / (1.0 - beta1 ** t)) * m2 / denom
    return p2, m2, v2


def adamw64(p, m, v, g, scale, step, wd, **hyper):
    """One AdamW step in fp64: the p, m, v a commit step stores (a tentative
    step writes this p to `out` and stores nothing). `scale` is the fp32
    grad scale as a Python float."""
    return _adamw(p.double(), m.double(), v.double(), g.double(), scale,
                  step, wd, **hyper)


def adamw32(p, m, v, g, scale, step, wd, **hyper):
    """The same step by torch_ref.fused_adamw_step in fp32."""
    from acco_amd.ops import torch_ref
    p, m, v = p.clone(), m.clone(), v.clone()
    torch_ref.fused_adamw_step(p, g, m, v, step, hyper["lr"], hyper["beta1"],
                               hyper["beta2"], hyper["eps"], wd,
                               grad_scale=scale, commit=True)
    return p, m, v


# --------------------------------------------------------------- colsum
COLSUM_CASES = [(1, 8, "bf16"), (3, 100, "bf16"), (513, 256 * 8 + 8, "bf16"),
                (5000, 24, "fp32"), (0, 64, "bf16"), (0, 64, "fp32")]


def colsum_input(P, D, dt):
    g = case_generator("colsum_%d_%d_%s" % (P, D, dt))
    x = torch.randn(P, D, generator=g)
    return x.bfloat16() if dt == "bf16" else x


def colsum64(x):
    return x.double().sum(0)


def colsum32(x):
    return x.float().sum(0)


# -------------------------------------------------------------- gemm_nt
GEMM_SHAPES = [(128, 128, 64), (256, 384, 192), (1024, 1152, 128)]


def gemm_inputs(M, N, K):
    g = case_generator("gemm_%d_%d_%d" % (M, N, K))
    return (torch.randn(M, K, generator=g).bfloat16(),
            torch.randn(N, K, generator=g).bfloat16())


def gemm64(A, B):
    return A.double() @ B.double().t()


def gemm32(A, B):
    return A.float() @ B.float().t()


def gemm_floor(A, B):
    K = A.shape[1]
    return K * 2.0 ** -24 * (A.double().abs() @ B.double().abs().t())
