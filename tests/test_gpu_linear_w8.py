"""ops.linear_w8 on the GPU: the kernel against f = sum_k double(x) *
double(code) * double(scale) + double(bias) (quantisation is an input, not an
error) under within_half_ulp with the floor (K + 4) * 2^-24 * (scale *
sum_k |x * code| + |bias|): bf16 x e4m3 products are exact in fp32, any order
of K fp32 additions errs by at most K * 2^-24 of the absolute sum, and scale,
bias and the split combine add a few roundings. Then dequantisation and k
mapping bit for bit, the dispatch, and both model families end to end.
MEASURED: RESULTS.md, "FP8 weight-only decode linear"."""

import copy
import math
from unittest import mock

import pytest
import torch

from acco_amd import ops
from acco_amd.models import quantize_weights
from acco_amd.models.kv_cache import KVCache
from acco_amd.ops.torch_ref import weight_quantize
from tests import test_gpu_decode_attention as TD
from tests.kv_cache_ref import teacher_forced
from tests.streaming_ref import case_generator, ulp_bf16, within_half_ulp
from tests.test_gpu_kv_cache_fp8 import extend_tail

pytestmark = pytest.mark.gpu
DEV, FP8 = "cuda", torch.float8_e4m3fn
K_ONE, K_SHORT, K_MOST = 64, 6336, 4096     # what check_splits asks of them


def check_splits(M, N, K):
    n_split, k_chunk = ops.linear_w8_splits(M, N, K)
    assert (n_split - 1) * k_chunk < K <= n_split * k_chunk
    if K == K_ONE:
        assert n_split == 1
    elif K == K_SHORT:
        assert n_split > 1 and K % k_chunk != 0      # a short last split
    elif K == K_MOST:       # the cap of 64 splits, or what 16 M allows of it
        assert n_split == 64 if M <= 4 else n_split >= 4
    return n_split, k_chunk


# (n_split, k_chunk) as the grid function gave them when the two kernels were
# consolidated; rows M in PIN_M, columns N in PIN_N
PIN_M, PIN_N = (1, 16, 17, 64), (1, 128, 129, 4096, 14336)
PINNED = {
    K_ONE: [
        [(1, 64), (1, 64), (1, 64), (1, 64), (1, 64)],
        [(1, 64), (1, 64), (1, 64), (1, 64), (1, 64)],
        [(1, 64), (1, 64), (1, 64), (1, 64), (1, 64)],
        [(1, 64), (1, 64), (1, 64), (1, 64), (1, 64)],
    ],
    K_SHORT: [
        [(50, 128), (50, 128), (50, 128), (15, 448), (4, 1600)],
        [(20, 320), (20, 320), (20, 320), (15, 448), (4, 1600)],
        [(20, 320), (20, 320), (20, 320), (15, 448), (4, 1600)],
        [(6, 1088), (6, 1088), (6, 1088), (6, 1088), (4, 1600)],
    ],
    K_MOST: [
        [(64, 64), (64, 64), (64, 64), (16, 256), (4, 1024)],
        [(16, 256), (16, 256), (16, 256), (16, 256), (4, 1024)],
        [(13, 320), (13, 320), (13, 320), (13, 320), (4, 1024)],
        [(4, 1024), (4, 1024), (4, 1024), (4, 1024), (4, 1024)],
    ],
    69632: [
        [(64, 1088), (64, 1088), (64, 1088), (16, 4352), (4, 17408)],
        [(64, 1088), (64, 1088), (64, 1088), (16, 4352), (4, 17408)],
        [(64, 1088), (64, 1088), (64, 1088), (16, 4352), (4, 17408)],
        [(64, 1088), (64, 1088), (64, 1088), (16, 4352), (4, 17408)],
    ],
}


def test_splits_pinned():
    """The grid is a host function of its three sizes: a refactor keeps it."""
    for K, rows in PINNED.items():
        for M, row in zip(PIN_M, rows):
            for N, want in zip(PIN_N, row):
                assert ops.linear_w8_splits(M, N, K) == want, (M, N, K)


def make(M, N, K, name):
    g = case_generator("linear_w8_%s_%d_%d_%d" % (name, M, N, K))
    h = torch.randn(M, 2, K, generator=g).bfloat16().to(DEV)
    w = torch.randn(N, K, generator=g) * torch.logspace(-2, 1, N)[:, None]
    codes, scale = (t.to(DEV) for t in weight_quantize(w))
    return h, codes, scale, torch.randn(N, generator=g).bfloat16().to(DEV)


def check(run, x, codes, scale, bias, tag, extra_half_ulp=False):
    K = x.shape[-1]
    xd, cd, sd = x.double(), codes.float().double(), scale.double()
    bd = bias.double() if bias is not None else torch.zeros_like(sd)
    f = (xd @ cd.t()) * sd + bd
    floor = (K + 4) * 2.0 ** -24 * ((xd.abs() @ cd.abs().t()) * sd + bd.abs())
    if extra_half_ulp:      # the bf16 rounding of the unscaled product
        floor = floor + 0.5 * ulp_bf16(xd @ cd.t()) * sd
    y = run(x, codes, scale, bias)
    assert y.shape == f.shape and y.dtype == torch.bfloat16
    ratio, idx = within_half_ulp(y, f, floor)
    print("RATIO linear_w8 %s M=%d N=%d K=%d bias=%d: %.4f"
          % (tag, x.shape[0], codes.shape[0], K, bias is not None, ratio))
    assert ratio <= 1.0, (tag, ratio, idx)
    assert torch.equal(TD._bits(y), TD._bits(run(x, codes, scale, bias))), \
        "same bits on every run"


# beyond the issue's grid: x restaged in LDS with one, two and three M tiles
@pytest.mark.parametrize("M,N,Ks", [
    (M, N, (K_ONE, K_SHORT, K_MOST)) for M in (1, 15, 16, 17, 64)
    for N in (1, 17, 257, 1000)] + [(1, 17, (69632,)), (17, 17, (69632,)),
                                     (40, 257, (6464,))])
def test_linear_w8_kernel(M, N, Ks):
    for K in Ks:
        n_split, k_chunk = check_splits(M, N, K)
        if len(Ks) == 1:
            assert k_chunk > 1024 // ((M + 15) // 16)
        h, codes, scale, bias = make(M, N, K, "kernel")
        for x in (h[:, 0].contiguous(), h[:, 0]):
            for b in (None, bias):
                check(ops.hip_ext().linear_w8, x, codes, scale, b,
                      "splits=%d stride=%d" % (n_split, x.stride(0)))


def test_every_code_in_every_k_slot():
    """x = I: y[m, n] = code[n, m] * scale[n], exact in bf16, every byte in
    every k slot of both MFMA operands; -0 comes out as +0 (0 + -0)."""
    n, k = torch.arange(256)[:, None], torch.arange(64)[None, :]
    codes = ((n + 4 * k) % 256).to(torch.uint8)
    codes[codes % 128 == 127] = 0                  # the two NaN codes
    codes = codes.to(DEV).view(FP8)
    scale = torch.exp2(-(torch.arange(256) % 8).float()).to(DEV)
    y = ops.linear_w8(torch.eye(64).bfloat16().to(DEV), codes, scale)
    want = ((codes.float() * scale[:, None]).t() + 0.0).bfloat16()
    assert torch.equal(TD._bits(y), TD._bits(want))


def test_linear_w8_dispatch(monkeypatch):
    spy = TD._Spy(ops.hip_ext())
    monkeypatch.setattr(ops, "hip_ext", lambda: spy)

    def boom(*a, **k):
        raise AssertionError("torch reference reached inside the contract")
    monkeypatch.setattr(ops.torch_ref, "linear_w8", boom)
    h, codes, scale, bias = make(65, 257, 256, "dispatch")

    def op(x, *a):          # leading dims [3, 2] or [5, 13] flatten to M
        return ops.linear_w8(x.unflatten(0, (-1, 2 if len(x) == 6 else 13)),
                             *a).flatten(0, 1)
    check(op, h[:6, 0], codes, scale, bias, "kernel")
    assert spy.calls == ["linear_w8"] * 2, spy.calls
    check(op, h[:, 0], codes, scale, bias, "M=65 fallback", True)
    assert spy.calls == ["linear_w8"] * 2, spy.calls


def _logits(model, ids, cache_dtype):
    """(decode_step, extend, full-forward) logits on a `cache_dtype` cache."""
    alloc = KVCache.allocate.__func__
    with mock.patch.object(KVCache, "allocate", classmethod(
            lambda cls, *a, **k: alloc(cls, *a, **dict(k, dtype=cache_dtype)))):
        dec, full = teacher_forced(model, ids, TD.E2E_PREFIX, TD.E2E_S)
        return dec, extend_tail(model, ids, TD.E2E_PREFIX, TD.E2E_S), full


@pytest.fixture(scope="module", params=["llama", "gptneo"])
def e2e(request):
    """rms errors against the fp64 CPU forward of the bf16 GPU forward (full),
    the fp64 CPU quantised model (w8) and the fp64 CPU model on an fp8 cache
    (kv), the last two per path (decode_step, extend); computed once."""
    model = TD._e2e_model(request.param)
    ids = torch.randint(0, 512, (len(TD.E2E_PREFIX), TD.E2E_S),
                        generator=torch.Generator().manual_seed(5))
    qm, m64 = quantize_weights(model), copy.deepcopy(model).double()
    ref = _logits(m64, ids, None)[2]

    def rms(a):
        return float((a.cpu() - ref).pow(2).mean().sqrt())
    err = dict(full=rms(_logits(copy.deepcopy(model).to(DEV), ids.to(DEV),
                                None)[2]),
               w8=[rms(a) for a in _logits(copy.deepcopy(qm).double(), ids,
                                           None)[:2]],
               kv=[rms(a) for a in _logits(m64, ids, FP8)[:2]])
    return request.param, copy.deepcopy(qm).to(DEV), ids.to(DEV), rms, err


@pytest.mark.parametrize("kv", [None, FP8], ids=["kv_bf16", "kv_fp8"])
def test_e2e_w8(e2e, kv):
    """e_w8 <= 2 sqrt(e_full^2 + e_q^2 (+ e_kv^2 on an fp8 cache)), the
    criterion and the reasoning of test_e2e_fp8_cache."""
    family, gpu_q, ids, rms, err = e2e
    got = _logits(gpu_q, ids, kv)[:2]
    for i, tag in enumerate(("decode_step", "extend")):
        terms = [err["full"], err["w8"][i]] + ([err["kv"][i]] if kv else [])
        bound = 2 * math.sqrt(sum(t * t for t in terms))
        print("E2E w8 %s %s %s rms %.4e terms %s bound %.4e"
              % (family, tag, "kv_fp8" if kv else "kv_bf16", rms(got[i]),
                 ["%.4e" % t for t in terms], bound))
        assert all(t > 0 for t in terms) and rms(got[i]) <= bound, tag
