"""ops.linear_w4 on the GPU: the kernel against f = sum_k double(x) *
double(w^) + double(bias), w^ the dequantised MXFP4 weight (quantisation is an
input, not an error), under within_half_ulp with the floor (K + 4) * 2^-24 *
(sum_k |x * w^| + |bias|): bf16 x (e2m1 * 2^e) products are exact in fp32, any
order of K fp32 additions errs by at most K * 2^-24 of the absolute sum, and
bias and the split combine add a few roundings. Then the convert and the k
mapping bit for bit, the dispatch, and both model families end to end.
MEASURED: RESULTS.md, "MXFP4 weight-only decode linear"."""

import copy
import math

import pytest
import torch

from acco_amd import ops
from acco_amd.models import quantize_weights
from acco_amd.ops.torch_ref import (weight_dequantize_mxfp4,
                                    weight_quantize_mxfp4)
from tests import test_gpu_decode_attention as TD
from tests.streaming_ref import case_generator, ulp_bf16, within_half_ulp
from tests.test_gpu_linear_w8 import _logits

pytestmark = pytest.mark.gpu
DEV, FP4 = "cuda", torch.float4_e2m1fn_x2
K_ONE, K_SHORT, K_MOST = 128, 6272, 32768    # what check_splits asks of them


def check_splits(M, N, K):
    n_split, k_chunk = ops.linear_w4_splits(M, N, K)
    assert (n_split - 1) * k_chunk < K <= n_split * k_chunk
    assert k_chunk % 512 == 0
    if K == K_ONE:
        assert n_split == 1
    elif K == K_SHORT:      # a short last split that ends inside a super-step
        assert n_split > 1 and K % k_chunk % 512 != 0
    elif K == K_MOST:       # the cap of 64 splits, or what 32 M allows of it
        assert n_split == 64 if M <= 16 else n_split >= 4
    return n_split, k_chunk


# (n_split, k_chunk) as the grid function gave them when the two kernels were
# consolidated; rows M in PIN_M, columns N in PIN_N
PIN_M, PIN_N = (1, 16, 17, 64), (1, 128, 129, 4096, 14336)
PINNED = {
    K_ONE: [
        [(1, 512), (1, 512), (1, 512), (1, 512), (1, 512)],
        [(1, 512), (1, 512), (1, 512), (1, 512), (1, 512)],
        [(1, 512), (1, 512), (1, 512), (1, 512), (1, 512)],
        [(1, 512), (1, 512), (1, 512), (1, 512), (1, 512)],
    ],
    K_SHORT: [
        [(13, 512), (13, 512), (13, 512), (13, 512), (4, 2048)],
        [(7, 1024), (7, 1024), (7, 1024), (7, 1024), (4, 2048)],
        [(7, 1024), (7, 1024), (7, 1024), (7, 1024), (4, 2048)],
        [(3, 2560), (3, 2560), (3, 2560), (3, 2560), (3, 2560)],
    ],
    K_MOST: [
        [(64, 512), (64, 512), (64, 512), (16, 2048), (4, 8192)],
        [(64, 512), (64, 512), (64, 512), (16, 2048), (4, 8192)],
        [(32, 1024), (32, 1024), (32, 1024), (16, 2048), (4, 8192)],
        [(16, 2048), (16, 2048), (16, 2048), (16, 2048), (4, 8192)],
    ],
    69632: [
        [(46, 1536), (46, 1536), (46, 1536), (16, 4608), (4, 17408)],
        [(46, 1536), (46, 1536), (46, 1536), (16, 4608), (4, 17408)],
        [(46, 1536), (46, 1536), (46, 1536), (16, 4608), (4, 17408)],
        [(34, 2048), (34, 2048), (34, 2048), (16, 4608), (4, 17408)],
    ],
}


def test_splits_pinned():
    """The grid is a host function of its three sizes: a refactor keeps it."""
    for K, rows in PINNED.items():
        for M, row in zip(PIN_M, rows):
            for N, want in zip(PIN_N, row):
                assert ops.linear_w4_splits(M, N, K) == want, (M, N, K)


def make(M, N, K, name):
    g = case_generator("linear_w4_%s_%d_%d_%d" % (name, M, N, K))
    h = torch.randn(M, 2, K, generator=g).bfloat16().to(DEV)
    w = torch.randn(N, K, generator=g) * torch.logspace(-2, 1, N)[:, None]
    codes, scales = weight_quantize_mxfp4(w.to(DEV))
    return h, codes, scales, torch.randn(N, generator=g).bfloat16().to(DEV)


def check(run, x, codes, scales, bias, tag, extra_half_ulp=False):
    K = x.shape[-1]
    xd, wd = x.double(), weight_dequantize_mxfp4(codes, scales, torch.float64)
    bd = bias.double() if bias is not None else xd.new_zeros(len(wd))
    f = xd @ wd.t() + bd
    floor = (K + 4) * 2.0 ** -24 * (xd.abs() @ wd.abs().t() + bd.abs())
    if extra_half_ulp:      # the bf16 rounding of the product before the bias
        floor = floor + 0.5 * ulp_bf16(xd @ wd.t())
    y = run(x, codes, scales, bias)
    assert y.shape == f.shape and y.dtype == torch.bfloat16
    ratio, idx = within_half_ulp(y, f, floor)
    print("RATIO linear_w4 %s M=%d N=%d K=%d bias=%d: %.4f"
          % (tag, x.shape[0], codes.shape[0], K, bias is not None, ratio))
    assert ratio <= 1.0, (tag, ratio, idx)
    assert torch.equal(TD._bits(y), TD._bits(run(x, codes, scales, bias))), \
        "same bits on every run"


# beyond the issue's grid: x restaged in LDS with one, two and three M tiles
@pytest.mark.parametrize("M,N,Ks", [
    (M, N, (K_ONE, K_SHORT, K_MOST)) for M in (1, 15, 16, 17, 64)
    for N in (1, 17, 257)] + [(1, 17, (69632,)), (17, 17, (69632,)),
                              (40, 257, (6272,))])
def test_linear_w4_kernel(M, N, Ks):
    for K in Ks:
        n_split, k_chunk = check_splits(M, N, K)
        if len(Ks) == 1:        # more than one slice of x per workgroup
            assert k_chunk > (1024 if M <= 16 else 512)
        h, codes, scales, bias = make(M, N, K, "kernel")
        for x in (h[:, 0].contiguous(), h[:, 0]):
            for b in (None, bias):
                check(ops.hip_ext().linear_w4, x, codes, scales, b,
                      "splits=%d stride=%d" % (n_split, x.stride(0)))


def test_every_code_in_every_k_slot():
    """x = I: y[m, n] = w^[n, m], exact in bf16. Over 256 rows every nibble
    value lands in both nibble positions of every byte, so in every k slot of
    every MFMA, under scale bytes that differ from block to block; -0 comes
    out as +0 (0 + -0)."""
    K = 512
    n, i = torch.arange(256)[:, None], torch.arange(K // 2)[None, :]
    codes = (((n + i) % 16) | (((n // 16 + 3 * i) % 16) << 4)).to(torch.uint8)
    scales = (7 + (37 * n + 101 * torch.arange(K // 32)[None, :]) % 241)
    codes, scales = codes.to(DEV), scales.to(torch.uint8).to(DEV)
    eye = torch.eye(K).bfloat16().to(DEV)
    want = (weight_dequantize_mxfp4(codes, scales, torch.bfloat16).t()
            + 0.0).contiguous()
    for m0 in range(0, K, 64):
        y = ops.linear_w4(eye[m0:m0 + 64], codes, scales)
        assert torch.equal(TD._bits(y), TD._bits(want[m0:m0 + 64])), m0


def test_linear_w4_dispatch(monkeypatch):
    spy = TD._Spy(ops.hip_ext())
    monkeypatch.setattr(ops, "hip_ext", lambda: spy)
    h, codes, scales, bias = make(65, 257, 256, "dispatch")
    h96, c96, s96, _ = make(3, 17, 96, "dispatch")
    assert torch.equal(ops.linear_w4(h96[:, 0], c96, s96),
                       ops.torch_ref.linear_w4(h96[:, 0], c96, s96))
    assert spy.calls == [], "K = 96 takes the reference"

    def boom(*a, **k):
        raise AssertionError("torch reference reached inside the contract")
    monkeypatch.setattr(ops.torch_ref, "linear_w4", boom)

    def op(x, *a):          # leading dims [., 2] or [5, 13] flatten to M
        return ops.linear_w4(x.unflatten(0, (-1, 13 if len(x) == 65 else 2)),
                             *a).flatten(0, 1)
    check(op, h[:6, 0], codes, scales, bias, "kernel")
    check(op, h[:64, 0], codes, scales, None, "M=64 kernel")
    assert spy.calls == ["linear_w4"] * 4, spy.calls
    check(op, h[:, 0], codes, scales, bias, "M=65 fallback", True)
    assert spy.calls == ["linear_w4"] * 4, spy.calls


@pytest.fixture(scope="module", params=["llama", "gptneo"])
def e2e(request):
    """rms errors against the fp64 CPU forward of the bf16 GPU forward (full)
    and of the fp64 CPU quantised model (w4) per path (decode_step, extend);
    computed once."""
    model = TD._e2e_model(request.param)
    ids = torch.randint(0, 512, (len(TD.E2E_PREFIX), TD.E2E_S),
                        generator=torch.Generator().manual_seed(5))
    qm, m64 = quantize_weights(model, dtype=FP4), copy.deepcopy(model).double()
    ref = _logits(m64, ids, None)[2]

    def rms(a):
        return float((a.cpu() - ref).pow(2).mean().sqrt())
    err = dict(full=rms(_logits(copy.deepcopy(model).to(DEV), ids.to(DEV),
                                None)[2]),
               w4=[rms(a) for a in _logits(copy.deepcopy(qm).double(), ids,
                                           None)[:2]])
    return request.param, copy.deepcopy(qm).to(DEV), ids.to(DEV), rms, err


def test_e2e_w4(e2e):
    """e_w4 <= 2 sqrt(e_full^2 + e_q^2), the criterion and the reasoning of
    test_e2e_w8."""
    family, gpu_q, ids, rms, err = e2e
    got = _logits(gpu_q, ids, None)[:2]
    for i, tag in enumerate(("decode_step", "extend")):
        terms = [err["full"], err["w4"][i]]
        bound = 2 * math.sqrt(sum(t * t for t in terms))
        print("E2E w4 %s %s rms %.4e terms %s bound %.4e"
              % (family, tag, rms(got[i]), ["%.4e" % t for t in terms], bound))
        assert all(t > 0 for t in terms) and rms(got[i]) <= bound, tag
