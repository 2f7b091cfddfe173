"""ops.act_quantize_mxfp8 / ops.gemm_w4a8 on the GPU: the quantiser bit for
bit against torch_ref; the operand layouts of the block-scaled MFMA bit for
bit (every weight code and every activation code in every k slot); the kernel
against f = double(dequant(x_q)) . double(w^)^T + bias, x_q from torch_ref
(quantisation is an input, not an error), under the criterion of
test_gpu_linear_w4.check: within_half_ulp with the floor (K + 4) * 2^-24 *
(sum |x_q w^| + |bias|) and the same bits on a second call, at every edge of
the 64 x 256 tile and of the split of K; the routing of W4Linear(act_dtype);
and the prefill of both model families end to end.
MEASURED: RESULTS.md, "MXFP4 x MXFP8 GEMM"."""

import copy
import math

import pytest
import torch

from acco_amd import ops
from acco_amd.models import W4Linear, quantize_weights
from acco_amd.ops import torch_ref as R
from tests import test_gpu_decode_attention as TD
from tests import test_gpu_linear_w4 as T4
from tests.streaming_ref import case_generator, within_half_ulp
from tests.test_gemm_w4a8 import every_act_code, hand_blocks
from tests.test_gpu_gemm_wq import _prefill, e2e  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
DEV, FP8 = "cuda", torch.float8_e4m3fn
BM, BN, KT = 64, 256, 128
K_ONE, K_SHORT, K_EVEN = 128, 6272, 1024


@pytest.mark.parametrize("K", [128, 6272])
@pytest.mark.parametrize("M", [1, 3, 65])
def test_quantiser_bit_for_bit(M, K):
    g = case_generator("act_quant_%d_%d" % (M, K))
    h = torch.randn(M, 2, K, generator=g) * torch.logspace(-3, 3, M)[:, None,
                                                                     None]
    h = h.bfloat16()
    blocks = hand_blocks()[0]
    for i in range(len(blocks)):        # scattered over rows and blocks
        b = (5 * i) % (K // 32)
        h[i % M, :, 32 * b:32 * b + 32] = blocks[i]
    h = h.to(DEV)
    for x in (h[:, 0].contiguous(), h[:, 0]):
        got, want = ops.act_quantize_mxfp8(x), R.act_quantize_mxfp8(x)
        assert got[0].dtype == FP8 and got[0].shape == (M, K)
        assert torch.equal(got[1], want[1]), "scale bytes"
        assert torch.equal(got[0].view(torch.uint8), want[0].view(torch.uint8))


def test_every_weight_code_in_every_k_slot():
    """x = I, M = K = 512: 1.0 quantises exactly (256 * 2^-8), zero blocks
    take byte 127, so y[m, n] = w^[n, m] bit for bit under the code and scale
    patterns of test_gpu_gemm_wq: the B layout and both scale paths."""
    K = 512
    n, i = torch.arange(256)[:, None], torch.arange(K // 2)[None, :]
    codes = (((n + i) % 16) | (((n // 16 + 3 * i) % 16) << 4)).to(torch.uint8)
    scales = (7 + (37 * n + 101 * torch.arange(K // 32)[None, :]) % 241)
    codes, scales = codes.to(DEV), scales.to(torch.uint8).to(DEV)
    want = R.weight_dequantize_mxfp4(codes, scales, torch.bfloat16)
    assert ops.gemm_w4a8_tiles(K, 256, K)[::2] == (8, 2)
    y = ops.gemm_w4a8(torch.eye(K).bfloat16().to(DEV), codes, scales)
    assert torch.equal(TD._bits(y), TD._bits((want.t() + 0.0).bfloat16()))


def test_every_act_code_in_every_k_slot():
    """The mirror image: the weight is the MXFP4 identity (code 2 = 1.0, scale
    byte 127) and x holds every e4m3 code in every k slot under block scales
    that the quantiser recovers (test_gemm_w4a8.test_act_round_trip), so
    y == x bit for bit: the A layout and its scale path. -0 comes out +0."""
    K = 512
    x = every_act_code(K, K)[0].to(DEV)
    n = torch.arange(K)
    codes = torch.zeros(K, K // 2, dtype=torch.uint8)
    codes[n, n // 2] = (2 << (4 * (n % 2))).to(torch.uint8)
    scales = torch.full((K, K // 32), 127, dtype=torch.uint8)
    y = ops.gemm_w4a8(x, codes.to(DEV), scales.to(DEV))
    assert torch.equal(TD._bits(y), TD._bits(x + 0.0))


def check_tiles(M, N, K):
    """Each case is what it is meant to be."""
    mb, nb, n_split, k_chunk = ops.gemm_w4a8_tiles(M, N, K)
    assert (mb, nb) == (-(-M // BM), -(-N // BN)) and k_chunk % KT == 0
    assert (n_split - 1) * k_chunk < K <= n_split * k_chunk
    if K == K_ONE:
        assert n_split == 1
    elif K == K_SHORT:
        assert n_split > 1 and K % k_chunk != 0
    elif K == K_EVEN:
        assert n_split > 1 and K % k_chunk == 0
    return n_split


def check(run, x, codes, scales, bias, tag):
    K = x.shape[-1]
    xd = R.act_dequantize_mxfp8(*R.act_quantize_mxfp8(x), torch.float64)
    wd = R.weight_dequantize_mxfp4(codes, scales, torch.float64)
    bd = bias.double() if bias is not None else xd.new_zeros(len(wd))
    f = xd @ wd.t() + bd
    floor = (K + 4) * 2.0 ** -24 * (xd.abs() @ wd.abs().t() + bd.abs())
    y = run(x, codes, scales, bias)
    assert y.shape == f.shape and y.dtype == torch.bfloat16
    ratio, idx = within_half_ulp(y, f, floor)
    print("RATIO gemm_w4a8 %s M=%d N=%d K=%d bias=%d: %.4f"
          % (tag, x.shape[0], codes.shape[0], K, bias is not None, ratio))
    assert ratio <= 1.0, (tag, ratio, idx)
    assert torch.equal(TD._bits(y), TD._bits(run(x, codes, scales, bias))), \
        "same bits on every run"


@pytest.mark.parametrize("N", [1, BN - 1, BN + 1])
@pytest.mark.parametrize("M", [1, BM - 1, BM, BM + 1, 2 * BM + 3])
def test_gemm_kernel(M, N):
    """The largest ratio over these cases is in RESULTS.md; it is below 1
    with the floor's constant (K + 4) as it stands."""
    for K in (K_ONE, K_SHORT, K_EVEN):
        n_split = check_tiles(M, N, K)
        h, codes, scales, bias = T4.make(M, N, K, "w4a8")
        for x in (h[:, 0].contiguous(), h[:, 0]):
            for b in (None, bias):
                check(ops.gemm_w4a8, x, codes, scales, b,
                      "splits=%d stride=%d" % (n_split, x.stride(0)))


def test_module_dispatch(monkeypatch):
    spy = TD._Spy(ops.hip_ext())
    monkeypatch.setattr(ops, "hip_ext", lambda: spy)
    monkeypatch.setattr(ops, "W4A8_GEMM_MIN_ROWS", 65)
    h96, c96, s96, _ = T4.make(65, 17, 96, "w4a8_dispatch")
    assert torch.equal(ops.gemm_w4a8(h96[:, 0], c96, s96),
                       R.linear_w4a8(h96[:, 0], c96, s96))
    assert spy.calls == [], "K = 96 takes the reference"
    h, codes, scales, bias = T4.make(65, 257, 256, "w4a8_dispatch")
    a8, plain = W4Linear(codes, scales, bias, FP8), W4Linear(codes, scales,
                                                              bias)
    check(lambda x, *a: a8(x.unflatten(0, (5, 13))).flatten(0, 1), h[:, 0],
          codes, scales, bias, "module")
    assert spy.calls == ["act_quantize_mxfp8", "gemm_w4a8"] * 2, spy.calls
    spy.calls.clear()
    a8(h[:64, 0]), plain(h[:, 0])
    assert spy.calls == ["linear_w4", "gemm_w4"], spy.calls


def test_e2e_prefill(e2e, monkeypatch):  # noqa: F811
    """e <= 2 sqrt(e_full^2 + e_q^2), the criterion of test_gpu_gemm_wq; e_q
    is the fp64 CPU prefill of the act_dtype model, which goes through
    torch_ref.linear_w4a8, so the rounding of the activations is inside it."""
    model, ids, rms, e_full = e2e
    monkeypatch.setattr(ops, "W4A8_GEMM_MIN_ROWS", 65)
    qm = quantize_weights(model, dtype=T4.FP4, act_dtype=FP8)
    e_q = rms(_prefill(copy.deepcopy(qm).double(), ids))
    spy = TD._Spy(ops.hip_ext())
    monkeypatch.setattr(ops, "hip_ext", lambda: spy)
    got = rms(_prefill(copy.deepcopy(qm).to(DEV), ids.to(DEV)))
    assert "gemm_w4a8" in spy.calls and "gemm_w4" not in spy.calls
    bound = 2 * math.sqrt(e_full ** 2 + e_q ** 2)
    print("E2E gemm_w4a8 prefill rms %.4e e_full %.4e e_q %.4e bound %.4e"
          % (got, e_full, e_q, bound))
    assert e_full > 0 and e_q > 0 and got <= bound
