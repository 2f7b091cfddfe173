"""ops.gemm_w8 / ops.gemm_w4 on the GPU, both formats through the same tests:
the kernel against fp64 under the criterion of test_gpu_linear_w8.py /
test_gpu_linear_w4.py (their `check`: within_half_ulp with the floor
(K + 4) * 2^-24 * (sum |x w^| + |bias|), whose derivation holds for any
summation order, and the same bits on a second call), at every edge of the
64 x 256 tile and of the split of K; the convert and the k mapping bit for
bit across row blocks; the routing of W8Linear / W4Linear; and the prefill of
both model families end to end.
MEASURED: RESULTS.md, "Tiled quantised GEMMs"."""

import copy
import math

import pytest
import torch

from acco_amd import ops
from acco_amd.models import W4Linear, W8Linear, quantize_weights
from acco_amd.models.kv_cache import KVCache
from acco_amd.ops.torch_ref import weight_dequantize_mxfp4
from tests import test_gpu_decode_attention as TD
from tests import test_gpu_linear_w4 as T4
from tests import test_gpu_linear_w8 as T8

pytestmark = pytest.mark.gpu
DEV = "cuda"
BM, BN, KT = 64, 256, 128
# per format: the skinny tests' module (make, check), the module class, the
# quantize_weights dtype, and K of one step / K_SHORT / even splits
FMT = {"w8": (T8, W8Linear, T8.FP8, (64, 6464, 1024)),
       "w4": (T4, W4Linear, T4.FP4, (128, 6272, 1024))}
fmts = pytest.mark.parametrize("fmt", list(FMT))


def check_tiles(fmt, M, N, K):
    """Each case is what it is meant to be."""
    mb, nb, n_split, k_chunk = getattr(ops, "gemm_%s_tiles" % fmt)(M, N, K)
    assert (mb, nb) == (-(-M // BM), -(-N // BN)) and k_chunk % KT == 0
    assert (n_split - 1) * k_chunk < K <= n_split * k_chunk
    k_one, k_short, k_even = FMT[fmt][3]
    if K == k_one:
        assert n_split == 1
    elif K == k_short:      # a short last split; fp8's ends inside a slice
        assert n_split > 1 and K % k_chunk != 0
        assert (K % k_chunk % KT != 0) == (fmt == "w8")
    elif K == k_even:
        assert n_split > 1 and K % k_chunk == 0
    return n_split


@fmts
@pytest.mark.parametrize("N", [1, BN - 1, BN + 1])
@pytest.mark.parametrize("M", [1, BM - 1, BM, BM + 1, 2 * BM + 3])
def test_gemm_kernel(fmt, M, N):
    T = FMT[fmt][0]
    for K in FMT[fmt][3]:
        n_split = check_tiles(fmt, M, N, K)
        h, codes, scale, bias = T.make(M, N, K, "gemm")
        for x in (h[:, 0].contiguous(), h[:, 0]):
            for b in (None, bias):
                T.check(getattr(ops.hip_ext(), "gemm_" + fmt), x, codes, scale,
                        b, "gemm splits=%d stride=%d" % (n_split, x.stride(0)))


@fmts
def test_every_code_in_every_k_slot(fmt):
    """x = I, M = K = 512 in one call: y[m, n] = w^[n, m], exact in bf16,
    with the code and scale patterns of the skinny tests: every code in every
    k slot of the MFMAs, across eight row blocks and two splits; -0 comes out
    as +0 (0 + -0)."""
    K = 512
    n = torch.arange(256)[:, None]
    if fmt == "w8":
        codes = ((n + 4 * torch.arange(K)[None, :]) % 256).to(torch.uint8)
        codes[codes % 128 == 127] = 0                  # the two NaN codes
        codes = codes.to(DEV).view(T8.FP8)
        scale = torch.exp2(-(torch.arange(256) % 8).float()).to(DEV)
        want = codes.float() * scale[:, None]
    else:
        i = torch.arange(K // 2)[None, :]
        codes = (((n + i) % 16) | (((n // 16 + 3 * i) % 16) << 4))
        scale = (7 + (37 * n + 101 * torch.arange(K // 32)[None, :]) % 241)
        codes = codes.to(torch.uint8).to(DEV)
        scale = scale.to(torch.uint8).to(DEV)
        want = weight_dequantize_mxfp4(codes, scale, torch.bfloat16)
    assert getattr(ops, "gemm_%s_tiles" % fmt)(K, 256, K)[::2] == (8, 2)
    y = getattr(ops, "gemm_" + fmt)(torch.eye(K).bfloat16().to(DEV), codes,
                                    scale)
    assert torch.equal(TD._bits(y), TD._bits((want.t() + 0.0).bfloat16()))


@fmts
def test_module_dispatch(fmt, monkeypatch):
    T, cls = FMT[fmt][:2]
    spy = TD._Spy(ops.hip_ext())
    monkeypatch.setattr(ops, "hip_ext", lambda: spy)
    h96, c96, s96, _ = T.make(65, 17, 96, "gemm_dispatch")
    ref = getattr(ops.torch_ref, "linear_" + fmt)
    assert torch.equal(getattr(ops, "gemm_" + fmt)(h96[:, 0], c96, s96),
                       ref(h96[:, 0], c96, s96))
    assert spy.calls == [], "K = 96 takes the reference"

    def boom(*a, **k):
        raise AssertionError("torch reference reached inside the contract")
    monkeypatch.setattr(ops.torch_ref, "linear_" + fmt, boom)
    h, codes, scale, bias = T.make(65, 257, 256, "gemm_dispatch")

    def module(x, codes, scale, bias):    # leading dims [32, 2] or [5, 13]
        return cls(codes, scale, bias)(
            x.unflatten(0, (-1, 13 if len(x) == 65 else 2))).flatten(0, 1)
    T.check(module, h[:64, 0], codes, scale, bias, "module M=64")
    assert spy.calls == ["linear_" + fmt] * 2, spy.calls
    spy.calls.clear()
    T.check(module, h[:, 0], codes, scale, bias, "module M=65")
    assert spy.calls == ["gemm_" + fmt] * 2, spy.calls


def _prefill(model, ids):
    cache = KVCache.allocate(model, len(ids), TD.E2E_S)
    width = max(TD.E2E_PREFIX)
    lens = torch.tensor(TD.E2E_PREFIX, dtype=torch.int32, device=ids.device)
    return model.prefill(ids[:, :width], lens, cache).double().cpu()


@pytest.fixture(scope="module", params=["llama", "gptneo"])
def e2e(request):
    """The prefill logits in fp64 on the CPU and e_full, the rms error of the
    bf16 GPU prefill against them; computed once per family."""
    model = TD._e2e_model(request.param)
    ids = torch.randint(0, 512, (len(TD.E2E_PREFIX), TD.E2E_S),
                        generator=torch.Generator().manual_seed(5))
    ref = _prefill(copy.deepcopy(model).double(), ids)

    def rms(a):
        return float((a - ref).pow(2).mean().sqrt())
    return model, ids, rms, rms(_prefill(copy.deepcopy(model).to(DEV),
                                         ids.to(DEV)))


@fmts
def test_e2e_prefill(e2e, fmt, monkeypatch):
    """e <= 2 sqrt(e_full^2 + e_q^2), the criterion and the reasoning of
    test_e2e_w8; e_q is the fp64 CPU prefill of the quantised model. The
    padded prompt is more than 64 rows: every projection takes the GEMM."""
    model, ids, rms, e_full = e2e
    qm = quantize_weights(model, dtype=FMT[fmt][2])
    e_q = rms(_prefill(copy.deepcopy(qm).double(), ids))
    spy = TD._Spy(ops.hip_ext())
    monkeypatch.setattr(ops, "hip_ext", lambda: spy)
    got = rms(_prefill(copy.deepcopy(qm).to(DEV), ids.to(DEV)))
    assert "gemm_" + fmt in spy.calls
    bound = 2 * math.sqrt(e_full ** 2 + e_q ** 2)
    print("E2E gemm_%s prefill rms %.4e e_full %.4e e_q %.4e bound %.4e"
          % (fmt, got, e_full, e_q, bound))
    assert e_full > 0 and e_q > 0 and got <= bound
