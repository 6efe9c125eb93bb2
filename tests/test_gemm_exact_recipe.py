"""The data recipe of tests/test_gpu_gemm_views.py and tests/test_gpu_grouped_views.py, checked
from the inputs alone (no GPU).

Those tests compare every GEMM route bitwise with an fp64 reference.  That is only sound
if the fp32 result is exact whatever the summation order, and it only bites if the bf16
rounding is really exercised: most expected outputs must need rounding, and some must be
exact ties between two bf16 neighbours, where round-to-nearest-even differs from both
round-half-away and truncation.  These are conditions on the inputs, asserted here for
every (K, R) the GPU module uses; they measure nothing of the kernels.
"""
import pytest
import torch

import test_gpu_gemm_views
import test_gpu_grouped_views
from test_gpu_gemm_views import SWIGLU_R, _framed, _int_values, _ints, _out_frame, _rmax, SENTINEL

# every (K, R) of both modules whose output is rounded to bf16; the grouped weight gradient's
# reduction lengths (the experts' row counts) have fp32 outputs only
RECIPE_KR = sorted(set(test_gpu_gemm_views.RECIPE_KR) | set(test_gpu_grouped_views.RECIPE_KR))
RECIPE_FP32_ONLY = sorted(set(test_gpu_grouped_views.RECIPE_TN_RED) - set(RECIPE_KR))

M, N = 96, 80


def _operands(K, R):
    ga, gb = torch.Generator().manual_seed(1000 + K), torch.Generator().manual_seed(2000 + K)
    return _ints((M, K), R, ga), _ints((N, K), R, gb)


def test_recipe_covers_the_issue_lengths():
    ks = {k for k, _ in RECIPE_KR}
    assert {8, 72, 200, 64, 192, 256, 96, 128, 384, 320, 7, 1000} <= ks
    assert all(R == (SWIGLU_R if R < 64 else 64) for _, R in RECIPE_KR)
    assert all(K * R * R <= 2 ** 23 for K, R in RECIPE_KR)
    assert set(test_gpu_gemm_views.RECIPE_KR) <= set(RECIPE_KR)
    # the grouped module: the register-loop gate, and the experts' row counts as reduction lengths
    assert {(72, SWIGLU_R), (136, SWIGLU_R), (136, 64)} <= set(RECIPE_KR)
    assert {1, 7, 50, 70, 127, 129, 320} <= {k for k, _ in test_gpu_grouped_views.RECIPE_TN_RED}
    assert all(R == 64 and K * R * R <= 2 ** 23 for K, R in test_gpu_grouped_views.RECIPE_TN_RED)


@pytest.mark.parametrize("K,R", RECIPE_KR)
def test_operands_survive_bf16(K, R):
    g1, g2 = torch.Generator().manual_seed(K), torch.Generator().manual_seed(K)
    iv = _int_values((M, K), R, g1)
    bv = _ints((M, K), R, g2)
    assert bv.dtype == torch.bfloat16
    assert torch.equal(bv.to(torch.int32), iv)                       # the same integers, exactly
    assert torch.equal(bv.float().to(torch.bfloat16), bv)            # a bf16 round trip changes nothing
    assert int(iv.min()) >= -R and int(iv.max()) <= R and R <= _rmax(K)
    assert int(iv.min()) == -R and int(iv.max()) == R                # the whole range is used


@pytest.mark.parametrize("K,R", RECIPE_KR + RECIPE_FP32_ONLY)
def test_fp32_product_is_exact_in_any_order(K, R):
    a, b = _operands(K, R)
    exact = a.double() @ b.double().T
    assert float(exact.abs().max()) < 2 ** 23
    g = torch.Generator().manual_seed(K + 7)
    for _ in range(2):
        p = torch.randperm(K, generator=g)
        y = a[:, p].float() @ b[:, p].float().T
        assert torch.equal(y.double(), exact)
    # partial sums taken apart and joined again (split-K), and the alpha = 0.5 half-integers
    h = K // 2
    y = 0.5 * (a[:, :h].float() @ b[:, :h].float().T) + 0.5 * (a[:, h:].float() @ b[:, h:].float().T)
    assert torch.equal(y.double(), 0.5 * exact)


@pytest.mark.parametrize("K,R", [kr for kr in RECIPE_KR if kr[1] == 64])
def test_bf16_rounding_is_exercised(K, R):
    """(The R = 2 operands of the SwiGLU cases keep |h| small on purpose: their h is exact in
    bf16 and those cases test the gate, so they are left out here.)"""
    a, b = _operands(K, R)
    exact = (a.double() @ b.double().T).float()
    rounded = exact.to(torch.bfloat16)
    assert float((rounded.float() != exact).float().mean()) >= 0.5
    low = exact.view(torch.int32) & 0xFFFF
    ties = low == 0x8000
    assert int(ties.sum()) >= 1
    # at a tie RNE picks the even neighbour: truncation and round-half-away each differ somewhere
    bits = exact.view(torch.int32)
    trunc = (bits & ~0xFFFF).view(torch.float32)
    away = ((bits + 0x8000) & ~0xFFFF).view(torch.float32)
    assert bool((rounded.float() != trunc).any()) and bool((rounded.float()[ties] != away[ties]).any())


def test_frames():
    buf, v = _framed(5, 16, torch.float32, SENTINEL, 3, 3, 8, 8, device="cpu")
    assert buf.shape == (11, 32) and v.shape == (5, 16) and v.storage_offset() == 3 * 32 + 8
    assert bool((buf == SENTINEL).all())
    for dt, es in ((torch.float32, 4), (torch.bfloat16, 2)):
        for cols in (5, 8, 69, 72, 261):
            _, v = _framed_cpu(cols, dt, "aligned")
            assert (v.storage_offset() * es) % 16 == 0 and (v.stride(0) * es) % 16 == 0 and v.stride(0) >= cols + 16
            _, v = _framed_cpu(cols, dt, "off1")
            assert (v.storage_offset() * es) % 16 == es and v.stride(0) % 8 == 0
            _, v = _framed_cpu(cols, dt, "oddld")
            assert (v.storage_offset() * es) % 16 == 0 and v.stride(0) % 2 == 1


def _framed_cpu(cols, dt, how):
    return _out_frame(4, cols, dt, how, device="cpu")
