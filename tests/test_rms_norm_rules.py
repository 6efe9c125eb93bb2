"""What the RMSNorm ops decide without a GPU:

* ``ops.rms_norm_validate``: what it accepts (contiguous operands, row views, column slices of a
  wider buffer, ``h`` over ``x`` or ``residual``) and every refusal;
* the fp64 mirrors ``ops.rms_norm_reference`` / ``ops.rms_norm_backward_reference`` against
  ``F.rms_norm`` in fp64 and autograd through it;
* ``ops.rms_norm_row_chunk`` against the rule of csrc/device/rmsnorm.hpp;
* ``LlamaConfig.norm``.
"""
import re
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

from collective_communication_mpi_amd import ops
from collective_communication_mpi_amd.parallel.llama_dp import NORM_KINDS, LlamaBlock, LlamaConfig

BF = torch.bfloat16
HEADER = Path(ops.__file__).resolve().parents[1] / "csrc" / "device" / "rmsnorm.hpp"


def _rows(T, d, seed=0):
    return torch.randn(T, d, generator=torch.Generator().manual_seed(seed)).to(BF)


def _weight(d, dtype=BF, seed=9):
    return (0.5 + torch.rand(d, generator=torch.Generator().manual_seed(seed))).to(dtype)


def test_validate_accepts_contiguous_operands_views_and_the_aliasing_forms():
    T, d = 5, 136
    x, r, w = _rows(T, d), _rows(T, d, 1), _weight(d)
    assert ops.rms_norm_validate(x, w) == (T, d)
    assert ops.rms_norm_validate(x, _weight(d, torch.float32), r, 1e-6) == (T, d)
    wide = _rows(2 * T, 3 * d + 8, 2)
    rows = wide[1::2]            # a row view: every other row
    cols = wide[:T, d:2 * d]     # a column slice of a wider buffer
    assert rows[:, :d].stride(0) == 2 * (3 * d + 8) and cols.stride(0) == 3 * d + 8
    assert ops.rms_norm_validate(rows[:, :d], w, cols, 1e-5, h=torch.empty(T, d, dtype=BF), y=wide[T:, 8:8 + d]) == (T, d)
    assert ops.rms_norm_validate(x, w, r, 1e-5, h=x) == (T, d)   # h over x
    assert ops.rms_norm_validate(x, w, r, 1e-5, h=r) == (T, d)   # h over residual
    assert ops.rms_norm_validate(cols, w, r, 1e-5, h=cols) == (T, d)
    one = wide[3:4, 8:8 + d]     # one row: its row stride is never used
    assert ops.rms_norm_validate(one, w) == (1, d)
    for dd in (8, 16384):
        assert ops.rms_norm_validate(_rows(1, dd), _weight(dd)) == (1, dd)


def test_validate_refusals():
    T, d = 5, 64
    x, r, w = _rows(T, d), _rows(T, d, 1), _weight(d)
    flat = _rows(1, T * (d + 8), 3).view(-1)
    for call in (lambda: ops.rms_norm_validate(x.float(), w),
                 lambda: ops.rms_norm_validate(x, w.double()),
                 lambda: ops.rms_norm_validate(x, w.half()),
                 lambda: ops.rms_norm_validate(x, w, r.float()),
                 lambda: ops.rms_norm_validate(x, w, r, 1e-5, h=x.float()),
                 lambda: ops.rms_norm_validate(x, w, y=x.float()),
                 lambda: ops.rms_norm_validate(None, w)):
        with pytest.raises(TypeError, match="rms_norm"):
            call()
    refused = {
        "d % 8 != 0": lambda: ops.rms_norm_validate(_rows(T, 12), _weight(12)),
        "d = 0": lambda: ops.rms_norm_validate(torch.empty(T, 0, dtype=BF), torch.empty(0, dtype=BF)),
        "d = 16392": lambda: ops.rms_norm_validate(_rows(1, 16392), _weight(16392)),
        "T = 0": lambda: ops.rms_norm_validate(torch.empty(0, d, dtype=BF), w),
        "three dimensions": lambda: ops.rms_norm_validate(x[None], w),
        "row stride % 8": lambda: ops.rms_norm_validate(flat[:T * (d + 4)].view(T, d + 4)[:, :d], w),
        "misaligned base": lambda: ops.rms_norm_validate(flat[4:4 + T * d].view(T, d), w),
        "column stride 2": lambda: ops.rms_norm_validate(_rows(T, 2 * d)[:, ::2], w),
        "residual shape": lambda: ops.rms_norm_validate(x, w, r[:-1]),
        "residual width": lambda: ops.rms_norm_validate(x, w, _rows(T, 2 * d)[:, :d + 8]),
        "y shape": lambda: ops.rms_norm_validate(x, w, y=_rows(T + 1, d)),
        "h shape": lambda: ops.rms_norm_validate(x, w, r, 1e-5, h=_rows(T, d + 8)),
        "h without residual": lambda: ops.rms_norm_validate(x, w, None, 1e-5, h=_rows(T, d)),
        "h at x with other strides": lambda: (lambda b: ops.rms_norm_validate(b[::2], w, r, 1e-5, h=b[:T]))(_rows(2 * T, d)),
        "weight shape": lambda: ops.rms_norm_validate(x, _weight(d + 8)),
        "weight [1, d]": lambda: ops.rms_norm_validate(x, w[None]),
        "non-contiguous weight": lambda: ops.rms_norm_validate(x, _weight(2 * d)[::2]),
        "misaligned weight": lambda: ops.rms_norm_validate(x, _weight(d + 8)[4:4 + d]),
        "eps = 0": lambda: ops.rms_norm_validate(x, w, None, 0.0),
        "eps < 0": lambda: ops.rms_norm_validate(x, w, None, -1e-5),
        "eps rounds to 0 in fp32": lambda: ops.rms_norm_validate(x, w, None, 1e-60),
        "eps = nan": lambda: ops.rms_norm_validate(x, w, None, float("nan")),
        "eps = inf": lambda: ops.rms_norm_validate(x, w, None, float("inf")),
        "eps a tensor": lambda: ops.rms_norm_validate(x, w, None, torch.tensor(1e-5)),
    }
    for what, call in refused.items():
        with pytest.raises(ValueError, match="rms_norm"):
            call()
            pytest.fail(f"{what} was accepted")


@pytest.mark.parametrize("wdtype", [BF, torch.float32], ids=["bf16", "fp32"])
def test_references_agree_with_fp64_rms_norm_and_autograd_through_it(wdtype):
    eps = 1e-5
    for T, d in ((1, 8), (3, 136), (9, 64)):
        x, r, w = _rows(T, d, T), _rows(T, d, T + 1), _weight(d, wdtype)
        for residual in (None, r):
            h, y, rstd = ops.rms_norm_reference(x, w, eps, residual)
            assert h.dtype == BF and y.dtype == torch.float64 and rstd.dtype == torch.float64
            assert torch.equal(h, x if residual is None else x + r)
            hd = h.double().requires_grad_()
            wd = w.double().requires_grad_()
            want = F.rms_norm(hd, (d,), wd, eps)
            assert ((y - want).abs() <= 1e-12 * want.abs()).all()
            want_rstd = 1.0 / torch.sqrt(h.double().pow(2).mean(dim=1) + eps)
            assert ((rstd - want_rstd).abs() <= 1e-12 * want_rstd).all()
            dy, dres = _rows(T, d, 50 + T), _rows(T, d, 60 + T)
            gh, gw = torch.autograd.grad(want, (hd, wd), dy.double())
            for dr in (None, dres):
                dh, dw = ops.rms_norm_backward_reference(dy, h, w, eps, dr)
                want_dh = gh if dr is None else gh + dr.double()
                scale = want_dh.abs().max()
                assert ((dh - want_dh).abs() <= 1e-12 * scale).all()
                assert ((dw - gw).abs() <= 1e-12 * gw.abs().max()).all()


def _header_constants():
    text = HEADER.read_text()
    found = dict(re.findall(r"constexpr int (kRms\w+) = (\d+);", text))
    return {k: int(v) for k, v in found.items()}, text


def test_row_chunk_is_the_rule_of_the_header():
    k, text = _header_constants()
    lo, hi, groups = k["kRmsMinChunk"], k["kRmsMaxChunk"], k["kRmsTargetGroups"]
    assert (lo, hi, groups) == (ops.kernels._RMS_MIN_CHUNK, ops.kernels._RMS_MAX_CHUNK, ops.kernels._RMS_TARGET_GROUPS)
    assert k["kRmsMaxD"] == ops.RMS_NORM_MAX_D == 16384 and k["kRmsThreads"] == 256
    # the header's rule, as it is written there
    assert "int64_t c = (T + kRmsTargetGroups - 1) / kRmsTargetGroups;" in text
    assert "if (c < kRmsMinChunk) c = kRmsMinChunk;" in text and "if (c > kRmsMaxChunk) c = kRmsMaxChunk;" in text
    rule = lambda T: max(lo, min(hi, (T + groups - 1) // groups))
    for d in (8, 136, 4096, 16384):
        for T in (1, 3, lo - 1, lo + 1, 257, lo * groups, lo * groups + 1, 9000, hi * groups, hi * groups + 1, 1 << 30):
            c = ops.rms_norm_row_chunk(T, d)
            assert c > 0 and c == rule(T) == ops.rms_norm_row_chunk(T, d)
    assert ops.rms_norm_row_chunk(4096, 4096) == 8 and ops.rms_norm_row_chunk(32768, 4096) == 32
    assert ops.rms_norm_row_chunk(lo * groups + 1, 64) == lo + 1
    for T, d in ((0, 8), (8, 0), (-1, 8)):
        with pytest.raises(ValueError, match="rms_norm_row_chunk"):
            ops.rms_norm_row_chunk(T, d)


class StubComm:
    def Get_size(self):
        return 1

    def Get_rank(self):
        return 0


def test_llama_config_norm():
    tiny = dict(d=256, heads=4, kv_heads=2, ffn=256, vocab=512, layers=1)
    assert NORM_KINDS == ("torch", "fused") and LlamaConfig().norm == "torch"
    with pytest.raises(ValueError, match="norm"):
        LlamaBlock(LlamaConfig(**tiny, norm="layer"), None, 0, "cpu")
    with pytest.raises(ValueError, match="norm"):
        LlamaBlock(LlamaConfig(d=36, heads=1, kv_heads=1, ffn=64, vocab=64, layers=1, norm="fused"), None, 0, "cpu")
    blk = LlamaBlock(LlamaConfig(**tiny, norm="fused"), StubComm(), 0, "cpu")
    assert sorted(n for n, _ in blk.named_parameters() if "norm" in n) == ["attn_norm.weight", "mlp_norm.weight"]
    with pytest.raises(ValueError, match="addend"):  # the pair form belongs to norm="fused"
        LlamaBlock(LlamaConfig(**tiny), StubComm(), 0, "cpu")(torch.zeros(8, 256, dtype=BF), 1, 8, None, torch.zeros(8, 256, dtype=BF))
