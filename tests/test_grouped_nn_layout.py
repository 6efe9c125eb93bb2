"""Host-side rules of the grouped dX kernel (no GPU): the argument checks of
``grouped_gemm_nn`` and the environment switches that choose the backward's routes."""
import pytest
import torch

from collective_communication_mpi_amd.ops import (
    grouped_dx_route,
    grouped_gemm_nn,
    grouped_nn_validate,
    grouped_swiglu_route,
)

G, CAP, N, K = 3, 40, 24, 16


def _args(**kw):
    a = dict(dy=torch.zeros(CAP, N, dtype=torch.bfloat16), w=torch.zeros(G, N, K, dtype=torch.bfloat16),
             counts=torch.zeros(G, dtype=torch.int32), out=None, out_dtype=torch.bfloat16)
    a.update(kw)
    return a


def test_accepts_what_the_forward_accepts():
    assert grouped_nn_validate(**_args()) == (CAP, G, N, K)
    assert grouped_nn_validate(**_args(counts=torch.zeros(G, dtype=torch.int64), out_dtype=torch.float32)) == (CAP, G, N, K)
    # free row strides on both operands and a strided output
    dy = torch.zeros(CAP, N + 8, dtype=torch.bfloat16)[:, :N]
    w = torch.zeros(G, N + 8, K + 8, dtype=torch.bfloat16)[:, :N, :K]
    out = torch.zeros(CAP, K + 8, dtype=torch.float32)[:, :K]
    assert grouped_nn_validate(**_args(dy=dy, w=w, out=out)) == (CAP, G, N, K)


BAD = {
    "dy dtype": (TypeError, dict(dy=torch.zeros(CAP, N, dtype=torch.float16))),
    "w dtype": (TypeError, dict(w=torch.zeros(G, N, K))),
    "reduction mismatch": (ValueError, dict(dy=torch.zeros(CAP, N + 8, dtype=torch.bfloat16))),
    "dy rank": (ValueError, dict(dy=torch.zeros(CAP, N, 1, dtype=torch.bfloat16))),
    "N % 8": (ValueError, dict(dy=torch.zeros(CAP, 20, dtype=torch.bfloat16), w=torch.zeros(G, 20, K, dtype=torch.bfloat16))),
    "K % 8": (ValueError, dict(w=torch.zeros(G, N, 12, dtype=torch.bfloat16))),
    "dy inner stride": (ValueError, dict(dy=torch.zeros(CAP, 2 * N, dtype=torch.bfloat16)[:, ::2])),
    "w inner stride": (ValueError, dict(w=torch.zeros(G, N, 2 * K, dtype=torch.bfloat16)[:, :, ::2])),
    "dy row stride": (ValueError, dict(dy=torch.zeros(CAP, N + 4, dtype=torch.bfloat16)[:, :N])),
    "w row stride": (ValueError, dict(w=torch.zeros(G, N, K + 4, dtype=torch.bfloat16)[:, :, :K])),
    "w expert stride": (ValueError, dict(w=torch.zeros(G * N * K + 2 * 4, dtype=torch.bfloat16).as_strided((G, N, K), (N * K + 4, K, 1)))),
    "counts length": (ValueError, dict(counts=torch.zeros(G + 1, dtype=torch.int32))),
    "counts dtype": (TypeError, dict(counts=torch.zeros(G, dtype=torch.float32))),
    "out shape": (ValueError, dict(out=torch.zeros(CAP, N, dtype=torch.bfloat16))),
    "out dtype": (TypeError, dict(out=torch.zeros(CAP, K, dtype=torch.float16))),
    "out_dtype": (TypeError, dict(out_dtype=torch.float16)),
    "out row stride": (ValueError, dict(out=torch.zeros(CAP, K + 4, dtype=torch.bfloat16)[:, :K])),
}


@pytest.mark.parametrize("what", list(BAD))
def test_argument_rules_name_the_op(what):
    exc, kw = BAD[what]
    with pytest.raises(exc, match="grouped_gemm_nn"):
        grouped_nn_validate(**_args(**kw))
    # the op applies the same rules before it touches the device
    a = _args(**kw)
    with pytest.raises(exc, match="grouped_gemm_nn"):
        grouped_gemm_nn(a["dy"], a["w"], a["counts"], out=a["out"], out_dtype=a["out_dtype"])


def test_dx_route_is_read_at_call_time(monkeypatch):
    monkeypatch.delenv("CCMPI_GROUPED_DX", raising=False)
    assert grouped_dx_route() == "nn"
    monkeypatch.setenv("CCMPI_GROUPED_DX", "transpose")
    assert grouped_dx_route() == "transpose"
    monkeypatch.setenv("CCMPI_GROUPED_DX", "nn")
    assert grouped_dx_route() == "nn"
    monkeypatch.setenv("CCMPI_GROUPED_DX", "fast")
    with pytest.raises(ValueError, match="CCMPI_GROUPED_DX"):
        grouped_dx_route()


def test_swiglu_route_is_read_at_call_time(monkeypatch):
    monkeypatch.delenv("CCMPI_GROUPED_SWIGLU", raising=False)
    assert grouped_swiglu_route() == "fused"
    monkeypatch.setenv("CCMPI_GROUPED_SWIGLU", "unfused")
    assert grouped_swiglu_route() == "unfused"
    monkeypatch.setenv("CCMPI_GROUPED_SWIGLU", "both")
    with pytest.raises(ValueError, match="CCMPI_GROUPED_SWIGLU"):
        grouped_swiglu_route()
