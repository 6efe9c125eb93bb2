"""The whole routed MoE layer on 2 and 3 ranks sharing the GPU
(tests/workers/moe_experts_worker.py): moe_dispatch -> GroupedExpertsMLP (grouped gate|up
GEMM, SwiGLU, grouped down GEMM, the rows per expert read on the device) -> weighted
moe_combine, checked per token against a dense fp64 evaluation under skewed routing (one
local expert over a tile, one empty); on 2 ranks also captured in one graph and replayed
with new tokens and routing."""
import pytest

from _launch import py, run_ranks

pytestmark = pytest.mark.gpu

ENV = {"CCMPI_DEVICE_TIMEOUT_S": "20"}


@pytest.mark.parametrize("n", [2, 3])
def test_moe_experts(n):
    r = run_ranks(n, py("tests/workers/moe_experts_worker.py"), timeout=240, env=ENV)
    assert "moe experts OK" in r.stdout
    assert "worst error / tolerance" in r.stdout
