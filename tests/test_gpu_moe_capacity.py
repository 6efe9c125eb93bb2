"""Routed MoE dispatch with a per-expert capacity on 2, 3 and 8 ranks sharing the GPU
(tests/workers/moe_capacity_worker.py): entries over ``expert_capacity`` are dropped in
(source rank, token, slot) priority without a fault code, the kept rows are bitwise copies in
the compacted (local expert, source rank, token, slot) order, expert_counts / row_of /
num_dropped are exact, a capacity nobody reaches is bit for bit the call without one, and
the combine, its backward and the grouped GEMM run over the result; on 2 ranks a captured
dispatch + combine replayed with routing that changes which entries drop."""
import pytest

from _launch import py, run_ranks

pytestmark = pytest.mark.gpu

ENV = {"CCMPI_DEVICE_TIMEOUT_S": "20"}


@pytest.mark.parametrize("n", [2, 3, 8])
def test_moe_expert_capacity(n):
    r = run_ranks(n, py("tests/workers/moe_capacity_worker.py"), timeout=240, env=ENV)
    assert "moe capacity OK" in r.stdout
