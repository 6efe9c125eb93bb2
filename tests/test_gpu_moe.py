"""Routed MoE token dispatch and weighted combine on 2, 3 and 8 ranks sharing the GPU
(tests/workers/moe_worker.py): dispatch as a pure copy into (local expert, source,
token, slot) order with exact expert_counts / row_of, bitwise against the existing
alltoallv at one expert per rank, round trips, combine bitwise (weights=None) and
against fp64 (weighted), 20 skewed back-to-back pairs, HIP graph replays (2 ranks),
and a receive buffer one row short (fault code 0xA00, nothing written past it)."""
import pytest

from _launch import py, run_ranks

pytestmark = pytest.mark.gpu

ENV = {"CCMPI_DEVICE_TIMEOUT_S": "20"}


@pytest.mark.parametrize("n", [2, 3, 8])
def test_moe_dispatch_combine(n):
    r = run_ranks(n, py("tests/workers/moe_worker.py"), timeout=240, env=ENV)
    assert "moe OK" in r.stdout
