"""Backward of the routed MoE collectives on 2, 3 and 8 ranks sharing the GPU
(tests/workers/moe_backward_worker.py): the combine's backward kernel -- dy bitwise
per routed row, refused and spare rows untouched, dweights against an fp64 dot within a
derived bound, exactly 0 for slots that are not live and bitwise reproducible -- and the
dispatch's autograd backward against the unweighted combine; on 2 ranks also captured in
a graph and replayed with new gradients, weights and routing."""
import pytest

from _launch import py, run_ranks

pytestmark = pytest.mark.gpu

ENV = {"CCMPI_DEVICE_TIMEOUT_S": "20"}


@pytest.mark.parametrize("n", [2, 3, 8])
def test_moe_backward(n):
    r = run_ranks(n, py("tests/workers/moe_backward_worker.py"), timeout=240, env=ENV)
    assert "moe backward OK" in r.stdout
    assert "worst error / bound" in r.stdout
