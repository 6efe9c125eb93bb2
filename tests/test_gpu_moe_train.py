"""One training step through the routed MoE layer on 2 and 3 ranks sharing the GPU
(tests/workers/moe_train_worker.py): autograd moe_dispatch -> GroupedExpertsMLP ->
autograd moe_combine with x and the combine weights as leaves, every gradient (x, weights,
this rank's expert weights) against a dense fp64 evaluation of all ranks' tokens under
skewed routing; then one RoutedMoE forward + backward, x.grad and the router gradient
against fp64 with the routing the forward chose."""
import pytest

from _launch import py, run_ranks

pytestmark = pytest.mark.gpu

ENV = {"CCMPI_DEVICE_TIMEOUT_S": "20"}


@pytest.mark.parametrize("n", [2, 3])
def test_moe_train(n):
    r = run_ranks(n, py("tests/workers/moe_train_worker.py"), timeout=240, env=ENV)
    assert "moe train OK" in r.stdout
    assert "worst error / tolerance" in r.stdout
