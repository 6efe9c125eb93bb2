"""One training step of RoutedMoE(gate="fused", expert_capacity=Ce, aux_loss_coef > 0) on 2
and 3 ranks sharing the GPU (tests/workers/moe_capacity_train_worker.py): every rank drops
entries over the capacity; x.grad, the router gradient and this rank's expert weight
gradients against a dense fp64 autograd model in which a dropped slot's term is masked to
zero (the mask from ``moe_kept`` on the host) and the load-balancing loss is added; the fused
gate's idx against ``torch.topk``."""
import pytest

from _launch import py, run_ranks

pytestmark = pytest.mark.gpu

ENV = {"CCMPI_DEVICE_TIMEOUT_S": "20"}


@pytest.mark.parametrize("n", [2, 3])
def test_moe_capacity_train(n):
    r = run_ranks(n, py("tests/workers/moe_capacity_train_worker.py"), timeout=240, env=ENV)
    assert "moe capacity train OK" in r.stdout
    assert "worst error / tolerance" in r.stdout
