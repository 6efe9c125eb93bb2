"""One training step of RoutedMoE(gate="fused", router_logits="mfma", expert_capacity=Ce,
aux_loss_coef > 0) on 2 and 3 ranks sharing the GPU (tests/workers/moe_router_train_worker.py):
x.grad, the router gradient and this rank's expert weight gradients against the dense fp64
autograd model of moe_capacity_train_worker.py, routed with the idx the layer chose; the
layer's selection against the fp64 top-k wherever the K-th gap is larger than rounding."""
import pytest

from _launch import py, run_ranks

pytestmark = pytest.mark.gpu

ENV = {"CCMPI_DEVICE_TIMEOUT_S": "20"}


@pytest.mark.parametrize("n", [2, 3])
def test_moe_router_train(n):
    r = run_ranks(n, py("tests/workers/moe_router_train_worker.py"), timeout=240, env=ENV)
    assert "moe router train OK" in r.stdout
    assert "worst error / tolerance" in r.stdout
