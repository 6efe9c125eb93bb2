"""The trainable routed MoE path, the parts that need no GPU: the public names
(``moe_combine_backward`` on DeviceGroup and Communicator, the autograd functions and
``RoutedMoE`` in ``parallel``) and the argument rules of the combine's backward, which
raise ValueError before any launch."""
from types import SimpleNamespace

import pytest
import torch

from collective_communication_mpi_amd import Communicator, parallel
from collective_communication_mpi_amd.device import DeviceGroup, MoEHandle, moe_backward_validate


def handle(T=6, K=2, D=8, dtype=torch.float32, cap=16, E=4):
    return MoEHandle(torch.zeros(T, K, dtype=torch.int32), torch.zeros(T, K, dtype=torch.int32),
                     torch.zeros(2, dtype=torch.int64), E, T, K, D, dtype, cap)


def test_public_names_exist():
    for cls in (Communicator, DeviceGroup):
        assert callable(getattr(cls, "moe_combine_backward"))
    for name in ("moe_dispatch", "moe_combine", "RoutedMoE", "GroupedExpertsMLP"):
        assert callable(getattr(parallel, name))
    assert issubclass(parallel.RoutedMoE, torch.nn.Module)


def test_validation_accepts_the_contract():
    h = handle()
    dout = torch.zeros(6, 8)
    moe_backward_validate(h, dout)                                            # weights, y, dy all None
    moe_backward_validate(h, dout, torch.zeros(6, 2), torch.zeros(16, 8), torch.zeros(20, 8))
    moe_backward_validate(h, dout, None, None, torch.zeros(16, 8))
    h0 = handle(T=0, K=8, D=24, dtype=torch.bfloat16, cap=1)
    z = torch.zeros(0, 24, dtype=torch.bfloat16)
    moe_backward_validate(h0, z, torch.zeros(0, 8), torch.zeros(1, 24, dtype=torch.bfloat16),
                          torch.zeros(3, 24, dtype=torch.bfloat16))
    moe_backward_validate(h0, z, None)


@pytest.mark.parametrize("via_group", [False, True])
def test_validation_raises_before_any_launch(via_group):
    h = handle()

    def call(dout, weights=None, y=None, dy=None):
        if via_group:  # the method itself, on a stand-in group: it must raise before it needs a GPU
            return DeviceGroup.moe_combine_backward(SimpleNamespace(size=2, torch=torch), dout, h, weights, y, dy)
        return moe_backward_validate(h, dout, weights, y, dy)

    ok = torch.zeros(6, 8)
    with pytest.raises(ValueError, match="dout must be"):
        call(torch.zeros(5, 8))                                  # rows != T
    with pytest.raises(ValueError, match="dout must be"):
        call(torch.zeros(6, 12))                                 # row length != D
    with pytest.raises(ValueError, match="dout must be"):
        call(torch.zeros(48))                                    # not 2-D
    with pytest.raises(ValueError, match="dtype"):
        call(ok.bfloat16())
    with pytest.raises(ValueError, match="weights"):
        call(ok, torch.zeros(6, 3))                              # not [T, K]
    with pytest.raises(ValueError, match="weights"):
        call(ok, torch.zeros(6, 2, dtype=torch.float64))         # not fp32
    with pytest.raises(ValueError, match="weights"):
        call(ok, torch.zeros(12))
    for name in ("y", "dy"):
        with pytest.raises(ValueError, match=f"{name} has 15 rows"):
            call(ok, **{name: torch.zeros(15, 8)})               # fewer rows than the dispatch buffer
        with pytest.raises(ValueError, match=f"{name} must be"):
            call(ok, **{name: torch.zeros(16, 8, dtype=torch.bfloat16)})
        with pytest.raises(ValueError, match=f"{name} must be"):
            call(ok, **{name: torch.zeros(16, 12)})
        with pytest.raises(ValueError, match=f"{name} must be"):
            call(ok, **{name: torch.zeros(128)})
    buf = torch.zeros(40, 8)
    with pytest.raises(ValueError, match="overlap"):
        call(ok, y=buf[:16], dy=buf[:16])                        # the same tensor
    with pytest.raises(ValueError, match="overlap"):
        call(ok, y=buf[:20], dy=buf[10:30])                      # overlapping views
    moe_backward_validate(h, ok, None, buf[:16], buf[16:32])     # adjacent is fine
