"""Argument rules of the MFMA router logits (``ops.moe_router_logits_validate``) and of
``RoutedMoE(router_logits=...)``; no GPU needed."""
import pytest
import torch

from collective_communication_mpi_amd import ops
from collective_communication_mpi_amd.parallel import RoutedMoE

SHAPES = [(0, 64, 8), (1, 8, 1), (5, 72, 8), (130, 200, 24), (257, 448, 96), (131, 1024, 200), (129, 7168, 256)]


def _pair(T, D, E):
    return torch.zeros(T, D, dtype=torch.bfloat16), torch.zeros(E, D, dtype=torch.float32)


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_accepts_the_supported_shapes(shape):
    assert ops.moe_router_logits_validate(*_pair(*shape)) == shape


def test_accepts_a_row_strided_x():
    wide = torch.zeros(9, 96, dtype=torch.bfloat16)
    assert ops.moe_router_logits_validate(wide[:, 8:72], torch.zeros(4, 64)) == (9, 64, 4)


def test_rejects_dtypes():
    x, r = _pair(4, 64, 8)
    with pytest.raises(TypeError):
        ops.moe_router_logits_validate(x.float(), r)
    with pytest.raises(TypeError):
        ops.moe_router_logits_validate(x, r.bfloat16())


@pytest.mark.parametrize("what", ["D % 8", "E == 0", "E == 257", "D mismatch", "router not contiguous",
                                  "x column stride", "x row stride", "x misaligned", "x 3-D"])
def test_rejects_shapes_and_strides(what):
    x, r = _pair(4, 64, 8)
    if what == "D % 8":
        x, r = _pair(4, 60, 8)
    elif what == "E == 0":
        r = torch.zeros(0, 64)
    elif what == "E == 257":
        r = torch.zeros(257, 64)
    elif what == "D mismatch":
        r = torch.zeros(8, 72)
    elif what == "router not contiguous":
        r = torch.zeros(64, 8).t()
    elif what == "x column stride":
        x = torch.zeros(64, 4, dtype=torch.bfloat16).t()
    elif what == "x row stride":
        x = torch.zeros(4, 68, dtype=torch.bfloat16)[:, :64]
    elif what == "x misaligned":
        x = torch.zeros(4, 72, dtype=torch.bfloat16)[:, 4:68]
    elif what == "x 3-D":
        x = torch.zeros(2, 2, 64, dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        ops.moe_router_logits_validate(x, r)


def test_split_rejects_what_it_cannot_take():
    with pytest.raises(TypeError):
        ops.split_bf16x3(torch.zeros(4, 8, dtype=torch.bfloat16))
    with pytest.raises(ValueError):
        ops.split_bf16x3(torch.zeros(4, 8), planes=4)
    with pytest.raises(ValueError):
        ops.split_bf16x3(torch.zeros(8, 4).t())
    with pytest.raises(ValueError):
        ops.split_bf16x3(torch.zeros(4, 8), concat=(0, 3))


def test_the_kernels_refuse_host_tensors():
    x, r = _pair(4, 64, 8)
    with pytest.raises(ValueError, match="GPU"):
        ops.split_bf16x3(r)
    with pytest.raises(ValueError, match="GPU"):
        ops.moe_router_logits_forward(x, r)
    with pytest.raises(ValueError, match="GPU"):
        ops.moe_router_logits_backward(torch.zeros(4, 8), x, torch.zeros(3, 8, 64, dtype=torch.bfloat16))


class _Group:
    """As much of a DeviceGroup as RoutedMoE's argument checks look at."""
    size = 1
    device = "cpu"


def test_routed_moe_rejects_an_unknown_router_logits():
    with pytest.raises(ValueError, match="router_logits"):
        RoutedMoE(_Group(), 64, 32, 4, 2, 16, router_logits="bogus")
