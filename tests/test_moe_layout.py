"""Routed MoE dispatch, the parts that need no GPU: the row layout derived from a
p x E count matrix (``moe_layout``: the segments of every rank tile its buffer in
(local expert, source) order), the public methods, and the argument rules that
raise ValueError before any launch."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from collective_communication_mpi_amd import Communicator
from collective_communication_mpi_amd.device import DeviceGroup, MoEHandle, moe_layout, moe_validate


def matrices(p):
    rng = np.random.default_rng(100 + p)
    for El in (1, 3, 4):
        E = p * El
        c = rng.integers(0, 50, size=(p, E))
        yield c
        z = c.copy()
        z[rng.integers(0, p)] = 0          # a rank that sends nothing
        z[:, rng.integers(0, E)] = 0       # an expert chosen by nobody
        yield z
        s = np.zeros((p, E), np.int64)     # extreme skew: one expert takes everything
        s[:, E - 1] = rng.integers(1, 2000, size=p)
        yield s
    yield np.zeros((p, p), np.int64)       # nothing routed at all


@pytest.mark.parametrize("p", [1, 2, 3, 8])
def test_layout_tiles_every_rank(p):
    for c in matrices(p):
        E = c.shape[1]
        El = E // p
        for me in range(p):
            base, expert_counts, totals = moe_layout(c, me)
            assert base.shape == (p, E) and totals.shape == (p,)
            assert np.array_equal(expert_counts, c.sum(axis=0)[me * El:(me + 1) * El])
            assert expert_counts.sum() == totals[me]
        for j in range(p):
            # walk rank j's segments in (local expert, source) order: each starts where the
            # previous one ended, the first at 0, the last ends at total_j (no gap, no overlap)
            at = 0
            for e in range(j * El, (j + 1) * El):
                for i in range(p):
                    assert base[i, e] == at, (p, j, e, i)
                    at += c[i, e]
            assert at == totals[j] == c[:, j * El:(j + 1) * El].sum()


def test_layout_rejects_bad_matrices():
    with pytest.raises(ValueError):
        moe_layout(np.zeros((2, 3), np.int64), 0)      # E % p
    with pytest.raises(ValueError):
        moe_layout(np.full((2, 2), -1), 0)
    with pytest.raises(ValueError):
        moe_layout(np.zeros((2, 2), np.int64), 2)


def test_public_methods_exist():
    for cls in (Communicator, DeviceGroup):
        assert callable(getattr(cls, "moe_dispatch")) and callable(getattr(cls, "moe_combine"))
    assert "total_bytes_transferred" in Communicator.moe_dispatch.__doc__
    h = MoEHandle(None, None, None, 8, 1, 2, 3, torch.float32, 4)
    assert (h.num_experts, h.T, h.K, h.D) == (8, 1, 2, 3)


def args(T=6, D=8, K=2, dtype=torch.float32, idx_dtype=torch.int64, cap=16):
    return torch.zeros(T, D, dtype=dtype), torch.zeros(T, K, dtype=idx_dtype), torch.zeros(cap, D, dtype=dtype)


def test_validation_accepts_the_contract():
    x, idx, recv = args()
    assert moe_validate(2, x, idx, 4, recv) == (6, 2, 8)
    x, idx, recv = args(T=0, D=24, K=8, dtype=torch.bfloat16, idx_dtype=torch.int32)
    assert moe_validate(8, x, idx, 256, recv) == (0, 8, 24)


@pytest.mark.parametrize("via_group", [False, True])
def test_validation_raises_before_any_launch(via_group):
    def call(p, x, idx, E, recv):
        if via_group:  # the method itself, on a stand-in group: it must raise before it needs a GPU
            return DeviceGroup.moe_dispatch(SimpleNamespace(size=p, torch=torch), x, idx, E, recv)
        return moe_validate(p, x, idx, E, recv)

    x, idx, recv = args()
    with pytest.raises(ValueError, match="multiple of the group size"):
        call(3, x, idx, 4, recv)                                 # E % p != 0
    with pytest.raises(ValueError, match="num_experts"):
        call(2, x, idx, 258, recv)                               # E > 256
    with pytest.raises(ValueError, match="num_experts"):
        call(2, x, idx, 0, recv)
    xk, idxk, recvk = args(K=9)
    with pytest.raises(ValueError, match="K must be"):
        call(2, xk, idxk, 4, recvk)                              # K > 8
    with pytest.raises(ValueError, match="rows"):
        call(2, x, torch.zeros(5, 2, dtype=torch.int64), 4, recv)   # topk_idx rows != T
    with pytest.raises(ValueError, match="recv_x"):
        call(2, x, idx, 4, torch.zeros(16, 12))                  # row length differs
    with pytest.raises(ValueError, match="recv_x"):
        call(2, x, idx, 4, torch.zeros(16, 8, dtype=torch.bfloat16))  # dtype differs
    with pytest.raises(ValueError, match="2-D"):
        call(2, x.reshape(-1), idx, 4, recv)
    with pytest.raises(ValueError, match="topk_idx must be"):
        call(2, x, idx.to(torch.float32), 4, recv)
    with pytest.raises(ValueError, match="bf16, fp16 or fp32"):
        call(2, x.double(), idx, 4, recv.double())
    x6, idx6, recv6 = args(D=6)
    with pytest.raises(ValueError, match="16 bytes"):
        call(2, x6, idx6, 4, recv6)                              # 24-B rows
