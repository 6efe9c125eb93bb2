"""Per-expert capacity of the routed MoE dispatch and the fused router, the parts that need
no GPU: the host mirrors ``moe_layout(..., expert_capacity=)`` and ``moe_kept`` against a
brute-force walk over the entries in (expert, source rank, token, slot) order, the new
argument rules of ``moe_validate`` (through the function and through
``DeviceGroup.moe_dispatch`` on a stand-in group, which must raise before it needs a GPU),
``moe_gate_validate``, and the handle's new attributes."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from collective_communication_mpi_amd import ops
from collective_communication_mpi_amd.device import DeviceGroup, MoEHandle, moe_kept, moe_layout, moe_validate
from collective_communication_mpi_amd.parallel import RoutedMoE


def walk(c, Ce):
    """Entry by entry: (kept [p, E], first kept row of every (source, expert) segment or -1,
    rows per expert, rows per rank)."""
    p, E = c.shape
    El = E // p
    kept = np.zeros((p, E), np.int64)
    first_row = np.full((p, E), -1, np.int64)
    col = np.zeros(E, np.int64)
    totals = np.zeros(p, np.int64)
    for e in range(E):                       # experts in order: rows of a rank are by local expert
        owner = e // El
        q = 0
        for i in range(p):                   # then source rank; (token, slot) order inside is the entry order
            for _ in range(int(c[i, e])):
                if q < Ce:
                    if first_row[i, e] < 0:
                        first_row[i, e] = totals[owner]
                    kept[i, e] += 1
                    col[e] += 1
                    totals[owner] += 1
                q += 1
    return kept, first_row, col, totals


def matrices(p):
    rng = np.random.default_rng(4100 + p)
    for El in (1, 2, 3):
        E = p * El
        for _ in range(6):
            c = rng.integers(0, 40, size=(p, E))
            c[:, rng.integers(0, E)] = 0                 # an empty expert
            yield c, int(rng.integers(1, 60))
        s = np.zeros((p, E), np.int64)                   # one expert takes everything
        s[:, 0] = rng.integers(5, 30, size=p)
        yield s, 4
    yield np.zeros((p, p), np.int64), 3


@pytest.mark.parametrize("p", [1, 2, 3, 8])
def test_capacity_layout_matches_the_walk(p):
    saw_nothing_kept = False
    for c, Ce in matrices(p):
        E = c.shape[1]
        El = E // p
        kept, first_row, col, totals = walk(c, Ce)
        assert np.array_equal(moe_kept(c, Ce), kept)
        before = np.cumsum(c, axis=0) - c
        saw_nothing_kept |= bool(((before >= Ce) & (c > 0)).any())
        for me in range(p):
            base, expert_counts, tot = moe_layout(c, me, expert_capacity=Ce)
            assert np.array_equal(expert_counts, col[me * El:(me + 1) * El])
            assert np.array_equal(tot, totals)
            has = kept > 0
            assert np.array_equal(base[has], first_row[has])
            # a segment with nothing kept lies where the expert's rows end or, for an expert
            # within capacity, where it would have started
            first = base[0]                                  # source 0 has before = 0
            assert np.array_equal(base, first[None, :] + np.minimum(before, Ce))
    assert saw_nothing_kept or p == 1


def test_a_rank_behind_a_full_expert_keeps_nothing():
    c = np.array([[5, 0, 1], [3, 2, 0], [4, 1, 0]])   # 3 ranks, one expert each; expert 0 is full after rank 0
    kept = moe_kept(c, 5)
    assert kept.tolist() == [[5, 0, 1], [0, 2, 0], [0, 1, 0]]
    base, ec, totals = moe_layout(c, 0, expert_capacity=5)
    assert ec.tolist() == [5] and totals.tolist() == [5, 3, 1]
    assert base[:, 0].tolist() == [0, 5, 5]


@pytest.mark.parametrize("p", [1, 2, 3, 8])
def test_a_capacity_above_every_column_changes_nothing(p):
    for c, _ in matrices(p):
        Ce = int(c.sum(axis=0).max()) + 1
        assert np.array_equal(moe_kept(c, Ce), c)
        for me in range(p):
            for a, b in zip(moe_layout(c, me), moe_layout(c, me, expert_capacity=Ce)):
                assert np.array_equal(a, b)


def test_layout_rejects_a_bad_capacity():
    c = np.ones((2, 2), np.int64)
    for bad in (0, -3):
        with pytest.raises(ValueError, match="expert_capacity"):
            moe_layout(c, 0, expert_capacity=bad)
        with pytest.raises(ValueError, match="expert_capacity"):
            moe_kept(c, bad)


def args(T=6, D=8, K=2, cap=16):
    return torch.zeros(T, D), torch.zeros(T, K, dtype=torch.int64), torch.zeros(cap, D)


@pytest.mark.parametrize("via_group", [False, True])
def test_capacity_validation_raises_before_any_launch(via_group):
    def call(p, x, idx, E, recv, Ce):
        if via_group:
            return DeviceGroup.moe_dispatch(SimpleNamespace(size=p, torch=torch), x, idx, E, recv, expert_capacity=Ce)
        return moe_validate(p, x, idx, E, recv, Ce)

    x, idx, recv = args(cap=12)                     # E = 8 on 2 ranks: 4 local experts
    with pytest.raises(ValueError, match="expert_capacity"):
        call(2, x, idx, 8, recv, 0)
    with pytest.raises(ValueError, match="expert_capacity"):
        call(2, x, idx, 8, recv, -1)
    x, idx, recv = args(cap=4 * 3 - 1)              # one row short of (E / p) * Ce
    with pytest.raises(ValueError, match="rows"):
        call(2, x, idx, 8, recv, 3)
    x, idx, recv = args(cap=4 * 3)
    assert moe_validate(2, x, idx, 8, recv, 3) == (6, 2, 8)
    assert moe_validate(2, x, idx, 8, recv) == (6, 2, 8)
    assert moe_validate(2, x, idx, 8, recv, None) == (6, 2, 8)


def test_gate_validation():
    v = ops.moe_gate_validate
    assert v(torch.zeros(3, 256), 8) == (3, 256, 8)
    assert v(torch.zeros(0, 8), 2) == (0, 8, 2)
    assert v(torch.zeros(1, 1), 1) == (1, 1, 1)
    assert v(torch.zeros(2, 5), 5) == (2, 5, 5)
    with pytest.raises(ValueError, match="experts"):
        v(torch.zeros(3, 257), 2)
    with pytest.raises(ValueError, match="experts"):
        v(torch.zeros(3, 0), 1)
    with pytest.raises(ValueError, match="top_k"):
        v(torch.zeros(3, 64), 9)
    with pytest.raises(ValueError, match="top_k"):
        v(torch.zeros(3, 4), 5)                              # K > E
    with pytest.raises(ValueError, match="top_k"):
        v(torch.zeros(3, 4), 0)
    with pytest.raises(TypeError, match="fp32"):
        v(torch.zeros(3, 8, dtype=torch.float16), 2)
    with pytest.raises(ValueError, match="contiguous"):
        v(torch.zeros(8, 3).t(), 2)
    with pytest.raises(ValueError, match=r"\[T, E\]"):
        v(torch.zeros(8), 2)
    for name in ("moe_gate", "moe_gate_forward", "moe_gate_backward"):
        assert callable(getattr(ops, name))


def test_handle_keeps_its_nine_argument_form():
    h = MoEHandle(None, None, None, 8, 1, 2, 3, torch.float32, 4)
    assert h.num_dropped is None and h.expert_capacity is None
    assert (h.num_experts, h.T, h.K, h.D, h.cap) == (8, 1, 2, 3, 4)
    h = MoEHandle(None, None, None, 8, 1, 2, 3, torch.float32, 4, "n", 5)
    assert (h.num_dropped, h.expert_capacity) == ("n", 5)


def test_capacity_for():
    assert RoutedMoE.capacity_for(1000, 2, 8, 1.0) == 250
    assert RoutedMoE.capacity_for(1000, 2, 8, 1.25) == 313
    assert RoutedMoE.capacity_for(7, 1, 4, 1.0) == 2
