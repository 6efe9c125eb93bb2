"""Argument rules of the packed form of flash attention (``ops.flash_attention_varlen_validate``)
and the host mirror of its slot map (``ops.flash_varlen_tile_map``), on CPU tensors: no GPU is
needed to accept or refuse an operand, and the map is the kernels' arithmetic in Python."""
import random

import pytest
import torch

from collective_communication_mpi_amd import ops
from collective_communication_mpi_amd.ops.kernels import FLASH_BK, FLASH_BQ

T, HQ, HKV, D = 40, 4, 2, 64
BF = torch.bfloat16


def _q(t=T, hq=HQ, d=D, dtype=BF):
    return torch.zeros(t, hq, d, dtype=dtype)


def _kv(t=T, hkv=HKV, d=D, dtype=BF):
    return torch.zeros(t, hkv, d, dtype=dtype)


def _cu(*bounds, dtype=torch.int32):
    return torch.tensor(bounds or (0, 13, 13, T), dtype=dtype)


def test_accepts():
    assert ops.flash_attention_varlen_validate(_q(), _kv(), _kv(), _cu()) == (T, 3, HQ, HKV, D)
    assert ops.flash_attention_varlen_validate(_q(hq=8, d=128), _kv(hkv=1, d=128), _kv(hkv=1, d=128), _cu(0, T)) == (
        T, 1, 8, 1, 128)
    assert ops.flash_attention_varlen_validate(_q(t=1), _kv(t=1), _kv(t=1), _cu(0, 0, 1, 1)) == (1, 3, HQ, HKV, D)
    # the contents of cu_seqlens are the caller's promise and are read on the device only
    assert ops.flash_attention_varlen_validate(_q(), _kv(), _kv(), _cu(5, -3, 900))[:2] == (T, 2)


def test_accepts_fused_qkv_column_slices():
    fused = torch.zeros(T, (HQ + 2 * HKV) * D, dtype=BF)
    q = fused[:, :HQ * D].view(T, HQ, D)
    k = fused[:, HQ * D:(HQ + HKV) * D].view(T, HKV, D)
    v = fused[:, (HQ + HKV) * D:].view(T, HKV, D)
    assert not any(t.is_contiguous() for t in (q, k, v))
    assert ops.flash_attention_varlen_validate(q, k, v, _cu()) == (T, 3, HQ, HKV, D)


def _rank_q():
    return _q().unsqueeze(0), _kv(), _kv(), _cu()


def _rank_k():
    return _q(), _kv().unsqueeze(0), _kv(), _cu()


def _rank_v():
    return _q(), _kv(), _kv()[:, 0], _cu()


def _dtype_q():
    return _q(dtype=torch.float16), _kv(), _kv(), _cu()


def _dtype_k():
    return _q(), _kv(dtype=torch.float32), _kv(), _cu()


def _dtype_v():
    return _q(), _kv(), _kv(dtype=torch.float16), _cu()


def _cu_int64():
    return _q(), _kv(), _kv(), _cu(dtype=torch.int64)


def _cu_float():
    return _q(), _kv(), _kv(), _cu(dtype=torch.float32)


def _cu_list():
    return _q(), _kv(), _kv(), [0, 13, T]


def _cu_none():
    return _q(), _kv(), _kv(), None


def _cu_wrong_device():
    return _q(), _kv(), _kv(), torch.zeros(3, dtype=torch.int32, device="meta")


def _cu_not_contiguous():
    return _q(), _kv(), _kv(), torch.zeros(8, dtype=torch.int32)[::2]


def _cu_one_boundary():
    return _q(), _kv(), _kv(), _cu(0)[:1]


def _cu_empty():
    return _q(), _kv(), _kv(), torch.zeros(0, dtype=torch.int32)


def _cu_two_dims():
    return _q(), _kv(), _kv(), torch.zeros(2, 2, dtype=torch.int32)


def _cu_too_many():
    return _q(), _kv(), _kv(), torch.zeros(65536 + 2, dtype=torch.int32)


def _head_dim():
    return _q(d=32), _kv(d=32), _kv(d=32), _cu()


def _head_dims_differ():
    return _q(), _kv(d=128), _kv(d=128), _cu()


def _group():
    return _q(hq=4), _kv(hkv=3), _kv(hkv=3), _cu()


def _token_counts_differ():
    return _q(), _kv(t=T + 1), _kv(t=T + 1), _cu()


def _kv_shapes_differ():
    return _q(), _kv(), _kv(hkv=1), _cu()


def _no_tokens():
    return _q(t=0), _kv(t=0), _kv(t=0), _cu(0, 0)


def _inner_stride():
    return torch.zeros(T, HQ, 2 * D, dtype=BF)[:, :, ::2], _kv(), _kv(), _cu()


def _row_stride():
    return _q(), torch.zeros(T, HKV * D + 4, dtype=BF)[:, :HKV * D].view(T, HKV, D), _kv(), _cu()


def _head_stride():
    return _q(), _kv(), torch.zeros(T, HKV, D + 4, dtype=BF)[:, :, :D], _cu()


def _alignment():
    return torch.zeros(T * HQ * D + 8, dtype=BF)[4:4 + T * HQ * D].view(T, HQ, D), _kv(), _kv(), _cu()


RULES = [
    (_rank_q, ValueError), (_rank_k, ValueError), (_rank_v, ValueError),
    (_dtype_q, TypeError), (_dtype_k, TypeError), (_dtype_v, TypeError),
    (_cu_int64, TypeError), (_cu_float, TypeError), (_cu_list, TypeError), (_cu_none, TypeError),
    (_cu_wrong_device, ValueError), (_cu_not_contiguous, ValueError), (_cu_one_boundary, ValueError),
    (_cu_empty, ValueError), (_cu_two_dims, ValueError), (_cu_too_many, ValueError),
    (_head_dim, ValueError), (_head_dims_differ, ValueError), (_group, ValueError),
    (_token_counts_differ, ValueError), (_kv_shapes_differ, ValueError), (_no_tokens, ValueError),
    (_inner_stride, ValueError), (_row_stride, ValueError), (_head_stride, ValueError), (_alignment, ValueError),
]


@pytest.mark.parametrize("make,error", RULES, ids=[m.__name__[1:] for m, _ in RULES])
def test_rejects(make, error):
    with pytest.raises(error, match="flash_attention_varlen") as caught:
        ops.flash_attention_varlen_validate(*make())
    assert type(caught.value) is error


def test_most_sequences_accepted():
    cu = torch.zeros(65536 + 1, dtype=torch.int32)
    assert ops.flash_attention_varlen_validate(_q(), _kv(), _kv(), cu)[1] == 65536


def test_raw_calls_refuse_before_the_extension():
    """Refused by the rule list, before the extension is touched, so CPU tensors are enough."""
    out, lse = torch.zeros(T, HQ, D, dtype=BF), torch.zeros(HQ, T)
    with pytest.raises(TypeError, match="cu_seqlens"):
        ops.flash_attention_varlen_forward(_q(), _kv(), _kv(), None)
    with pytest.raises(TypeError, match="cu_seqlens"):
        ops.flash_attention_varlen_forward(_q(), _kv(), _kv(), _cu(dtype=torch.int64), out=out, lse=lse)
    with pytest.raises(ValueError, match="dout"):
        ops.flash_attention_varlen_backward(out.unsqueeze(0), _q(), _kv(), _kv(), _cu(), out, lse)
    with pytest.raises(ValueError, match="lse"):
        ops.flash_attention_varlen_backward(out, _q(), _kv(), _kv(), _cu(), out, lse.t().contiguous())
    with pytest.raises(TypeError, match="dk"):
        ops.flash_attention_varlen_backward(out, _q(), _kv(), _kv(), _cu(), out, lse, dk=_kv().float())
    with pytest.raises(ValueError, match="dv"):
        ops.flash_attention_varlen_backward(out, _q(), _kv(), _kv(), _cu(), out, lse, dv=_kv().unsqueeze(0))
    with pytest.raises(ValueError, match="delta"):
        ops.flash_attention_varlen_backward(out, _q(), _kv(), _kv(), _cu(), out, lse, delta=torch.zeros(1, HQ, T))


# ---------------------------------------------------------------------------
# the slot map
# ---------------------------------------------------------------------------
def _boundaries(lengths):
    cu = [0]
    for n in lengths:
        cu.append(cu[-1] + n)
    return cu


def _length_lists(blk):
    edge = [0, 1, blk - 1, blk, blk + 1]
    rng = random.Random(1000 + blk)
    lists = [[n] for n in edge if n] + [edge, edge[::-1], [0, 0, 3, 0], [1] * 9, [2 * blk + 1, 0, blk, blk - 1, 3 * blk]]
    for _ in range(40):
        lists.append([rng.choice(edge + [rng.randrange(0, 4 * blk)]) for _ in range(rng.randrange(1, 12))])
    return [ls for ls in lists if sum(ls) > 0]


@pytest.mark.parametrize("blk", [FLASH_BK, FLASH_BQ])
def test_tile_map_holds_every_tile_once(blk):
    assert (FLASH_BK, FLASH_BQ) == (64, 128)
    for lengths in _length_lists(blk):
        cu = _boundaries(lengths)
        total, n = cu[-1], len(lengths)
        for given in (cu, torch.tensor(cu, dtype=torch.int32)):
            slots = ops.flash_varlen_tile_map(given, blk, total)
            assert len(slots) == total // blk + n
            assert slots == ops.flash_varlen_tile_map(given, blk)  # T defaults to cu[n]
            busy = [s for s in slots if s is not None]
            want = [(i, t, cu[i], cu[i + 1]) for i in range(n) for t in range(-(-lengths[i] // blk))]
            assert sorted(busy) == want, lengths  # every (sequence, tile) once and nothing else
            assert busy == want  # and in slot order: a sequence's slots start at cu[i] // blk + i
            for i in range(n):
                if lengths[i]:
                    assert slots[cu[i] // blk + i] == (i, 0, cu[i], cu[i + 1])


@pytest.mark.parametrize("blk", [FLASH_BK, FLASH_BQ])
def test_tile_map_truncates_the_last_sequence(blk):
    lengths = [blk + 1, 0, 3 * blk]
    cu = _boundaries(lengths)
    total = cu[-1] - blk - 7  # cu[n] > T
    slots = ops.flash_varlen_tile_map(cu, blk, total)
    assert len(slots) == total // blk + 3
    busy = [s for s in slots if s is not None]
    assert busy == [(0, 0, 0, blk + 1), (0, 1, 0, blk + 1)] + [(2, t, blk + 1, total) for t in range(2)]
    # rows [cu[n], T) belong to nobody
    slots = ops.flash_varlen_tile_map(cu, blk, cu[-1] + 5 * blk)
    assert len(slots) == cu[-1] // blk + 5 + 3
    assert [s for s in slots if s is not None] == [(i, t, cu[i], cu[i + 1]) for i in range(3)
                                                   for t in range(-(-lengths[i] // blk))]


@pytest.mark.parametrize("blk", [FLASH_BK, FLASH_BQ])
def test_tile_map_stays_inside_the_tensors_whatever_the_boundaries(blk):
    total = 5 * blk + 9
    rng = random.Random(77 + blk)
    broken = [[-5, 3, total], [0, -1, -total], [7, 3, 1, 0], [0, total + 1, total + 9], [2 ** 31 - 1] * 4,
              [-2 ** 31, 2 ** 31 - 1], [0, 4 * blk, blk, 6 * blk, 2 * blk], [total, 0], [blk, blk, blk]]
    for _ in range(60):
        broken.append([rng.choice([-2 ** 31, -1, 0, 1, blk, total, total + 1, 2 ** 31 - 1, rng.randrange(-total, 2 * total)])
                       for _ in range(rng.randrange(2, 10))])
    for cu in broken:
        slots = ops.flash_varlen_tile_map(cu, blk, total)
        assert len(slots) == total // blk + len(cu) - 1
        for s in slots:
            if s is not None:
                seq, tile, begin, end = s
                assert 0 <= seq < len(cu) - 1
                assert 0 <= begin <= end <= total
                assert tile >= 0 and tile * blk < end - begin  # its rows begin + tile * blk .. lie in [begin, end)


def test_tile_map_refuses_nonsense():
    with pytest.raises(ValueError, match="flash_varlen_tile_map"):
        ops.flash_varlen_tile_map([0, 5], 0)
    with pytest.raises(ValueError, match="flash_varlen_tile_map"):
        ops.flash_varlen_tile_map([0], 64)
    with pytest.raises(ValueError, match="flash_varlen_tile_map"):
        ops.flash_varlen_tile_map([0, 0], 64)

