"""Rotary position embedding on the CPU: every refusal of ``ops.rope_validate`` with its exception
type, ``ops.rope_table`` against ``math.cos`` / ``math.sin``, the defining properties of the fp64
mirror ``ops.rope_reference``, and the model's configuration rules.  No GPU is needed to accept or
refuse an operand."""
import math

import pytest
import torch

from collective_communication_mpi_amd import ops
from collective_communication_mpi_amd.parallel.llama_dp import LlamaBlock, LlamaConfig, LlamaModel

B, S, T, HQ, HKV, D, P = 2, 6, 40, 4, 2, 64, 64
BF = torch.bfloat16


def _x(*shape, dtype=BF):
    return torch.zeros(*shape, dtype=dtype)


def _table(p=P, d=D, dtype=torch.float32):
    return torch.zeros(p, 2, d // 2, dtype=dtype)


def _cu(*bounds, dtype=torch.int32):
    return torch.tensor(bounds or (0, 13, 13, T), dtype=dtype)


def test_accepts():
    q, k = _x(B, S, HQ, D), _x(B, S, HKV, D)
    assert ops.rope_validate(q, k, _table()) == (B, S, HQ, HKV, D, P)
    assert ops.rope_validate(q, None, _table()) == (B, S, HQ, 0, D, P)
    assert ops.rope_validate(q, k, _table(), P - S) == (B, S, HQ, HKV, D, P)  # pos0 + S = P is the last that fits
    # the heads are independent: no GQA rule here
    assert ops.rope_validate(_x(B, S, 3, D), _x(B, S, 5, D), _table())[2:4] == (3, 5)
    for d in (16, 80, 256):
        assert ops.rope_validate(_x(1, 1, 1, d), None, _table(1, d)) == (1, 1, 1, 0, d, 1)
    # packed; the contents of cu_seqlens are the caller's promise and are read on the device only
    assert ops.rope_validate(_x(T, HQ, D), _x(T, HKV, D), _table(), cu_seqlens=_cu()) == (1, T, HQ, HKV, D, P)
    assert ops.rope_validate(_x(T, HQ, D), None, _table(8), cu_seqlens=_cu(5, -3, 900))[:2] == (1, T)
    # outputs: views of their own, or the inputs themselves
    assert ops.rope_validate(q, k, _table(), q_out=q, k_out=_x(B, S, HKV, D))[0] == B


def test_accepts_fused_qkv_column_slices():
    fused = torch.zeros(T, (HQ + 2 * HKV) * D, dtype=BF)
    q = fused[:, :HQ * D].view(T, HQ, D)
    k = fused[:, HQ * D:(HQ + HKV) * D].view(T, HKV, D)
    assert not q.is_contiguous() and not k.is_contiguous()
    assert ops.rope_validate(q, k, _table(), cu_seqlens=_cu(), q_out=q, k_out=k) == (1, T, HQ, HKV, D, P)
    assert ops.rope_validate(q.view(2, T // 2, HQ, D), k.view(2, T // 2, HKV, D), _table()) == (2, T // 2, HQ, HKV, D, P)


def _odd_stride():
    return torch.zeros(B, S, HQ, D + 4, dtype=BF)[..., :D]


def _misaligned(shape):
    n = math.prod(shape)
    return torch.zeros(n + 8, dtype=BF)[4:4 + n].view(*shape)


TYPE_ERRORS = {
    "q fp16": lambda: (_x(B, S, HQ, D, dtype=torch.float16), None, _table()),
    "k fp32": lambda: (_x(B, S, HQ, D), _x(B, S, HKV, D, dtype=torch.float32), _table()),
    "table fp64": lambda: (_x(B, S, HQ, D), None, _table(dtype=torch.float64)),
    "table bf16": lambda: (_x(B, S, HQ, D), None, _table(dtype=BF)),
    "cu int64": lambda: (_x(T, HQ, D), None, _table(), 0, _cu(dtype=torch.int64)),
    "cu list": lambda: (_x(T, HQ, D), None, _table(), 0, [0, T]),
    "q_out fp32": lambda: (_x(B, S, HQ, D), None, _table(), 0, None, _x(B, S, HQ, D, dtype=torch.float32)),
    "k_out fp16": lambda: (_x(B, S, HQ, D), _x(B, S, HKV, D), _table(), 0, None, None,
                           _x(B, S, HKV, D, dtype=torch.float16)),
}

VALUE_ERRORS = {
    "rank 3 with pos0": lambda: (_x(T, HQ, D), None, _table()),
    "rank 4 with cu_seqlens": lambda: (_x(B, S, HQ, D), None, _table(), 0, _cu()),
    "rank 5": lambda: (_x(1, B, S, HQ, D), None, _table()),
    "cu_seqlens and pos0": lambda: (_x(T, HQ, D), None, _table(), 3, _cu()),
    "negative pos0": lambda: (_x(B, S, HQ, D), None, _table(), -1),
    "pos0 not an int": lambda: (_x(B, S, HQ, D), None, _table(), 1.0),
    "pos0 a bool": lambda: (_x(B, S, HQ, D), None, _table(), True),
    "k other batch": lambda: (_x(B, S, HQ, D), _x(B + 1, S, HKV, D), _table()),
    "k other length": lambda: (_x(B, S, HQ, D), _x(B, S + 1, HKV, D), _table()),
    "k other head dim": lambda: (_x(B, S, HQ, D), _x(B, S, HKV, D // 2), _table()),
    "k other rank": lambda: (_x(B, S, HQ, D), _x(B * S, HKV, D), _table()),
    "packed k other T": lambda: (_x(T, HQ, D), _x(T - 1, HKV, D), _table(), 0, _cu()),
    "k_out without k": lambda: (_x(B, S, HQ, D), None, _table(), 0, None, None, _x(B, S, HKV, D)),
    "D = 8": lambda: (_x(B, S, HQ, 8), None, _table(d=8)),
    "D = 24": lambda: (_x(B, S, HQ, 24), None, _table(d=24)),
    "D = 272": lambda: (_x(B, S, HQ, 272), None, _table(d=272)),
    "no tokens": lambda: (_x(B, 0, HQ, D), None, _table()),
    "no heads": lambda: (_x(B, S, 0, D), None, _table()),
    "table for another D": lambda: (_x(B, S, HQ, D), None, _table(d=D // 2)),
    "table rank 2": lambda: (_x(B, S, HQ, D), None, torch.zeros(P, D)),
    "table [P, 1, D/2]": lambda: (_x(B, S, HQ, D), None, torch.zeros(P, 1, D // 2)),
    "table without rows": lambda: (_x(B, S, HQ, D), None, _table(0)),
    "table not contiguous": lambda: (_x(B, S, HQ, D), None, torch.zeros(P, 2, D)[..., ::2]),
    "table misaligned": lambda: (_x(B, S, HQ, D), None, torch.zeros(P * D + 3)[1:1 + P * D].view(P, 2, D // 2)),
    "pos0 + S > P": lambda: (_x(B, S, HQ, D), None, _table(), P - S + 1),
    "S > P": lambda: (_x(B, S, HQ, D), None, _table(S - 1)),
    "cu_seqlens one boundary": lambda: (_x(T, HQ, D), None, _table(), 0, _cu(0)),
    "cu_seqlens rank 2": lambda: (_x(T, HQ, D), None, _table(), 0, _cu().view(2, 2)),
    "cu_seqlens strided": lambda: (_x(T, HQ, D), None, _table(), 0, torch.zeros(8, dtype=torch.int32)[::2]),
    "too many sequences": lambda: (_x(T, HQ, D), None, _table(), 0, torch.zeros(ops.ROPE_MAX_SEQS + 2, dtype=torch.int32)),
    "q stride on D": lambda: (_x(B, S, HQ, 2 * D)[..., ::2], None, _table()),
    "q head stride not a multiple of 8": lambda: (_odd_stride(), None, _table()),
    "q misaligned": lambda: (_misaligned((B, S, HQ, D)), None, _table()),
    "k misaligned": lambda: (_x(B, S, HQ, D), _misaligned((B, S, HKV, D)), _table()),
    "q_out other shape": lambda: (_x(B, S, HQ, D), None, _table(), 0, None, _x(B, S, HQ + 1, D)),
    "q_out odd stride": lambda: (_x(B, S, HQ, D), None, _table(), 0, None, _odd_stride()),
    "q_out misaligned": lambda: (_x(B, S, HQ, D), None, _table(), 0, None, _misaligned((B, S, HQ, D))),
    "k_out other shape": lambda: (_x(B, S, HQ, D), _x(B, S, HKV, D), _table(), 0, None, None, _x(B, S, HQ, D)),
}


@pytest.mark.parametrize("case", sorted(TYPE_ERRORS))
def test_refuses_dtypes_with_type_error(case):
    with pytest.raises(TypeError):
        ops.rope_validate(*TYPE_ERRORS[case]())


@pytest.mark.parametrize("case", sorted(VALUE_ERRORS))
def test_refuses_the_rest_with_value_error(case):
    with pytest.raises(ValueError):
        ops.rope_validate(*VALUE_ERRORS[case]())


def test_in_place_means_the_same_view():
    buf = torch.zeros(B, S, HQ, 2 * D, dtype=BF)
    q = buf[..., :D]
    other = buf.view(-1)[:B * S * HQ * D].view(B, S, HQ, D)  # the same address, other strides
    assert ops.rope_validate(q, None, _table(), q_out=q)[0] == B
    with pytest.raises(ValueError, match="in place"):
        ops.rope_validate(q, None, _table(), q_out=other)


def test_the_public_calls_validate_before_anything_else():
    """``rope_apply`` and ``rope`` refuse on the CPU, before they reach for the extension."""
    with pytest.raises(ValueError):
        ops.rope_apply(_x(B, S, HQ, D), None, _table(), P)
    with pytest.raises(TypeError):
        ops.rope(_x(B, S, HQ, D, dtype=torch.float32), None, _table())
    with pytest.raises(ValueError):
        ops.rope(_x(T, HQ, D), None, _table(), pos0=1, cu_seqlens=_cu())


# --- the table ---------------------------------------------------------------------------------

@pytest.mark.parametrize("d", [16, 128])
def test_table_against_math(d):
    """fp64 angles, one rounding to fp32: each entry is the fp32 nearest to math.cos / math.sin of
    ``p * theta^(-2j/d)`` up to the last bit of the fp64 evaluation (|difference| <= 2^-25, half an
    fp32 ulp of a value below 1, plus 2^-40 for the fp64 argument and libm)."""
    n_pos, theta = 8192, 500000.0
    t = ops.rope_table(n_pos, d, theta)
    assert t.shape == (n_pos, 2, d // 2) and t.dtype == torch.float32 and t.is_contiguous() and t.device.type == "cpu"
    for p in (0, 1, 4095, n_pos - 1):
        for j in range(d // 2):
            a = p * theta ** (-2.0 * j / d)
            assert abs(t[p, 0, j].item() - math.cos(a)) <= 2.0 ** -25 + 2.0 ** -40, (p, j)
            assert abs(t[p, 1, j].item() - math.sin(a)) <= 2.0 ** -25 + 2.0 ** -40, (p, j)
    assert torch.equal(t[0, 0], torch.ones(d // 2)) and torch.equal(t[0, 1], torch.zeros(d // 2))


def test_table_with_custom_inv_freq():
    d, n_pos = 16, 100
    inv = torch.tensor([0.5 ** j / 3.0 for j in range(d // 2)], dtype=torch.float64)
    t = ops.rope_table(n_pos, d, inv_freq=inv)
    for p in (0, 1, 57, n_pos - 1):
        for j in range(d // 2):
            a = p * inv[j].item()
            assert abs(t[p, 0, j].item() - math.cos(a)) <= 2.0 ** -25 + 2.0 ** -40
            assert abs(t[p, 1, j].item() - math.sin(a)) <= 2.0 ** -25 + 2.0 ** -40
    assert not torch.equal(t, ops.rope_table(n_pos, d))
    with pytest.raises(TypeError):
        ops.rope_table(n_pos, d, inv_freq=inv.float())
    with pytest.raises(ValueError):
        ops.rope_table(n_pos, d, inv_freq=inv[:-1])
    with pytest.raises(ValueError):
        ops.rope_table(0, d)
    with pytest.raises(ValueError):
        ops.rope_table(n_pos, 15)


# --- the fp64 mirror -----------------------------------------------------------------------------
# The table is fp32: c^2 + s^2 = 1 up to two roundings of 2^-24 relative each, |c^2 + s^2 - 1| <=
# 2^-22 with room to spare.  Every property below holds to that, not to fp64's last bit.
UNIT = 2.0 ** -22


def _pairs(x, interleaved):
    d = x.shape[-1]
    return (x[..., 0::2], x[..., 1::2]) if interleaved else (x[..., :d // 2], x[..., d // 2:])


@pytest.mark.parametrize("interleaved", [False, True])
def test_reference_properties(interleaved):
    g = torch.Generator().manual_seed(11)
    d, n_pos = 32, 300
    table = ops.rope_table(n_pos, d)
    x = torch.randn(2, 50, 3, d, generator=g, dtype=torch.float64)
    pos = torch.randint(0, n_pos, (2, 50), generator=g)
    pos[0, 0] = 0
    y = ops.rope_reference(x, table, pos, interleaved)
    assert y.dtype == torch.float64 and y.shape == x.shape
    # each pair's norm is preserved
    (x1, x2), (y1, y2) = _pairs(x, interleaved), _pairs(y, interleaved)
    n_in, n_out = x1 ** 2 + x2 ** 2, y1 ** 2 + y2 ** 2
    assert ((n_out - n_in).abs() <= UNIT * n_in).all()
    # position 0 is the identity, exactly
    assert torch.equal(y[0, 0], x[0, 0])
    # inverse=True undoes it
    back = ops.rope_reference(y, table, pos, interleaved, inverse=True)
    assert ((back - x).abs() <= UNIT * (x1.abs() + x2.abs()).max()).all()
    # and is the transpose: <R x, g> = <x, R^T g> (the same products in another order)
    gr = torch.randn(x.shape, generator=g, dtype=torch.float64)
    lhs, rhs = (y * gr).sum(), (x * ops.rope_reference(gr, table, pos, interleaved, inverse=True)).sum()
    assert abs(lhs - rhs) <= 1e-12 * (x.abs() * gr.abs()).sum()


@pytest.mark.parametrize("interleaved", [False, True])
def test_reference_scores_depend_on_the_distance_only(interleaved):
    """<R_i q, R_j k> = <q, R_(j - i) k>: the same q and k at positions (i, j) and (i + m, j + m)
    give the same score.  Angles are p * f in fp64 and the table rounds cos / sin to fp32, so the
    two sides agree to a few 2^-24 |q| |k|."""
    g = torch.Generator().manual_seed(5)
    d, n_pos = 64, 512
    table = ops.rope_table(n_pos, d, theta=10000.0)
    q = torch.randn(1, 1, 1, d, generator=g, dtype=torch.float64)
    k = torch.randn(1, 1, 1, d, generator=g, dtype=torch.float64)
    bound = 8 * 2.0 ** -24 * (q.norm() * k.norm()).item()

    def score(i, j):
        qi = ops.rope_reference(q, table, torch.tensor([[i]]), interleaved)
        kj = ops.rope_reference(k, table, torch.tensor([[j]]), interleaved)
        return (qi * kj).sum().item()

    for i, j in ((0, 0), (7, 3), (100, 31), (3, 250)):
        base = score(i, j)
        for m in (1, 17, 200):
            assert abs(score(i + m, j + m) - base) <= bound, (i, j, m)
    assert abs(score(7, 3) - score(7, 4)) > 100 * bound  # and it does depend on the distance


def test_reference_interleaved_is_half_split_on_deinterleaved_input():
    g = torch.Generator().manual_seed(2)
    d = 16
    table = ops.rope_table(40, d)
    x = torch.randn(3, 2, d, generator=g, dtype=torch.float64)
    pos = torch.tensor([5, 0, 39])
    de = torch.cat((x[..., 0::2], x[..., 1::2]), dim=-1)
    half = ops.rope_reference(de, table, pos)
    re = torch.stack((half[..., :d // 2], half[..., d // 2:]), dim=-1).reshape(x.shape)
    assert torch.equal(ops.rope_reference(x, table, pos, interleaved=True), re)
    with pytest.raises(ValueError):
        ops.rope_reference(x, table, pos.int())
    with pytest.raises(ValueError):
        ops.rope_reference(x, table, pos[:2])


# --- the model's configuration ---------------------------------------------------------------------
TINY = dict(d=256, heads=4, kv_heads=2, ffn=256, vocab=512, layers=1)


def test_config_defaults_keep_rope_off():
    cfg = LlamaConfig()
    assert cfg.rope is False and cfg.rope_theta == 500000.0 and cfg.max_positions == 8192
    assert LlamaConfig(**TINY).rope is False


def test_config_errors_fire_without_a_gpu():
    with pytest.raises(ValueError, match="head dim"):  # head dim 8
        LlamaBlock(LlamaConfig(d=64, heads=8, kv_heads=2, ffn=64, vocab=64, layers=1, rope=True), None, 0, "cpu")
    with pytest.raises(ValueError, match="max_positions"):
        LlamaBlock(LlamaConfig(**TINY, rope=True, max_positions=0), None, 0, "cpu")
    with pytest.raises(ValueError, match="rope_theta"):
        LlamaModel(LlamaConfig(**TINY, rope=True, rope_theta=0.0), None, "cpu")
    with pytest.raises(ValueError, match="rope_table"):  # a block of a rope model needs the model's table
        LlamaBlock(LlamaConfig(**TINY, rope=True), None, 0, "cpu")


def test_grid_limit_is_a_rule():
    """tokens x D / 16 x min(heads, 64) beyond 256 x (2^31 - 1) threads is refused by the rules,
    not only by the extension (expanded tensors: no memory behind them)."""
    d = 256
    big = torch.zeros(1, 1, 1, d, dtype=BF).expand(1, 1 << 30, 64, d)
    with pytest.raises(ValueError, match="grid"):
        ops.rope_validate(big, None, torch.zeros(1, dtype=torch.float32).as_strided((1 << 30, 2, d // 2), (0, 0, 0)))
    ok = torch.zeros(1, 1, 1, d, dtype=BF).expand(1, 1 << 30, 7, d)  # 2^30 x 16 x 7 threads fit
    with pytest.raises(ValueError, match="contiguous"):  # the next rule in line: the stand-in table
        ops.rope_validate(ok, None, torch.zeros(1, dtype=torch.float32).as_strided((1 << 30, 2, d // 2), (0, 0, 0)))


class StubComm:
    def __init__(self, size, rank=0):
        self.size, self.rank = size, rank

    def Get_size(self):
        return self.size

    def Get_rank(self):
        return self.rank


def test_max_positions_is_enforced_before_anything_runs():
    """A sequence (under cp: cp_size x seq) beyond max_positions raises from ``LlamaModel.forward``
    before the embedding, and from ``LlamaBlock.forward`` before its norm: on the CPU, where any
    launch of a device kernel would fail instead."""
    cfg = LlamaConfig(**TINY, attention="flash", loss="fused", rope=True, max_positions=8)
    model = LlamaModel(cfg, StubComm(1), "cpu")
    assert model.rope_table.shape == (8, 2, 32)
    with pytest.raises(ValueError, match="max_positions"):
        model(torch.zeros(2, 9, dtype=torch.long))
    with pytest.raises(ValueError, match="max_positions"):
        model.blocks[0](torch.zeros(18, 256, dtype=BF), 2, 9)
    split = LlamaBlock(cfg, StubComm(1), 0, "cpu", cp=StubComm(3, 1), rope_table=model.rope_table)
    assert (split.cp_size, split.cp_rank) == (3, 1)
    split.check_positions(2)
    with pytest.raises(ValueError, match="3 x 3 positions"):
        split(torch.zeros(6, 256, dtype=BF), 2, 3)
    LlamaBlock(LlamaConfig(**TINY), StubComm(1), 0, "cpu").check_positions(10 ** 9)  # rope=False: no rule
