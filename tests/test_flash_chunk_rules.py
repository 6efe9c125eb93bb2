"""Argument rules of the chunk form of flash attention (``ops.flash_attention_chunk_validate``,
the ``dk`` / ``dv`` rules of ``ops.flash_attention_chunk_backward``) and of the model's ``cp``
option, on CPU tensors: no GPU is needed to accept or refuse an operand."""
import pytest
import torch

from collective_communication_mpi_amd import ops
from collective_communication_mpi_amd.parallel import context_parallel_attention  # noqa: F401
from collective_communication_mpi_amd.parallel.llama_dp import LlamaBlock, LlamaConfig
import test_flash_attention_rules as self_rules

B, SQ, SK, HQ, HKV, D = 2, 5, 12, 4, 2, 64
BF = torch.bfloat16


def _q(sq=SQ, hq=HQ, d=D, dtype=BF):
    return torch.zeros(B, sq, hq, d, dtype=dtype)


def _kv(sk=SK, hkv=HKV, d=D, dtype=BF):
    return torch.zeros(B, sk, hkv, d, dtype=dtype)


def _segmented(n, L, pad=0, hkv=HKV, d=D, dtype=BF):
    """[n, B, L, Hkv, D] view whose segments are ``pad`` elements further apart than they are long."""
    seg = B * L * hkv * d + pad
    buf = torch.zeros(n * seg, dtype=dtype)
    return buf.as_strided((n, B, L, hkv, d), (seg, L * hkv * d, hkv * d, d, 1))


def test_accepts_other_key_length():
    assert ops.flash_attention_chunk_validate(_q(), _kv(), _kv()) == (B, SQ, SK, SK, HQ, HKV, D)
    assert ops.flash_attention_chunk_validate(_q(sq=7), _kv(sk=3), _kv(sk=3), 0) == (B, 7, 3, 3, HQ, HKV, D)
    assert ops.flash_attention_chunk_validate(_q(sq=1), _kv(sk=1), _kv(sk=1)) == (B, 1, 1, 1, HQ, HKV, D)


def test_accepts_segments_with_padded_stride():
    k, v = _segmented(3, 4, pad=24), _segmented(3, 4, pad=8)
    assert not k.is_contiguous() and k.stride(0) != v.stride(0)
    assert ops.flash_attention_chunk_validate(_q(), k, v, 7, kv_segment=4) == (B, SQ, 12, 4, HQ, HKV, D)
    # contiguous segments, and segments of one key
    assert ops.flash_attention_chunk_validate(_q(), _segmented(2, 6), _segmented(2, 6), kv_segment=6)[2:4] == (12, 6)
    assert ops.flash_attention_chunk_validate(_q(), _segmented(12, 1, 8), _segmented(12, 1, 8), kv_segment=1)[2:4] == (12, 1)


@pytest.mark.parametrize("q_pos0", [0, 1, 7, 15, 17, 31, 33, 63, 65, 127, 129, 257, (1 << 30) - SQ])
def test_accepts_offsets_off_every_tile_grid(q_pos0):
    assert ops.flash_attention_chunk_validate(_q(), _kv(), _kv(), q_pos0)[:3] == (B, SQ, SK)


def _neg_offset():
    return (_q(), _kv(), _kv(), -1), {}


def _offset_past_limit():
    return (_q(), _kv(), _kv(), (1 << 30) - SQ + 1), {}


def _offset_not_int():
    return (_q(), _kv(), _kv(), 1.0), {}


def _segment_shapes_differ():
    return (_q(), _segmented(3, 4), _segmented(4, 3)), {"kv_segment": 4}


def _segment_length_differs():
    return (_q(), _segmented(3, 4), _segmented(3, 4)), {"kv_segment": 3}


def _segment_stride_not_8():
    return (_q(), _segmented(3, 4, pad=4), _segmented(3, 4)), {"kv_segment": 4}


def _segment_needs_5d():
    return (_q(), _kv(), _kv()), {"kv_segment": 4}


def _five_d_needs_segment():
    return (_q(), _segmented(3, 4), _segmented(3, 4)), {}


def _kv_lengths_differ():
    return (_q(), _kv(sk=12), _kv(sk=11)), {}


def _empty_keys():
    return (_q(), _kv(sk=0), _kv(sk=0)), {}


def _bad_dtype_k():
    return (_q(), _kv(dtype=torch.float16), _kv()), {}


def _bad_dtype_q():
    return (_q(dtype=torch.float32), _kv(), _kv()), {}


def _bad_head_dim():
    return (_q(d=32), _kv(d=32), _kv(d=32)), {}


def _bad_group():
    return (_q(hq=4), _kv(hkv=3), _kv(hkv=3)), {}


RULES = [
    (_neg_offset, ValueError), (_offset_past_limit, ValueError), (_offset_not_int, ValueError),
    (_segment_shapes_differ, ValueError), (_segment_length_differs, ValueError), (_segment_stride_not_8, ValueError),
    (_segment_needs_5d, ValueError), (_five_d_needs_segment, ValueError), (_kv_lengths_differ, ValueError),
    (_empty_keys, ValueError), (_bad_dtype_k, TypeError), (_bad_dtype_q, TypeError), (_bad_head_dim, ValueError),
    (_bad_group, ValueError),
]


@pytest.mark.parametrize("make,error", RULES, ids=[m.__name__[1:] for m, _ in RULES])
def test_rejects(make, error):
    args, kw = make()
    with pytest.raises(error, match="flash_attention_chunk"):
        ops.flash_attention_chunk_validate(*args, **kw)


def _backward_args(segmented):
    q = _q()
    k, v = (_segmented(3, 4, pad=8), _segmented(3, 4, pad=8)) if segmented else (_kv(), _kv())
    out, lse = torch.zeros(B, SQ, HQ, D, dtype=BF), torch.zeros(B, HQ, SQ)
    return (torch.zeros_like(out), q, k, v, out, lse), {"kv_segment": 4 if segmented else None}


@pytest.mark.parametrize("segmented", [False, True], ids=["flat", "segmented"])
def test_backward_refuses_mismatched_dk(segmented):
    """Refused before the extension is touched, so a CPU tensor is enough."""
    args, kw = _backward_args(segmented)
    good = torch.zeros_like(args[2])
    with pytest.raises(TypeError, match="dk"):
        ops.flash_attention_chunk_backward(*args, dk=good.float(), dv=good, **kw)
    with pytest.raises(TypeError, match="dv"):
        ops.flash_attention_chunk_backward(*args, dk=good, dv=good.half(), **kw)
    wrong = _kv(sk=SK + 1) if not segmented else _kv()  # another length / the flat shape of the same keys
    with pytest.raises(ValueError, match="dk"):
        ops.flash_attention_chunk_backward(*args, dk=wrong, dv=good, **kw)
    if segmented:
        with pytest.raises(ValueError, match="dv"):
            ops.flash_attention_chunk_backward(*args, dk=good, dv=_segmented(3, 4, pad=4), **kw)  # segment stride % 8


def test_self_attention_still_refuses_another_key_length():
    with pytest.raises(ValueError, match="flash_attention"):
        ops.flash_attention_validate(_q(), _kv(), _kv())
    with pytest.raises(ValueError, match="flash_attention"):
        ops.flash_attention_validate(_q(), _segmented(1, SQ), _segmented(1, SQ))


def _cases_of_both_forms():
    """Every rejecting case of the two tables that both forms can express: q, k, v with
    q_pos0 = 0 and kv_segment = None.  The self form has one sequence length, so a case of the
    chunk table gets a q of its key length, and the self table's sequence_mismatch, which is
    that one rule of its own, stays with test_self_attention_still_refuses_another_key_length."""
    cases = [("self-" + make.__name__[5:], make(), error) for make, error in self_rules.RULES
             if make is not self_rules._bad_sequence_mismatch]
    for make, error in RULES:
        (q, k, v, *offset), kw = make()
        if offset or kw:
            continue
        if k.dim() == 4 and k.shape[1] != q.shape[1]:
            q = torch.zeros(q.shape[0], k.shape[1], *q.shape[2:], dtype=q.dtype)
        cases.append(("chunk-" + make.__name__[1:], (q, k, v), error))
    return cases


BOTH = _cases_of_both_forms()


@pytest.mark.parametrize("qkv,error", [c[1:] for c in BOTH], ids=[c[0] for c in BOTH])
def test_both_forms_refuse_alike(qkv, error):
    """One rule list behind both validators: the same exception type, and messages that differ in
    the prefix only."""
    with pytest.raises(error) as as_self:
        ops.flash_attention_validate(*qkv)
    with pytest.raises(error) as as_chunk:
        ops.flash_attention_chunk_validate(*qkv, q_pos0=0, kv_segment=None)
    assert type(as_self.value) is type(as_chunk.value) is error
    said, prefix = str(as_self.value), "flash_attention"
    assert said.startswith(prefix) and not said.startswith(prefix + "_chunk")
    assert str(as_chunk.value) == prefix + "_chunk" + said[len(prefix):]


def test_both_tables_are_covered():
    """Left to one form are only the cases it alone can express: an offset, segments, another key length."""
    left_out = {"self-" + m.__name__[5:] for m, _ in self_rules.RULES} | {"chunk-" + m.__name__[1:] for m, _ in RULES}
    left_out -= {c[0] for c in BOTH}
    assert left_out == {"self-sequence_mismatch", "chunk-neg_offset", "chunk-offset_past_limit", "chunk-offset_not_int",
                        "chunk-segment_shapes_differ", "chunk-segment_length_differs", "chunk-segment_stride_not_8",
                        "chunk-segment_needs_5d"}


def test_self_validator_returns_the_chunk_validators_dims():
    fused = torch.zeros(B * SQ, (HQ + 2 * HKV) * D, dtype=BF)
    sliced = (fused[:, :HQ * D].view(B, SQ, HQ, D), fused[:, HQ * D:(HQ + HKV) * D].view(B, SQ, HKV, D),
              fused[:, (HQ + HKV) * D:].view(B, SQ, HKV, D))
    for qkv in (self_rules._qkv(), self_rules._qkv(hq=8, hkv=1, d=128), self_rules._qkv(b=1, s=1, hq=1, hkv=1), sliced):
        b, sq, sk, seg, hq, hkv, d = ops.flash_attention_chunk_validate(*qkv)
        assert sq == sk == seg
        assert ops.flash_attention_validate(*qkv) == (b, sq, hq, hkv, d)


def test_model_refuses_context_parallel_sdpa():
    cfg = LlamaConfig(d=256, heads=4, kv_heads=2, ffn=256, vocab=512, layers=1, attention="sdpa")
    with pytest.raises(ValueError, match="flash"):
        LlamaBlock(cfg, None, 0, "cpu", cp=object())
