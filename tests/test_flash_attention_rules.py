"""Argument rules of ``ops.flash_attention`` (``flash_attention_validate``) and of the model's
``attention`` option, on CPU tensors: no GPU is needed to accept or refuse an operand."""
import pytest
import torch

from collective_communication_mpi_amd import ops
from collective_communication_mpi_amd.parallel.llama_dp import LlamaBlock, LlamaConfig

B, S, HQ, HKV, D = 2, 5, 4, 2, 64


def _qkv(b=B, s=S, hq=HQ, hkv=HKV, d=D, dtype=torch.bfloat16):
    return (torch.zeros(b, s, hq, d, dtype=dtype), torch.zeros(b, s, hkv, d, dtype=dtype),
            torch.zeros(b, s, hkv, d, dtype=dtype))


def _offset(t, elements):
    """The same shape, contiguous, starting ``elements`` elements into a fresh buffer."""
    flat = torch.zeros(t.numel() + elements, dtype=t.dtype)
    assert flat.data_ptr() % 16 == 0
    return flat[elements:].view(t.shape)


def test_accepts_contiguous():
    assert ops.flash_attention_validate(*_qkv()) == (B, S, HQ, HKV, D)
    assert ops.flash_attention_validate(*_qkv(hq=8, hkv=1, d=128)) == (B, S, 8, 1, 128)
    assert ops.flash_attention_validate(*_qkv(b=1, s=1, hq=1, hkv=1)) == (1, 1, 1, 1, D)


def test_accepts_slices_of_a_fused_buffer():
    fused = torch.zeros(B * S, (HQ + 2 * HKV) * D, dtype=torch.bfloat16)
    q = fused[:, :HQ * D].view(B, S, HQ, D)
    k = fused[:, HQ * D:(HQ + HKV) * D].view(B, S, HKV, D)
    v = fused[:, (HQ + HKV) * D:].view(B, S, HKV, D)
    assert not q.is_contiguous() and not k.is_contiguous() and not v.is_contiguous()
    assert ops.flash_attention_validate(q, k, v) == (B, S, HQ, HKV, D)


def _bad_dtype_q():
    q, k, v = _qkv()
    return q.float(), k, v


def _bad_dtype_v():
    q, k, v = _qkv()
    return q, k, v.half()


def _bad_rank():
    q, k, v = _qkv()
    return q.view(B, S, HQ * D), k, v


def _bad_head_dim():
    return _qkv(d=32)


def _bad_head_dim_96():
    return _qkv(d=96)


def _bad_group():
    return _qkv(hq=4, hkv=3)


def _bad_empty_sequence():
    return _qkv(s=0)


def _bad_batch_mismatch():
    q, _, _ = _qkv()
    _, k, v = _qkv(b=B + 1)
    return q, k, v


def _bad_sequence_mismatch():
    q, _, _ = _qkv()
    _, k, v = _qkv(s=S + 1)
    return q, k, v


def _bad_dim_mismatch():
    q, _, _ = _qkv(d=64)
    _, k, v = _qkv(d=128)
    return q, k, v


def _bad_kv_mismatch():
    q, k, _ = _qkv()
    _, _, v = _qkv(hkv=1)
    return q, k, v


def _bad_inner_stride():
    q, k, v = _qkv()
    wide = torch.zeros(B, S, HQ, 2 * D, dtype=torch.bfloat16)
    return wide[..., ::2], k, v


def _bad_head_stride():
    q, _, v = _qkv()
    # kv heads 4 elements apart: overlapping rows of one buffer
    buf = torch.zeros(B * S * 8 * D, dtype=torch.bfloat16)
    k = buf.as_strided((B, S, HKV, D), (S * 2 * D, 2 * D, 4, 1))
    return q, k, v


def _bad_sequence_stride():
    q, k, _ = _qkv()
    row = HKV * D + 4  # rows 4 elements longer than the heads they hold
    buf = torch.zeros(B * 2 * S * row, dtype=torch.bfloat16)
    v = buf.as_strided((B, S, HKV, D), (2 * S * row, row, D, 1))
    return q, k, v


def _bad_batch_stride():
    q, k, v = _qkv()
    buf = torch.zeros(B * (S * HQ * D + 4), dtype=torch.bfloat16)
    return buf.as_strided((B, S, HQ, D), (S * HQ * D + 4, HQ * D, D, 1)), k, v


def _bad_alignment():
    q, k, v = _qkv()
    return q, _offset(k, 4), v  # 8 bytes past a 16-byte boundary


RULES = [
    (_bad_dtype_q, TypeError), (_bad_dtype_v, TypeError), (_bad_rank, ValueError), (_bad_head_dim, ValueError),
    (_bad_head_dim_96, ValueError), (_bad_group, ValueError), (_bad_empty_sequence, ValueError),
    (_bad_batch_mismatch, ValueError), (_bad_sequence_mismatch, ValueError), (_bad_dim_mismatch, ValueError),
    (_bad_kv_mismatch, ValueError), (_bad_inner_stride, ValueError), (_bad_head_stride, ValueError),
    (_bad_sequence_stride, ValueError), (_bad_batch_stride, ValueError), (_bad_alignment, ValueError),
]


@pytest.mark.parametrize("make,error", RULES, ids=[m.__name__[5:] for m, _ in RULES])
def test_rejects(make, error):
    with pytest.raises(error, match="flash_attention"):
        ops.flash_attention_validate(*make())


def test_aligned_offset_is_accepted():
    q, k, v = _qkv()
    assert ops.flash_attention_validate(q, _offset(k, 8), v) == (B, S, HQ, HKV, D)


def test_constants():
    assert ops.FLASH_BQ >= 16 and ops.FLASH_BQ % 16 == 0
    assert ops.FLASH_BK >= 32 and ops.FLASH_BK % 32 == 0


def test_model_refuses_unknown_attention():
    with pytest.raises(ValueError, match="attention"):
        LlamaBlock(LlamaConfig(d=256, heads=4, kv_heads=2, ffn=256, vocab=512, layers=1, attention="nope"), None, 0,
                   "cpu")


def test_model_refuses_flash_at_head_dim_32():
    cfg = LlamaConfig(d=128, heads=4, kv_heads=2, ffn=256, vocab=512, layers=1, attention="flash")
    assert cfg.head_dim == 32
    with pytest.raises(ValueError, match="head dim"):
        LlamaBlock(cfg, None, 0, "cpu")


def test_default_attention_is_sdpa():
    assert LlamaConfig().attention == "sdpa"
