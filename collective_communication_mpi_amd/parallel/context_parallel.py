"""Context parallelism in the all-gather form: the sequence axis of attention split over a
communicator, as Llama 3 was trained.

Rank ``r`` of ``p`` holds positions ``[r S_loc, (r + 1) S_loc)`` of q, k and v (the same ``B`` and
``S_loc`` on every rank is the caller's promise; nothing is exchanged on the host per call).

Forward: ``k | v`` are packed into one symmetric-heap buffer [2, B, S_loc, Hkv, D] (the one staging
copy), all-gathered into [p, 2, B, S_loc, Hkv, D], and the chunk kernel
(``ops.flash_attention_chunk_forward``, ``q_pos0 = r S_loc``) reads K and V from that buffer as
it is: segment ``i`` of the key axis is rank ``i``'s shard (``kv_segment = S_loc``), so the
gathered K / V are never transposed into [B, S, Hkv, D].

Backward: only the local shards, ``out`` and ``lse`` are kept between forward and backward
(O(S / p) per layer); K | V are gathered again, the chunk backward writes this rank's bf16
``dk | dv`` partials for ALL positions straight into a [p, 2, B, S_loc, Hkv, D] heap buffer (keys the
chunk cannot see get exact zeros) and one reduce-scatter (SUM) returns the local
[2, B, S_loc, Hkv, D].

Both directions are collectives: every rank of ``comm`` calls them in the same order, also a rank
that needs no gradient of its own q (autograd runs the backward when any of q, k, v of the rank
requires a gradient; a rank where none does must call ``context_parallel_attention_backward``
itself).  The gather / partial buffers are grow-only persistent heap scratch shared by all
layers of the group; the raw forms take caller-allocated ones so that a captured graph can own
them."""
from __future__ import annotations

from typing import Optional

import torch

from ..ops.kernels import (
    flash_attention_chunk,
    flash_attention_chunk_backward,
    flash_attention_chunk_forward,
    flash_attention_chunk_validate,
    flash_is_view,
)
from .layout import device_group_for


def _validate(q, k, v):
    """The local shards: q [B, S_loc, Hq, D], k / v [B, S_loc, Hkv, D] bf16 under the rules of
    ``ops.flash_attention_chunk_validate``; returns ``(B, S_loc, Hq, Hkv, D)``."""
    B, Sq, Sk, _, Hq, Hkv, D = flash_attention_chunk_validate(q, k, v)
    if Sq != Sk:
        raise ValueError(f"context_parallel_attention: q, k and v are one rank's shard of the same S_loc positions, got "
                         f"{Sq} query and {Sk} key rows")
    return B, Sq, Hq, Hkv, D


def _heap(dev, name: str, t, key: str, shape):
    """A caller's heap buffer (exact shape, bf16, contiguous, symmetric) or the group's scratch."""
    if t is None:
        return dev.scratch_view(key, shape, torch.bfloat16)
    if t.dtype != torch.bfloat16:
        raise TypeError(f"context_parallel_attention: {name} must be bf16, got {t.dtype}")
    if tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError(f"context_parallel_attention: {name} must be a contiguous {tuple(shape)} tensor, got "
                         f"{tuple(t.shape)}")
    if not dev.is_symmetric(t) or t.data_ptr() % 16:
        raise ValueError(f"context_parallel_attention: {name} must be a 16-byte-aligned symmetric-heap tensor "
                         "(comm.empty)")
    return t


def _gather_kv(dev, k, v, stage, gathered, shape):
    """k | v -> stage [2, B, S_loc, Hkv, D] -> gathered [p, 2, B, S_loc, Hkv, D]; returns the
    segmented [p, B, S_loc, Hkv, D] views of K and V."""
    p = dev.size
    stage = _heap(dev, "stage", stage, "cp_stage", (2, *shape))
    gathered = _heap(dev, "gathered", gathered, "cp_gathered", (p, 2, *shape))
    stage[0].copy_(k)
    stage[1].copy_(v)
    dev.allgather(stage, gathered, algo="auto", symmetric=True)
    return gathered[:, 0], gathered[:, 1]


def context_parallel_attention_forward(comm, q, k, v, causal: bool = True, scale: Optional[float] = None, out=None,
                                       lse=None, *, stage=None, gathered=None):
    """Raw forward, a collective over ``comm``: ``(out [B, S_loc, Hq, D] bf16, lse [B, Hq, S_loc]
    fp32)`` of this rank's queries against the keys of all ranks (causal: up to its own last
    position).  ``stage`` [2, B, S_loc, Hkv, D] and ``gathered`` [p, 2, B, S_loc, Hkv, D] are
    symmetric-heap bf16 buffers (default: the group's persistent scratch); with them, ``out`` and
    ``lse`` passed the call allocates nothing and never synchronises."""
    B, S_loc, Hq, Hkv, D = _validate(q, k, v)
    dev = device_group_for(comm)
    if dev.size == 1:
        return flash_attention_chunk_forward(q, k, v, causal, scale, out, lse)
    kg, vg = _gather_kv(dev, k, v, stage, gathered, (B, S_loc, Hkv, D))
    return flash_attention_chunk_forward(q, kg, vg, causal, scale, out, lse, q_pos0=dev.rank * S_loc, kv_segment=S_loc)


def context_parallel_attention_backward(comm, dout, q, k, v, out, lse, causal: bool = True,
                                        scale: Optional[float] = None, dq=None, dkv=None, delta=None, *, stage=None,
                                        gathered=None, partial=None):
    """Raw backward, a collective over ``comm``: returns ``(dq, dk, dv)`` of the local shards,
    ``dk`` and ``dv`` the halves of ``dkv`` [2, B, S_loc, Hkv, D] bf16 contiguous.  K | V are
    gathered again (``stage``, ``gathered`` as in the forward); ``partial``
    [p, 2, B, S_loc, Hkv, D] is the symmetric-heap buffer the chunk backward writes this rank's
    bf16 partials of every rank's dk | dv into, and the reduce-scatter's source.  The partials
    are rounded to bf16 once before the sum and the sum once after it."""
    B, S_loc, Hq, Hkv, D = _validate(q, k, v)
    dev = device_group_for(comm)
    shape = (B, S_loc, Hkv, D)
    if dkv is None:
        dkv = torch.empty((2, *shape), dtype=torch.bfloat16, device=q.device)
    elif dkv.dtype != torch.bfloat16:
        raise TypeError(f"context_parallel_attention: dkv must be bf16, got {dkv.dtype}")
    elif tuple(dkv.shape) != (2, *shape) or not dkv.is_contiguous() or dkv.device != q.device:
        raise ValueError(f"context_parallel_attention: dkv must be a contiguous {(2, *shape)} tensor on {q.device}")
    if dev.size == 1:
        dq, _, _ = flash_attention_chunk_backward(dout, q, k, v, out, lse, causal, scale, dq, dkv[0], dkv[1], delta)
        return dq, dkv[0], dkv[1]
    p = dev.size
    partial = _heap(dev, "partial", partial, "cp_partial", (p, 2, *shape))
    kg, vg = _gather_kv(dev, k, v, stage, gathered, shape)
    dq, _, _ = flash_attention_chunk_backward(dout, q, kg, vg, out, lse, causal, scale, dq, partial[:, 0], partial[:, 1],
                                              delta, q_pos0=dev.rank * S_loc, kv_segment=S_loc)
    dev.reduce_scatter(partial, dkv, "SUM", symmetric=True)
    return dq, dkv[0], dkv[1]


class _ContextParallelAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, comm, causal, scale):
        out, lse = context_parallel_attention_forward(comm, q, k, v, causal, scale)
        ctx.save_for_backward(q, k, v, out, lse)  # the local shards only: the gathered K | V are not kept
        ctx.comm, ctx.causal, ctx.scale = comm, causal, scale
        ctx.mark_non_differentiable(lse)
        return out, lse

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout, _dlse):
        q, k, v, out, lse = ctx.saved_tensors
        if not flash_is_view(dout):
            dout = dout.contiguous()
        dq, dk, dv = context_parallel_attention_backward(ctx.comm, dout, q, k, v, out, lse, ctx.causal, ctx.scale)
        return dq, dk, dv, None, None, None


def context_parallel_attention(comm, q, k, v, causal: bool = True, scale: Optional[float] = None):
    """Differentiable attention of this rank's shard ``q`` [B, S_loc, Hq, D], ``k`` / ``v``
    [B, S_loc, Hkv, D] (bf16) over the sequence held by all ranks of ``comm`` in rank order:
    ``out`` [B, S_loc, Hq, D] bf16.  Forward and backward are collectives over ``comm`` (see the
    module docstring); a communicator of one rank is ``ops.flash_attention_chunk``."""
    _validate(q, k, v)
    if device_group_for(comm).size == 1:
        return flash_attention_chunk(q, k, v, causal, scale)
    return _ContextParallelAttention.apply(q, k, v, comm, bool(causal), scale)[0]
