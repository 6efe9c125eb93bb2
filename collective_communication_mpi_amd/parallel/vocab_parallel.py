"""Vocab-parallel cross-entropy: the loss of a head whose vocabulary is sharded over a TP group
(``ColumnParallelLinear(d, vocab, tp)``), without ever gathering the logits.

Rank ``r`` of ``p`` holds the columns ``[r Vloc, (r + 1) Vloc)`` of the logits as ``logits_shard``
[T, Vloc] bf16 (the rules of ``ops.cross_entropy_validate``); ``targets`` [T] int64, in global
vocabulary numbering, are the same on every rank (the same ``T`` and ``Vloc`` everywhere is the
caller's promise; nothing is exchanged on the host per call).

Forward: the stats kernel (``ops.cross_entropy_stats``, ``vocab_start = r Vloc``) writes this
rank's partials ``(m, s, zt, hit)`` [splits, T, 4] fp32 into a symmetric-heap block, one all-gather
of ``16 * splits * T`` bytes per rank fills [p, splits, T, 4], and ``ops.cross_entropy_combine``
merges every row's ``p * splits`` partials in index order (rank-major).  Every rank merges the same
partials in the same order, so ``loss``, ``lse``, ``row_loss`` and ``n_valid`` are bitwise identical
on all ranks.  Results for different TP sizes are NOT bitwise equal: the merge order differs.

Backward: local.  ``ops.cross_entropy_backward`` on this rank's shard with the global ``lse`` and
``n_valid``; the head's own backward all-reduces dX.

The forward is a collective: every rank of ``comm`` calls it in the same order.  The stats /
gathered buffers are grow-only persistent heap scratch of the group; the raw forms take
caller-allocated ones so that a captured graph can own them.  A communicator of one rank is
``ops.cross_entropy``."""
from __future__ import annotations

import torch

from ..ops.kernels import (
    cross_entropy,
    cross_entropy_backward,
    cross_entropy_combine,
    cross_entropy_stats,
    cross_entropy_validate,
    xent_row_splits,
)
from .layout import _host_comm, device_group_for


def _heap(dev, name: str, t, key: str, shape):
    """A caller's heap buffer (exact shape, fp32, contiguous, symmetric) or the group's scratch."""
    if t is None:
        return dev.scratch_view(key, shape, torch.float32)
    if t.dtype != torch.float32:
        raise TypeError(f"vocab_parallel_cross_entropy: {name} must be fp32, got {t.dtype}")
    if tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError(f"vocab_parallel_cross_entropy: {name} must be a contiguous {tuple(shape)} tensor, got "
                         f"{tuple(t.shape)}")
    if not dev.is_symmetric(t) or t.data_ptr() % 16:
        raise ValueError(f"vocab_parallel_cross_entropy: {name} must be a 16-byte-aligned symmetric-heap tensor "
                         "(comm.empty)")
    return t


def vocab_parallel_cross_entropy_forward(comm, logits_shard, targets, ignore_index: int = -100, lse=None,
                                         row_loss=None, loss_sum=None, n_valid=None, *, mean=None, work=None,
                                         stats=None, gathered=None):
    """Raw forward, a collective over ``comm``: ``(lse [T], row_loss [T], loss_sum [1])`` fp32 and
    ``n_valid [1]`` int64 of the whole vocabulary, bitwise identical on every rank.  ``stats``
    [splits, T, 4] and ``gathered`` [p, splits, T, 4] (``splits = ops.xent_row_splits(T, Vloc)``)
    are symmetric-heap fp32 buffers (default: the group's persistent scratch); ``mean`` [1] fp32
    receives ``loss_sum / n_valid`` (0 when no row is valid), ``work`` is
    ``ops.cross_entropy_combine``'s workspace.  With all of them passed the call allocates nothing
    and never synchronises with the host."""
    T, V = cross_entropy_validate(logits_shard, targets)
    p = _host_comm(comm).Get_size()
    if p == 1:  # no device plane needed
        st = cross_entropy_stats(logits_shard, targets, 0, stats)
        return cross_entropy_combine(st, targets, ignore_index, lse, row_loss, loss_sum, n_valid, mean=mean, work=work)
    dev = device_group_for(comm)
    splits = xent_row_splits(T, V)
    stats = _heap(dev, "stats", stats, "xent_stats", (splits, T, 4))
    gathered = _heap(dev, "gathered", gathered, "xent_gathered", (p, splits, T, 4))
    cross_entropy_stats(logits_shard, targets, dev.rank * V, stats)
    dev.allgather(stats, gathered, algo="auto", symmetric=True)
    return cross_entropy_combine(gathered.view(p * splits, T, 4), targets, ignore_index, lse, row_loss, loss_sum,
                                 n_valid, mean=mean, work=work)


def vocab_parallel_cross_entropy_backward(comm, logits_shard, targets, lse, n_valid, grad=None,
                                          ignore_index: int = -100, dlogits=None):
    """Raw backward, local (no collective): ``dlogits`` [T, Vloc] bf16 of this rank's shard from the
    forward's ``lse`` and ``n_valid`` (``ops.cross_entropy_backward`` with ``vocab_start = r
    Vloc``).  ``dlogits`` may be ``logits_shard``."""
    _, V = cross_entropy_validate(logits_shard, targets)
    return cross_entropy_backward(logits_shard, targets, lse, n_valid, grad, _host_comm(comm).Get_rank() * V,
                                  ignore_index, dlogits)


class _VocabParallelCrossEntropy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, targets, comm, ignore_index):
        mean = torch.empty(1, dtype=torch.float32, device=logits.device)
        lse, _, _, n_valid = vocab_parallel_cross_entropy_forward(comm, logits, targets, ignore_index, mean=mean)
        ctx.save_for_backward(logits, targets, lse, n_valid)  # nothing of size [T, V] beyond the logits
        ctx.comm, ctx.ignore_index = comm, ignore_index
        return mean.view(())

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dloss):
        logits, targets, lse, n_valid = ctx.saved_tensors
        g = dloss.to(torch.float32).reshape(1)  # stays on the device: no host synchronisation
        return (vocab_parallel_cross_entropy_backward(ctx.comm, logits, targets, lse, n_valid, g, ctx.ignore_index),
                None, None, None)


def vocab_parallel_cross_entropy(comm, logits_shard, targets, ignore_index: int = -100):
    """Differentiable mean cross-entropy (fp32 scalar, the same bits on every rank) of the logits
    whose columns are sharded over ``comm`` in rank order, over the rows whose target is not
    ``ignore_index`` (0, with zero gradients, when no row is valid).  The forward is a collective
    over ``comm`` (see the module docstring), the backward is local; a communicator of one rank is
    ``ops.cross_entropy``."""
    cross_entropy_validate(logits_shard, targets)
    if _host_comm(comm).Get_size() == 1:
        return cross_entropy(logits_shard, targets, ignore_index)
    return _VocabParallelCrossEntropy.apply(logits_shard, targets, comm, int(ignore_index))
