"""The routed MoE collectives as differentiable functions, and a routed MoE layer.

``moe_dispatch`` and ``moe_combine`` wrap ``DeviceGroup.moe_dispatch`` / ``moe_combine`` for
autograd.  The backward of the dispatch is the unweighted combine of the incoming gradient
(``dx[t] = sum_k d_recv_owner[row_of[t, k]]``, the fp32 slot-ordered sum of the forward
kernel); the backward of the combine is one kernel, ``DeviceGroup.moe_combine_backward``
(``dy_owner[row_of[t, k]] = w[t, k] * dout[t]`` pushed into the owners' buffers,
``dweights[t, k] = <dout[t], y_owner[row_of[t, k]]>`` pulled from them).

Three things to know:

* The backward passes contain collectives.  Every rank of the group must run them, in
  the same order, also a rank with ``T == 0`` tokens: on every rank ``x`` (for the
  dispatch) and ``y`` (for the combine) must take part in a graph that is differentiated.
  Whether ``weights`` needs a gradient must not differ between ranks either: a rank that
  computes ``dweights`` reads ``y`` on every rank, which publishes it only when it does too.
* The collectives read and write peers' memory, so ``recv_x``, ``y``, the gradient of
  ``recv_x`` and the gradient of ``y`` live in the symmetric heap.  A tensor that is not
  already there (the expert block's output, the gradient autograd hands in) is copied into
  a heap buffer first; these staging copies of ``[cap, D]`` are the only extra passes over
  the payload.  Whether a tensor needs staging must not differ between ranks (it does
  not when every rank runs the same model code): the allocation is collective.
* Heap buffers are allocated per call (``group.empty``: a collective host call, the same
  sequence on every rank) and owned by their tensors: a block returns to the heap when
  the last reference -- the autograd graph's included -- is gone.
"""
from __future__ import annotations

import math

import torch

from .. import ops
from .moe_experts import GroupedExpertsMLP


def _dev(group):
    """The DeviceGroup of ``group`` (a DeviceGroup, or a Communicator holding one)."""
    return getattr(group, "dev", group)


def _in_heap(dev, t: torch.Tensor) -> torch.Tensor:
    """``t`` itself when it is a contiguous, 16-B aligned symmetric-heap tensor, else a
    copy of it in a new heap buffer (collective allocation)."""
    if t.is_contiguous() and t.data_ptr() % 16 == 0 and dev.is_symmetric(t):
        return t
    buf = dev.empty(tuple(t.shape), t.dtype)
    buf.copy_(t)
    return buf


def _aligned(t: torch.Tensor) -> torch.Tensor:
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


class _Dispatch(torch.autograd.Function):
    """Ties ``recv_x``, which the dispatch already filled, to ``x`` in the autograd graph."""

    @staticmethod
    def forward(ctx, x, recv_x, dev, handle):
        ctx.dev, ctx.handle = dev, handle
        return recv_x.view_as(recv_x)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_recv):
        dx = ctx.dev.moe_combine(_in_heap(ctx.dev, d_recv), ctx.handle, None)
        return dx, None, None, None


class _Combine(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, weights, dev, handle):
        ys = _in_heap(dev, y)
        w = None if weights is None else weights.contiguous()
        ctx.dev, ctx.handle = dev, handle
        ctx.save_for_backward(ys, w)
        return dev.moe_combine(ys, handle, w)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        ys, w = ctx.saved_tensors
        dev = ctx.dev
        want_dw = w is not None and ctx.needs_input_grad[1]
        dy = dev.empty(tuple(ys.shape), ys.dtype)
        dy, dw = dev.moe_combine_backward(_aligned(dout), ctx.handle, w, y=ys if want_dw else None, dy=dy)
        return dy, dw, None, None


def moe_dispatch(group, x, topk_idx, num_experts: int, cap: int, *, expert_capacity=None):
    """Differentiable ``group.moe_dispatch``: ``x`` [T, D] and ``topk_idx`` [T, K] give
    ``(recv_x, handle)``, ``recv_x`` [cap, D] allocated from the symmetric heap.
    Differentiable in ``x``; the backward stages the gradient of ``recv_x`` into the heap
    when needed and runs the unweighted ``moe_combine`` (a collective: see the module
    notes).  Rows of the gradient at or past the rank's total are never read.
    ``expert_capacity`` (the same on every rank) is the dispatch's: an entry over its
    expert's capacity is dropped (``row_of`` -1, counted in ``handle.num_dropped``), takes no
    row and gets no gradient."""
    dev = _dev(group)
    recv_x = dev.empty((int(cap), x.shape[1]), x.dtype)
    handle = dev.moe_dispatch(_aligned(x.detach()), topk_idx, int(num_experts), recv_x,
                              expert_capacity=expert_capacity)
    return _Dispatch.apply(x, recv_x, dev, handle), handle


def moe_combine(group, y, handle, weights=None):
    """Differentiable ``group.moe_combine``: ``out[t] = sum_k w[t, k] * y_owner[row_of[t, k]]``.
    Differentiable in ``y`` [>= cap, D] and ``weights`` [T, K] fp32.  The forward stages ``y``
    into the heap when needed and keeps that buffer; the backward is one
    ``moe_combine_backward`` (a collective: see the module notes), which computes
    ``dweights`` only when ``weights`` needs a gradient.  The gradient of ``y`` is a heap
    buffer whose rows at or past the rank's total are unspecified, the contract
    ``grouped_linear`` has for its inputs."""
    return _Combine.apply(y, weights, _dev(group), handle)


class RoutedMoE(torch.nn.Module):
    """A routed mixture-of-experts layer over the ranks of ``group``: ``num_experts``
    SwiGLU experts, ``num_experts // p`` consecutive ones per rank, ``top_k`` per token.

    ``forward(x)`` with this rank's tokens ``x`` [T, d_model] in bf16, the grouped GEMMs'
    input type (T may differ per rank and be 0): router logits ``x . router^T`` in fp32,
    softmax and ``topk`` in torch (they are [T, E]-sized; ``gate="fused"``: one kernel), the chosen probabilities renormalised to sum to one per token
    (``renormalize``), then ``moe_dispatch -> GroupedExpertsMLP -> moe_combine``.  Gradients
    reach the router through the combine's ``dweights``, and ``x`` through both the
    dispatch backward and the router.  ``capacity`` is the number of rows of every rank's
    receive buffer: a host-known bound on the rows one rank can receive (at most
    ``top_k`` times all ranks' tokens).  ``last_handle`` is the most recent forward's
    ``MoEHandle`` (``topk_idx``, ``row_of``, ``expert_counts``).  Forward and backward are
    collectives: every rank runs both.

    ``expert_capacity`` (None: no limit; the same on every rank) caps the rows of every
    expert: the first ``expert_capacity`` entries of an expert in (source rank, token, slot)
    order are kept, the others dropped without an error -- they add nothing to the output
    and get no gradient; the weights of a token's kept slots are not renormalised again.
    ``last_handle.num_dropped`` counts this rank's dropped entries.  ``capacity`` must then be
    at least ``(num_experts / p) * expert_capacity``, which is also all it needs to be:
    ``capacity_for`` gives the usual ``factor * tokens * top_k / num_experts``.

    ``gate="fused"`` computes the same logits and hands them to ``ops.moe_gate`` (softmax,
    top-k, renormalisation and the statistics below in one kernel, one more for the
    backward); ``gate="torch"`` is the chain of torch ops.  The two agree up to fp32 rounding,
    and on ties between logits the fused gate takes the lower expert index.

    ``router_logits="mfma"`` computes the logits with ``ops.moe_router_logits``: the fp32 router
    as three bf16 planes on the matrix cores, one pass over ``x``, and no fp32 copy of ``x`` kept
    for the backward; ``"torch"`` (the default) is ``x.float() @ router.t()``.  Both gates take
    either result unchanged.  The two settings agree up to fp32 rounding (they sum in different
    orders) and may pick different experts where two logits are closer than that.

    After a forward ``aux_loss`` is the Switch load-balancing loss of this rank's tokens,
    ``E * sum_e f_e P_e`` with ``f_e`` the share of the T * K selections that chose expert e
    (detached) and ``P_e`` the mean router probability of e; 1 at perfect balance, 0 when
    T = 0.  It is not scaled: ``aux_loss_coef`` is only stored, for the caller's
    ``loss + layer.aux_loss_coef * layer.aux_loss``."""

    def __init__(self, group, d_model: int, d_ff: int, num_experts: int, top_k: int, capacity: int,
                 renormalize: bool = True, dtype=torch.bfloat16, expert_capacity=None, gate: str = "torch",
                 aux_loss_coef: float = 0.0, router_logits: str = "torch"):
        super().__init__()
        dev = _dev(group)
        if num_experts < 1 or num_experts % dev.size:
            raise ValueError(f"RoutedMoE: num_experts ({num_experts}) must be a positive multiple of the group "
                             f"size ({dev.size})")
        if not 1 <= top_k <= min(8, num_experts):
            raise ValueError("RoutedMoE: top_k must be in [1, min(8, num_experts)]")
        if capacity < 1:
            raise ValueError("RoutedMoE: capacity must be at least one row")
        if gate not in ("torch", "fused"):
            raise ValueError(f"RoutedMoE: gate must be 'torch' or 'fused', got {gate!r}")
        if router_logits not in ("torch", "mfma"):
            raise ValueError(f"RoutedMoE: router_logits must be 'torch' or 'mfma', got {router_logits!r}")
        if expert_capacity is not None:
            expert_capacity = int(expert_capacity)
            if expert_capacity < 1:
                raise ValueError("RoutedMoE: expert_capacity must be at least 1")
            if capacity < (num_experts // dev.size) * expert_capacity:
                raise ValueError(f"RoutedMoE: capacity ({capacity}) must be at least (num_experts / p) * "
                                 f"expert_capacity = {(num_experts // dev.size) * expert_capacity}")
        self.group, self.num_experts, self.top_k, self.capacity = dev, num_experts, top_k, int(capacity)
        self.renormalize = renormalize
        self.expert_capacity, self.gate, self.aux_loss_coef = expert_capacity, gate, float(aux_loss_coef)
        self.router_logits = router_logits
        self.aux_loss = None
        self.router = torch.nn.Parameter(torch.randn(num_experts, d_model, device=dev.device, dtype=torch.float32)
                                         / math.sqrt(d_model))
        self.experts = GroupedExpertsMLP(num_experts // dev.size, d_model, d_ff, device=dev.device, dtype=dtype)
        self.last_handle = None

    @staticmethod
    def capacity_for(tokens_all_ranks: int, top_k: int, num_experts: int, factor: float = 1.0) -> int:
        """The per-expert capacity ``ceil(factor * tokens_all_ranks * top_k / num_experts)``:
        ``factor`` times an expert's rows under perfectly balanced routing."""
        return int(math.ceil(factor * tokens_all_ranks * top_k / num_experts))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        T = x.shape[0]
        if self.router_logits == "mfma":
            logits = ops.moe_router_logits(x, self.router)
        else:
            logits = x.float() @ self.router.t()
        if self.gate == "fused":
            w, idx, prob_sum, expert_tokens = ops.moe_gate(logits, self.top_k, self.renormalize)
        else:
            probs = torch.softmax(logits, dim=-1)
            w, idx = probs.topk(self.top_k, dim=-1)
            if self.renormalize:
                w = w / w.sum(dim=-1, keepdim=True)
            prob_sum = probs.sum(dim=0)
            expert_tokens = torch.zeros(self.num_experts, dtype=torch.int64, device=x.device)
            expert_tokens.scatter_add_(0, idx.reshape(-1), torch.ones_like(idx.reshape(-1)))
        if T:
            f = expert_tokens.detach().to(torch.float32) / float(T * self.top_k)
            self.aux_loss = self.num_experts * (f * (prob_sum / float(T))).sum()
        else:
            self.aux_loss = prob_sum.sum() * 0.0
        recv_x, h = moe_dispatch(self.group, x, idx, self.num_experts, self.capacity,
                                 expert_capacity=self.expert_capacity)
        self.last_handle = h
        y = self.experts(recv_x, h.expert_counts)
        return moe_combine(self.group, y, h, w)
