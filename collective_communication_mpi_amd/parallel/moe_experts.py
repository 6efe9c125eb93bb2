"""The expert block of a routed MoE layer: what runs between ``moe_dispatch`` and
``moe_combine`` on the rows a rank received, grouped by local expert.

Everything is shaped by host-known values (the buffer's capacity, the number of local
experts); the rows per expert are read on the device from ``expert_counts``, so the block
makes no host synchronisation in either direction and can be captured in a graph together
with the dispatch and the combine around it."""
from __future__ import annotations

import math

import torch

from ..ops import (
    grouped_dx,
    grouped_gemm_nt_swiglu,
    grouped_gemm_tn,
    grouped_grad_rows,
    grouped_linear,
    grouped_swiglu_route,
    swiglu_pairs,
    swiglu_pairs_backward,
)


class _SwiGLUPairs(torch.autograd.Function):
    """``silu(h[:, 0::2]) * h[:, 1::2]`` over the whole buffer (one HIP kernel each way)."""

    @staticmethod
    def forward(ctx, h):
        ctx.save_for_backward(h)
        return swiglu_pairs(h)

    @staticmethod
    def backward(ctx, da):
        (h,) = ctx.saved_tensors
        return swiglu_pairs_backward(h, da)


class _GroupedGateUp(torch.autograd.Function):
    """``swiglu_pairs(grouped_gemm_nt(x, w, counts))`` with the gate applied in the GEMM's
    epilogue (``grouped_gemm_nt_swiglu``).  Backward: the SwiGLU backward kernel on the saved
    ``h``, then dX (``grouped_dx``) and dW (``grouped_gemm_tn``) as ``grouped_linear`` has them."""

    @staticmethod
    def forward(ctx, x, w, counts):
        wb = w if w.dtype == torch.bfloat16 else w.to(torch.bfloat16)
        h, glu = grouped_gemm_nt_swiglu(x, wb, counts)
        ctx.save_for_backward(x, wb, counts, h)
        ctx.w_dtype = w.dtype
        return glu

    @staticmethod
    def backward(ctx, da):
        x, wb, counts, h = ctx.saved_tensors
        dh = grouped_grad_rows(swiglu_pairs_backward(h, da))
        # dW before dX: h and da stay alive until this node returns, and the peak of the backward
        # is the fp32 dW next to its cast; dx is allocated once the fp32 copy is gone
        dx = dw = None
        if ctx.needs_input_grad[1]:
            dw = grouped_gemm_tn(dh, x, counts).to(ctx.w_dtype)
        if ctx.needs_input_grad[0]:
            dx = grouped_dx(dh, wb, counts, x.dtype)
        return dx, dw, None


class GroupedExpertsMLP(torch.nn.Module):
    """SwiGLU MLPs of the ``num_local_experts`` experts of this rank over the rows of
    ``moe_dispatch``'s receive buffer:

        y[r] = down[g] . swiglu(gate_up[g] . x[r])        for the rows r of local expert g

    ``gate_up`` is ``[G, 2 * d_ff, d_model]`` with the gate and up rows of a hidden unit
    interleaved (row 2j = gate j, row 2j + 1 = up j: the order ``swiglu_pairs`` expects);
    ``down`` is ``[G, d_model, d_ff]``.  ``forward(recv_x, expert_counts)`` runs the grouped
    gate|up GEMM with the SwiGLU gate in its epilogue (``grouped_gemm_nt_swiglu``, the rows of
    the experts only) and the grouped down GEMM; it is differentiable through the SwiGLU
    backward kernel, ``grouped_gemm_nn`` (dX) and ``grouped_gemm_tn`` (dW).
    ``CCMPI_GROUPED_SWIGLU=unfused`` (read at call time) keeps the three-step form, the gate as
    its own kernel over the whole buffer; ``CCMPI_GROUPED_DX=transpose`` the dX on a transposed
    copy of the weights (both for A/B runs).  Rows at or
    past ``sum(expert_counts)`` of the result (and of the gradient for ``recv_x``) are
    unspecified; ``moe_combine`` never reads them."""

    def __init__(self, num_local_experts: int, d_model: int, d_ff: int, device=None, dtype=torch.bfloat16):
        super().__init__()
        if num_local_experts < 1 or num_local_experts > 256:
            raise ValueError("GroupedExpertsMLP: num_local_experts must be in [1, 256]")
        if d_model % 8 or d_ff % 8 or d_model < 8 or d_ff < 8:
            raise ValueError("GroupedExpertsMLP: d_model and d_ff must be positive multiples of 8")
        if dtype not in (torch.bfloat16, torch.float32):
            raise TypeError("GroupedExpertsMLP weights are bf16, or fp32 master weights")
        self.num_local_experts, self.d_model, self.d_ff = num_local_experts, d_model, d_ff
        self.gate_up = torch.nn.Parameter(torch.empty(num_local_experts, 2 * d_ff, d_model, device=device, dtype=dtype))
        self.down = torch.nn.Parameter(torch.empty(num_local_experts, d_model, d_ff, device=device, dtype=dtype))
        self.reset_parameters()

    def reset_parameters(self) -> None:
        with torch.no_grad():
            self.gate_up.copy_(torch.randn(self.gate_up.shape, device=self.gate_up.device) / math.sqrt(self.d_model))
            self.down.copy_(torch.randn(self.down.shape, device=self.down.device) / math.sqrt(self.d_ff))

    def forward(self, recv_x: torch.Tensor, expert_counts: torch.Tensor) -> torch.Tensor:
        if grouped_swiglu_route() == "fused":
            if self.gate_up.dtype not in (torch.bfloat16, torch.float32):
                raise TypeError("GroupedExpertsMLP weights must be bf16 or fp32")
            a = _GroupedGateUp.apply(recv_x, self.gate_up, expert_counts)  # [cap, d_ff]
        else:
            h = grouped_linear(recv_x, self.gate_up, expert_counts)   # [cap, 2 d_ff], (gate, up) interleaved
            a = _SwiGLUPairs.apply(h)                                 # [cap, d_ff]
        return grouped_linear(a, self.down, expert_counts)        # [cap, d_model]
