"""Device ops backed by the hand-written HIP kernels of ``_device`` (gfx950).

Every op fails loudly (raises) when the extension is missing or an input
violates a kernel precondition; there is no silent eager fallback."""
from .kernels import (  # noqa: F401
    gemm_nt,
    gemm_tn,
    gemm_ring,
    linear,
    swiglu,
    swiglu_pairs,
    swiglu_pairs_backward,
    gemm_nt_swiglu,
    transpose,
    interleave_lastaxis,
    deinterleave_lastaxis,
    grouped_gemm_nt,
    grouped_gemm_tn,
    grouped_gemm_nn,
    grouped_gemm_nt_swiglu,
    grouped_nn_validate,
    grouped_dx,
    grouped_dx_route,
    grouped_grad_rows,
    grouped_swiglu_route,
    grouped_linear,
    grouped_validate,
    grouped_tile_map,
    moe_gate,
    moe_gate_forward,
    moe_gate_backward,
    moe_gate_validate,
)
