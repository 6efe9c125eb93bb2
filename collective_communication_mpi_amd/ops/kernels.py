"""Python entry points of the device kernels (csrc/device/*.hip)."""
from __future__ import annotations

import os
from typing import Optional

import torch

from .. import _native

_ACT = {None: 0, "none": 0, "relu": 1, "gelu": 2}


def _D():
    return _native.device()


def _stream(t: torch.Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream


_TN_VARIANT = None  # tests / benchmarks: force the TN kernel (0 = 128x128, 1 = 256x256 ping-pong)


def set_tn_variant(v):
    global _TN_VARIANT
    _TN_VARIANT = v


def _auto_splitk(tiles: int, K: int) -> int:
    """Split K until the grid has ~2 workgroups per CU, keeping >= 4 K-tiles per split."""
    nk = (K + 63) // 64
    want = max(1, 512 // max(tiles, 1))
    return int(max(1, min(want, nk // 4, 32)))


def gemm_nt(a: torch.Tensor, b: torch.Tensor, out: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None,
            alpha: float = 1.0, accumulate: bool = False, act: Optional[str] = None,
            out_dtype: torch.dtype = torch.bfloat16, splitk: Optional[int] = None) -> torch.Tensor:
    """``out = act(alpha * a @ b.T + bias) (+ out)`` on MFMA (v_mfma_f32_16x16x32_bf16).

    a: [M, K] bf16 row-major (row stride may exceed K), b: [N, K] bf16; K % 8 == 0.
    bias: [N] fp32 or bf16.  out: [M, N] bf16 or fp32 (fp32 accumulate inside).

    a and b may be views of larger buffers (column windows, row slices) as long as they start
    16-B aligned and their row strides are multiples of 8 elements; anything else raises
    ValueError.  What lies around them never reaches a result.  ``out`` may be any view with
    unit column stride: a misaligned start, an odd row stride or N % 8 != 0 take the
    per-element stores, and nothing outside ``[M, N]`` is written.  A bf16 output is one
    round-to-nearest-even of the fp32 result (of result + previous contents with
    ``accumulate``).  ``splitk`` > 1 needs an fp32 output and no activation (ValueError).
    """
    if a.dtype != torch.bfloat16 or b.dtype != torch.bfloat16:
        raise TypeError("gemm_nt expects bf16 operands")
    if a.dim() != 2 or b.dim() != 2 or a.shape[1] != b.shape[1]:
        raise ValueError(f"gemm_nt shape mismatch: {tuple(a.shape)} x {tuple(b.shape)}^T")
    if a.stride(1) != 1 or b.stride(1) != 1:
        raise ValueError("gemm_nt operands must be K-contiguous")
    M, K = a.shape
    N = b.shape[0]
    if out is None:
        if accumulate:
            raise ValueError("accumulate needs an output tensor")
        out = torch.empty((M, N), dtype=out_dtype, device=a.device)
    if out.stride(1) != 1 or out.shape != (M, N):
        raise ValueError("gemm_nt output must be [M, N] with unit column stride")
    if out.dtype not in (torch.bfloat16, torch.float32):
        raise TypeError("gemm_nt output must be bf16 or fp32")
    bias_kind = 0
    bias_ptr = 0
    if bias is not None:
        bias_kind = 1 if bias.dtype == torch.float32 else 2
        if bias.dtype not in (torch.float32, torch.bfloat16) or not bias.is_contiguous() or bias.numel() != N:
            raise ValueError("bias must be a contiguous [N] fp32/bf16 tensor")
        bias_ptr = bias.data_ptr()
    if splitk is None:
        fp32_plain = out.dtype == torch.float32 and act is None
        splitk = _auto_splitk(((M + 127) // 128) * ((N + 127) // 128), K) if fp32_plain else 1
    _D().gemm_nt(a.data_ptr(), b.data_ptr(), out.data_ptr(), bias_ptr, M, N, K, a.stride(0), b.stride(0),
                 out.stride(0), float(alpha), bool(accumulate), bias_kind, _ACT[act], out.dtype == torch.bfloat16,
                 int(splitk), _stream(a))
    return out


def gemm_tn(a: torch.Tensor, b: torch.Tensor, out: Optional[torch.Tensor] = None, alpha: float = 1.0,
            accumulate: bool = False, splitk: Optional[int] = None, tail: Optional[torch.Tensor] = None,
            workspace: Optional[bool] = None) -> torch.Tensor:
    """``out[N1, N2] (+)= alpha * a[M, N1].T @ b[M, N2]`` (weight gradients dW = dY^T X) in fp32,
    reading both operands M-major through ds_read_b64_tr_b16 (no transposes).

    ``tail``: split the result by columns -- ``out`` (``[N1, c]``, accumulated if
    ``accumulate``) receives columns ``< c`` and ``tail`` (``[N1, N2 - c]``,
    overwritten) the rest, straight from the split-K reduction (one GEMM over a
    row-concatenated operand ``b = [X | Y]`` gives ``a^T X`` and ``a^T Y``).

    Both outputs need 16-B aligned rows then (start and row stride): only the reduction
    pass splits the columns, and it writes 16-B vectors.

    ``workspace``: split-K partials through a workspace + one reduction pass (True)
    or fp32 atomics into ``out`` (False); default by output size.

    a, b: bf16 with unit column stride, 16-B aligned start and rows (row strides may exceed
    N1 / N2: column windows and row slices of larger buffers are fine), N1 % 8 == N2 % 8 == 0;
    M is free, rows at and past M are never read into a result.  Without ``tail``, ``out``
    may be any fp32 view with unit column stride (a misaligned start or an odd row stride
    takes the per-element epilogue); nothing outside ``[N1, N2]`` is written."""
    if a.dtype != torch.bfloat16 or b.dtype != torch.bfloat16:
        raise TypeError("gemm_tn expects bf16 operands")
    if a.dim() != 2 or b.dim() != 2 or a.shape[0] != b.shape[0] or a.stride(1) != 1 or b.stride(1) != 1:
        raise ValueError(f"gemm_tn shape mismatch: {tuple(a.shape)}^T x {tuple(b.shape)}")
    M, N1 = a.shape
    N2 = b.shape[1]
    csplit = 0
    if tail is not None:
        if out is None:
            raise ValueError("gemm_tn: tail needs an explicit out")
        csplit = out.shape[1]
        if (tail.dtype != torch.float32 or tail.shape != (N1, N2 - csplit) or tail.stride(1) != 1
                or csplit % 4 or tail.stride(0) % 4 or tail.data_ptr() % 16):
            raise ValueError("gemm_tn tail must be fp32 [N1, N2 - out cols], 16-B aligned rows, out cols % 4 == 0")
        if out.dtype != torch.float32 or out.shape[0] != N1 or out.stride(1) != 1:
            raise ValueError("gemm_tn output must be fp32 [N1, c] with unit column stride")
        if out.stride(0) % 4 or out.data_ptr() % 16:
            raise ValueError("gemm_tn: with a tail, out needs 16-B aligned rows too (the split-K reduction "
                             "writes both as 16-B vectors)")
    elif out is None:
        if accumulate:
            raise ValueError("accumulate needs an output tensor")
        out = torch.empty((N1, N2), dtype=torch.float32, device=a.device)
    if tail is None and (out.dtype != torch.float32 or out.shape != (N1, N2) or out.stride(1) != 1):
        raise ValueError("gemm_tn output must be fp32 [N1, N2] with unit column stride")
    # variant 1 (256x256 ping-pong TN) is opt-in: measured slower than the 128x128 TN kernel on
    # every shape tried (benchmarks/gemm_tn_splitk.py, profiles/r1_gemm_fastepi/tn_variants.txt)
    variant = _TN_VARIANT if _TN_VARIANT is not None else 0
    if variant == 1 and not (M % 128 == 0 and N1 >= 256 and N2 >= 256):
        variant = 0
    if splitk is None:
        if variant == 1:  # 256x256 tiles: split K until ~1 workgroup per CU, >= 2 K-tile pairs per split
            tiles = ((N1 + 255) // 256) * ((N2 + 255) // 256)
            splitk = int(max(1, min(256 // max(tiles, 1), M // 256, 64)))
        else:
            splitk = _auto_splitk(((N1 + 127) // 128) * ((N2 + 127) // 128), M)
    if tail is not None:
        splitk = max(2, splitk)  # the column split happens in the split-K reduction
    ws = 0
    # large outputs: partials in a workspace + one reduction pass instead of fp32 atomics
    # (dW_qkv 768x768: 80 -> 68 us); small outputs keep the atomics (one launch fewer)
    use_ws = workspace if workspace is not None else (variant == 1 or N1 * N2 >= (1 << 18) or tail is not None)
    if splitk > 1 and N2 % 4 == 0 and (use_ws or tail is not None):
        ws = torch.empty(splitk * N1 * N2, dtype=torch.float32, device=a.device).data_ptr()
    _D().gemm_tn(a.data_ptr(), b.data_ptr(), out.data_ptr(), M, N1, N2, a.stride(0), b.stride(0), out.stride(0),
                 float(alpha), bool(accumulate), int(splitk), _stream(a), ws, int(variant),
                 0 if tail is None else tail.data_ptr(), 0 if tail is None else tail.stride(0), csplit)
    return out


def linear(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, act: Optional[str] = None,
           out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``x[..., K] @ w[N, K].T + bias`` with the MFMA GEMM (bf16 out)."""
    lead = x.shape[:-1]
    y = gemm_nt(x.reshape(-1, x.shape[-1]), w, out=None if out is None else out.reshape(-1, w.shape[0]),
                bias=bias, act=act)
    return y.reshape(*lead, w.shape[0])


def gemm_ring(a: torch.Tensor, b: torch.Tensor, ta: bool, tb: bool, out: Optional[torch.Tensor] = None,
              alpha: float = 1.0, accumulate: bool = False, out_dtype: torch.dtype = torch.bfloat16,
              a_nt: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
    """``out = alpha * op(a) @ op(b).T (+ out)`` on the four-wave LDS-ring MFMA kernel
    (csrc/device/gemm_w4.hip), with either operand K-major: op(a) = a.T if ``ta`` (a is
    [K, M]) else a ([M, K]); op(b) = b.T if ``tb`` (b is [K, N]) else b ([N, K]).
    dX = dY W is ``gemm_ring(dY, W, False, True)``, dW = dY^T X is
    ``gemm_ring(dY, X, True, True)``: no transposes.  Returns None when the kernel does
    not apply (K % 64, 16-B alignment, > 2 GiB operands): the caller falls back.
    ``a_nt``: op(a) already in N layout (``a.T`` contiguous, e.g. the dh^T the SwiGLU
    backward writes): the N-layout pair ring runs on it, no transpose of ``a``."""
    if a.dtype != torch.bfloat16 or b.dtype != torch.bfloat16 or a.dim() != 2 or b.dim() != 2:
        raise TypeError("gemm_ring expects 2-D bf16 operands")
    if a.stride(1) != 1 or b.stride(1) != 1:
        raise ValueError("gemm_ring operands must have unit inner stride")
    M, K = (a.shape[1], a.shape[0]) if ta else (a.shape[0], a.shape[1])
    N, Kb = (b.shape[1], b.shape[0]) if tb else (b.shape[0], b.shape[1])
    if K != Kb:
        raise ValueError(f"gemm_ring shape mismatch: op(a) {M}x{K}, op(b) {N}x{Kb}")
    if out is None:
        if accumulate:
            raise ValueError("accumulate needs an output tensor")
        out = torch.empty((M, N), dtype=out_dtype, device=a.device)
    if out.shape != (M, N) or out.stride(1) != 1 or out.dtype not in (torch.bfloat16, torch.float32):
        raise ValueError("gemm_ring output must be [M, N] bf16/fp32 with unit column stride")
    route = os.environ.get("CCMPI_KMAJOR_ROUTE", "pair")
    if ta and route == "pair":
        # dW = dY^T X with both operands M-major on the pair-slot ring's TA (+ TB) form: no
        # transposes at all (an N-layout copy the producer wrote is not needed either).
        # Llama-3-8B MLP at T = 4096: dW_down 0.369 ms against 0.464 ms for both operands
        # transposed, the whole block forward + backward 3.334 ms against 3.395 ms
        # (profiles/r5_fourth).  CCMPI_KMAJOR_ROUTE=transpose: the round-4 route
        ok = _D().gemm_ring(a.data_ptr(), b.data_ptr(), out.data_ptr(), M, N, K, a.stride(0), b.stride(0),
                            out.stride(0), 1, int(tb), float(alpha), bool(accumulate), out.dtype == torch.bfloat16,
                            _stream(a))
        if ok:
            return out
    if ta and (a_nt is not None or _kmajor_via_transpose(M, N, K, a, b)):
        # K-major A transposed first (k_transpose16_v, ~6 TB/s) -- or taken from a_nt, the
        # N-layout copy its producer wrote -- then the pair-slot ring: its whole-line DMA
        # pieces and one ds_read_b128 per fragment beat the 4-slot K-major ring's two
        # transposed LDS reads per fragment (profiles/r4_bwd).  A K-major B stays K-major:
        # the pair ring reads it directly (its dX = dY W form), so dW = dY^T X transposes
        # at most dY (CCMPI_WGRAD_B=transpose: the old route, both operands transposed)
        at = a_nt if a_nt is not None else transpose(a)
        if tb and os.environ.get("CCMPI_WGRAD_B", "kmajor") == "kmajor":
            return gemm_ring(at, b, False, True, out=out, alpha=alpha, accumulate=accumulate, out_dtype=out_dtype)
        bt = transpose(b) if tb else b
        return gemm_ring(at, bt, False, False, out=out, alpha=alpha, accumulate=accumulate, out_dtype=out_dtype)
    ok = _D().gemm_ring(a.data_ptr(), b.data_ptr(), out.data_ptr(), M, N, K, a.stride(0), b.stride(0), out.stride(0),
                        int(ta), int(tb), float(alpha), bool(accumulate), out.dtype == torch.bfloat16, _stream(a))
    return out if ok else None


def _kmajor_via_transpose(M: int, N: int, K: int, a: torch.Tensor, b: torch.Tensor) -> bool:
    """Route a K-major ring GEMM through transposed copies (CCMPI_KMAJOR_ROUTE=transpose,
    read per call; default ``pair``: the pair ring reads K-major operands itself; ``ring``: the
    4-slot K-major kernel): K-major A (the dW = dY^T X form), large GEMMs only, and not long
    K.  dX = dY W (K-major B only) stays on the ring: a transposed weight copy + the pair ring
    measured no faster (profiles/r4_bwd)."""
    if os.environ.get("CCMPI_KMAJOR_ROUTE", "pair") != "transpose":
        return False
    dmin = int(os.environ.get("CCMPI_KMAJOR_MIN_DIM", 1024))  # (tests lower both thresholds)
    return (M >= dmin and N >= dmin and K <= 16384 and K % 8 == 0 and M % 8 == 0 and N % 8 == 0
            and M * N * K >= int(os.environ.get("CCMPI_KMAJOR_MIN_MACS", 1 << 33))
            and a.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 0
            and a.stride(0) % 8 == 0 and b.stride(0) % 8 == 0)


def transpose(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """2-D transpose of a 16-bit tensor: 16-B register-transpose kernel when the shape and
    strides are multiples of 8 elements (k_transpose16_v), else the LDS-tiled one."""
    if x.dim() != 2 or x.element_size() != 2 or x.stride(1) != 1:
        raise ValueError("transpose expects a 2-D row-contiguous 16-bit tensor")
    R, C = x.shape
    if out is None:
        out = torch.empty((C, R), dtype=x.dtype, device=x.device)
    _D().transpose16(x.data_ptr(), out.data_ptr(), R, C, x.stride(0), out.stride(0), _stream(x))
    return out


def _swiglu_rows(t: torch.Tensor) -> torch.Tensor:
    """2-D view ``[rows, cols]`` with unit column stride (copies only if it must)."""
    t2 = t.reshape(-1, t.shape[-1])
    ok = t2.stride(1) == 1 and t2.stride(0) % 8 == 0 and t2.data_ptr() % 16 == 0
    return t2 if ok else t2.contiguous()


class _SwiGLU(torch.autograd.Function):
    """``silu(h[..., :k]) * h[..., k:]`` in one HIP kernel each way (csrc/device/swiglu.hip);
    saves only ``h`` (the gate|up GEMM output), backward writes ``dh`` in one pass."""

    @staticmethod
    def forward(ctx, h):
        h2 = _swiglu_rows(h)
        k = h2.shape[1] // 2
        a = torch.empty(*h.shape[:-1], k, dtype=h.dtype, device=h.device)
        _D().swiglu_fwd(h2.data_ptr(), a.data_ptr(), h2.shape[0], k, h2.stride(0), k, _stream(h2))
        ctx.save_for_backward(h2)
        ctx.lead = h.shape[:-1]
        return a

    @staticmethod
    def backward(ctx, da):
        (h2,) = ctx.saved_tensors
        k = h2.shape[1] // 2
        da2 = _swiglu_rows(da)
        dh = torch.empty(*ctx.lead, 2 * k, dtype=h2.dtype, device=h2.device)
        _D().swiglu_bwd(h2.data_ptr(), da2.data_ptr(), dh.data_ptr(), h2.shape[0], k, h2.stride(0), da2.stride(0),
                        2 * k, _stream(h2))
        return dh


def swiglu(h: torch.Tensor) -> torch.Tensor:
    """SwiGLU gate of a ``[..., 2k]`` gate|up tensor: ``silu(h[..., :k]) * h[..., k:]``.

    CUDA bf16 with ``k % 8 == 0`` runs the fused HIP kernels (fp32 math, one bf16
    rounding); anything else (CPU, other dtypes) is computed by torch ops."""
    if h.shape[-1] % 2:
        raise ValueError("swiglu needs an even last dimension (gate | up)")
    k = h.shape[-1] // 2
    if h.is_cuda and h.dtype == torch.bfloat16 and k % 8 == 0 and h.data_ptr() % 16 == 0:
        return _SwiGLU.apply(h)
    return torch.nn.functional.silu(h[..., :k]) * h[..., k:]


def swiglu_pairs(h: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """SwiGLU gate of interleaved (gate, up) pairs: ``silu(h[:, 0::2]) * h[:, 1::2]``
    (``h`` [T, 2k] bf16 CUDA, row-contiguous; one HIP kernel, no autograd)."""
    T, n = h.shape
    if out is None:
        out = torch.empty((T, n // 2), dtype=h.dtype, device=h.device)
    _D().swiglu_fwd_il(h.data_ptr(), out.data_ptr(), T, n // 2, h.stride(0), out.stride(0), _stream(h))
    return out


def swiglu_pairs_backward(h: torch.Tensor, da: torch.Tensor, transposed: bool = False):
    """Gradient of ``swiglu_pairs`` w.r.t. its interleaved input (one HIP kernel).  With
    ``transposed`` (T % 8 == 0): returns ``(dh, dh^T)``, the transposed copy written by the
    same kernel (the weight-gradient GEMM's N-layout operand, no separate transpose)."""
    T, n = h.shape
    da = da if (da.stride(1) == 1 and da.stride(0) % 4 == 0) else da.contiguous()
    dh = torch.empty_like(h)
    if transposed:
        dht = torch.empty(n, T, device=h.device, dtype=h.dtype)
        _D().swiglu_bwd_il_t(h.data_ptr(), da.data_ptr(), dh.data_ptr(), dht.data_ptr(), T, n // 2, h.stride(0),
                             da.stride(0), dh.stride(0), dht.stride(0), _stream(h))
        return dh, dht
    _D().swiglu_bwd_il(h.data_ptr(), da.data_ptr(), dh.data_ptr(), T, n // 2, h.stride(0), da.stride(0),
                       dh.stride(0), _stream(h))
    return dh


def gemm_nt_swiglu(a: torch.Tensor, b: torch.Tensor, h: torch.Tensor, glu: torch.Tensor) -> bool:
    """``h = a @ b.T`` (bf16) with the SwiGLU gate of h's interleaved column pairs written
    to ``glu`` by the GEMM's own epilogue (LDS-ring kernel, csrc/device/gemm_w4.hip EPI 2).
    Returns False (nothing launched) when the ring kernel's fast form does not apply."""
    M, K = a.shape
    N = b.shape[0]
    if not (a.stride(1) == 1 and b.stride(1) == 1 and h.shape == (M, N) and h.stride(1) == 1
            and glu.shape == (M, N // 2) and glu.stride(1) == 1):
        return False
    return bool(_D().gemm_nt_swiglu(a.data_ptr(), b.data_ptr(), h.data_ptr(), glu.data_ptr(), M, N, K, a.stride(0),
                                    b.stride(0), h.stride(0), glu.stride(0), _stream(a)))


def interleave_lastaxis(stage: torch.Tensor, p: int) -> torch.Tensor:
    """``[p, *lead, k] -> [*lead, p*k]`` (np.concatenate(parts, axis=-1))."""
    stage = stage.contiguous()
    lead, k = stage.shape[1:-1], stage.shape[-1]
    M = stage[0].numel() // max(k, 1)
    out = torch.empty(*lead, p * k, dtype=stage.dtype, device=stage.device)
    _D().interleave_lastaxis(stage.data_ptr(), out.data_ptr(), M, p, k * stage.element_size(), _stream(stage))
    return out


def deinterleave_lastaxis(x: torch.Tensor, p: int) -> torch.Tensor:
    """``[*lead, p*k] -> [p, *lead, k]`` (np.stack(np.split(x, p, axis=-1)))."""
    x = x.contiguous()
    n = x.shape[-1]
    if n % p:
        raise ValueError("last axis not divisible by p")
    k = n // p
    M = x.numel() // max(n, 1)
    out = torch.empty(p, *x.shape[:-1], k, dtype=x.dtype, device=x.device)
    _D().deinterleave_lastaxis(x.data_ptr(), out.data_ptr(), M, p, k * x.element_size(), _stream(x))
    return out


# ---------------------------------------------------------------------------
# grouped expert GEMM over routed MoE rows (csrc/device/grouped_gemm.hip)
# ---------------------------------------------------------------------------
GROUPED_MAX_EXPERTS = 256  # = device.MOE_MAX_EXPERTS: one count per thread of the kernel's scan
GROUPED_BM = 128           # rows per tile


def grouped_tile_map(counts, cap: int, bm: int = GROUPED_BM):
    """Host mirror of the grouped kernels' tile walk: the ``(expert, first_row, rows)`` of
    every row tile, in the order the kernel numbers them.  Expert g owns rows
    ``[off_g, off_g + c_g)`` with ``c_g = max(counts[g], 0)`` and ``off_g`` their prefix sum,
    both ends clamped to ``cap``; its tiles start at ``off_g`` (so no tile spans two experts)
    and the last one is short.  There are at most ``ceil(cap / bm) + len(counts)`` tiles,
    which is the row-tile count the forward kernel's grid is sized for."""
    cap, bm = int(cap), int(bm)
    if bm < 1:
        raise ValueError("grouped_tile_map: bm must be positive")
    tiles = []
    at = 0
    for g, c in enumerate(counts):
        off = min(at, cap)
        at += min(max(int(c), 0), max(cap, 0))
        end = min(at, cap)
        for r0 in range(off, end, bm):
            tiles.append((g, r0, min(bm, end - r0)))
    return tiles


def grouped_validate(x, w, counts, out=None, bias=None, out_dtype=torch.bfloat16):
    """Argument rules of ``grouped_gemm_nt`` that need no GPU; raises TypeError (dtypes) /
    ValueError (shapes, strides, bounds) like ``gemm_nt`` and returns ``(cap, G, N, K)``.
    ``w`` is ``[G, N, K]`` with unit inner stride; its other two strides are free (multiples
    of 8 elements), so the ``[G, K, N]`` view of one transposed ``[K, G * N]`` copy is accepted."""
    if x.dtype != torch.bfloat16 or w.dtype != torch.bfloat16:
        raise TypeError("grouped GEMM expects bf16 operands")
    if x.dim() != 2 or w.dim() != 3 or x.shape[1] != w.shape[2]:
        raise ValueError(f"grouped GEMM shape mismatch: x {tuple(x.shape)}, w {tuple(w.shape)} (want [cap, K], [G, N, K])")
    cap, K = x.shape
    G, N = w.shape[0], w.shape[1]
    if G < 1 or G > GROUPED_MAX_EXPERTS:
        raise ValueError(f"grouped GEMM: the number of experts must be in [1, {GROUPED_MAX_EXPERTS}], got {G}")
    if K < 8 or N < 8 or K % 8 or N % 8:
        raise ValueError(f"grouped GEMM: K ({K}) and N ({N}) must be positive multiples of 8")
    if x.stride(1) != 1 or w.stride(2) != 1:
        raise ValueError("grouped GEMM operands must have unit inner stride")
    if (cap > 1 and x.stride(0) % 8) or (N > 1 and w.stride(1) % 8) or (G > 1 and w.stride(0) % 8):
        raise ValueError("grouped GEMM: row and expert strides must be multiples of 8 elements (16 bytes)")
    if x.data_ptr() % 16 or w.data_ptr() % 16:
        raise ValueError("grouped GEMM: operands must be 16-B aligned")
    if counts.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"grouped GEMM: counts must be int32 or int64, got {counts.dtype}")
    if counts.dim() != 1 or counts.shape[0] != G or not counts.is_contiguous():
        raise ValueError(f"grouped GEMM: counts must be a contiguous [{G}] tensor, got {tuple(counts.shape)}")
    if counts.device != x.device or w.device != x.device:
        raise ValueError("grouped GEMM: x, w and counts must be on the same device")
    if out is not None:
        if out.dtype not in (torch.bfloat16, torch.float32):
            raise TypeError("grouped GEMM output must be bf16 or fp32")
        if out.shape != (cap, N) or out.stride(1) != 1 or out.device != x.device:
            raise ValueError("grouped GEMM output must be [cap, N] with unit column stride on x's device")
        if out.data_ptr() % 16 or (cap > 1 and (out.stride(0) * out.element_size()) % 16):
            raise ValueError("grouped GEMM output rows must be 16-B aligned")
    elif out_dtype not in (torch.bfloat16, torch.float32):
        raise TypeError("grouped GEMM output must be bf16 or fp32")
    if bias is not None:
        if bias.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError("grouped GEMM bias must be fp32 or bf16")
        if bias.shape != (G, N) or not bias.is_contiguous() or bias.device != x.device:
            raise ValueError("grouped GEMM bias must be a contiguous [G, N] tensor on x's device")
    return int(cap), int(G), int(N), int(K)


def grouped_gemm_nt(x: torch.Tensor, w: torch.Tensor, counts: torch.Tensor, out: Optional[torch.Tensor] = None,
                    bias: Optional[torch.Tensor] = None, alpha: float = 1.0,
                    out_dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    """``out[r] = alpha * x[r] @ w[g].T (+ bias[g])`` for every row r of expert g, the rows
    per expert read from the device tensor ``counts`` (``moe_dispatch``'s ``expert_counts``):
    no host synchronisation, a grid that does not depend on the counts, capturable in a graph.

    x: [cap, K] bf16 (row stride free), w: [G, N, K] bf16, counts: [G] int32 / int64 on the
    device, bias: [G, N] fp32 / bf16, out: [cap, N] bf16 or fp32.  Expert g owns rows
    ``[off_g, off_g + c_g)``, ``c_g = max(counts[g], 0)``, ``off_g`` their prefix sum; the
    ranges are clamped to cap (counts adding up to more truncate the last experts).  Rows at
    or past ``sum(c_g)`` are left untouched: with ``out=None`` they are uninitialised."""
    cap, G, N, K = grouped_validate(x, w, counts, out, bias, out_dtype)
    if out is None:
        out = torch.empty((cap, N), dtype=out_dtype, device=x.device)
    bias_kind = 0 if bias is None else (1 if bias.dtype == torch.float32 else 2)
    _D().grouped_gemm_nt(x.data_ptr(), w.data_ptr(), out.data_ptr(), 0 if bias is None else bias.data_ptr(),
                         counts.data_ptr(), cap, N, K, G, x.stride(0) if cap > 1 else K, w.stride(1), w.stride(0),
                         out.stride(0) if cap > 1 else N, N, float(alpha), bias_kind, out.dtype == torch.bfloat16,
                         counts.dtype == torch.int64, _stream(x))
    return out


def grouped_tn_validate(dy, x, counts, out=None):
    """Argument rules of ``grouped_gemm_tn`` that need no GPU; raises TypeError (dtypes) /
    ValueError (shapes, strides, alignment) and returns ``(cap, G, N, K)``.  ``dy`` [cap, N] and
    ``x`` [cap, K] follow the forward's operand rules (unit inner stride, 16-B aligned rows);
    ``out`` is fp32 ``[G, N, K]`` with unit inner stride, 16-B aligned rows and expert blocks."""
    if dy.dtype != torch.bfloat16 or x.dtype != torch.bfloat16:
        raise TypeError("grouped_gemm_tn expects bf16 operands")
    if dy.dim() != 2 or x.dim() != 2 or dy.shape[0] != x.shape[0] or dy.stride(1) != 1 or x.stride(1) != 1:
        raise ValueError(f"grouped_gemm_tn shape mismatch: {tuple(dy.shape)}^T x {tuple(x.shape)}")
    if counts.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"grouped_gemm_tn: counts must be int32 or int64, got {counts.dtype}")
    G = counts.numel()
    if counts.dim() != 1 or not counts.is_contiguous() or G < 1 or G > GROUPED_MAX_EXPERTS:
        raise ValueError(f"grouped_gemm_tn: counts must be a contiguous [G] tensor, 1 <= G <= {GROUPED_MAX_EXPERTS}")
    if counts.device != x.device or dy.device != x.device:
        raise ValueError("grouped_gemm_tn: dy, x and counts must be on the same device")
    cap, N = dy.shape
    K = x.shape[1]
    if N < 8 or K < 8 or N % 8 or K % 8:
        raise ValueError(f"grouped_gemm_tn: N ({N}) and K ({K}) must be positive multiples of 8")
    if cap > 1 and (dy.stride(0) % 8 or x.stride(0) % 8):
        raise ValueError("grouped_gemm_tn: row strides must be multiples of 8 elements (16 bytes)")
    if dy.data_ptr() % 16 or x.data_ptr() % 16:
        raise ValueError("grouped_gemm_tn: operands must be 16-B aligned")
    if out is not None:
        if out.dtype != torch.float32:
            raise TypeError("grouped_gemm_tn output must be fp32")
        if out.shape != (G, N, K) or out.stride(2) != 1 or out.device != x.device:
            raise ValueError("grouped_gemm_tn output must be fp32 [G, N, K] with unit inner stride on x's device")
        if out.data_ptr() % 16 or out.stride(1) % 4 or out.stride(0) % 4:
            raise ValueError("grouped_gemm_tn output rows and expert blocks must be 16-B aligned")
    return int(cap), int(G), int(N), int(K)


def grouped_gemm_tn(dy: torch.Tensor, x: torch.Tensor, counts: torch.Tensor, out: Optional[torch.Tensor] = None,
                    alpha: float = 1.0) -> torch.Tensor:
    """Weight gradients of ``grouped_gemm_nt``: ``out[g] = alpha * dy[rows of g].T @ x[rows of g]``,
    fp32 ``[G, N, K]`` (dy [cap, N], x [cap, K] bf16, same row rules).  Both operands are read
    row-major through ds_read_b64_tr_b16; rows outside an expert are masked at the load (they
    may hold anything, NaN included); an expert with no rows gets zeros.  One workgroup per
    (expert, 128 x 128 tile) walks the expert's rows in order: deterministic, no atomics."""
    cap, G, N, K = grouped_tn_validate(dy, x, counts, out)
    if out is None:
        out = torch.empty((G, N, K), dtype=torch.float32, device=x.device)
    _D().grouped_gemm_tn(dy.data_ptr(), x.data_ptr(), out.data_ptr(), counts.data_ptr(), cap, N, K, G,
                         dy.stride(0) if cap > 1 else N, x.stride(0) if cap > 1 else K, out.stride(1), out.stride(0),
                         float(alpha), counts.dtype == torch.int64, _stream(x))
    return out


def grouped_nn_validate(dy, w, counts, out=None, out_dtype=torch.bfloat16):
    """Argument rules of ``grouped_gemm_nn`` that need no GPU; raises TypeError (dtypes) /
    ValueError (shapes, strides, bounds) and returns ``(cap, G, N, K)``.  ``dy`` is
    ``[cap, N]`` and ``w`` is ``[G, N, K]`` exactly as ``grouped_gemm_nt`` takes it: unit inner
    strides, row and expert strides free multiples of 8 elements."""
    if dy.dtype != torch.bfloat16 or w.dtype != torch.bfloat16:
        raise TypeError("grouped_gemm_nn expects bf16 operands")
    if dy.dim() != 2 or w.dim() != 3 or dy.shape[1] != w.shape[1]:
        raise ValueError(f"grouped_gemm_nn shape mismatch: dy {tuple(dy.shape)}, w {tuple(w.shape)} "
                         "(want [cap, N], [G, N, K])")
    cap, N = dy.shape
    G, K = w.shape[0], w.shape[2]
    if G < 1 or G > GROUPED_MAX_EXPERTS:
        raise ValueError(f"grouped_gemm_nn: the number of experts must be in [1, {GROUPED_MAX_EXPERTS}], got {G}")
    if K < 8 or N < 8 or K % 8 or N % 8:
        raise ValueError(f"grouped_gemm_nn: N ({N}) and K ({K}) must be positive multiples of 8")
    if dy.stride(1) != 1 or w.stride(2) != 1:
        raise ValueError("grouped_gemm_nn operands must have unit inner stride")
    if (cap > 1 and dy.stride(0) % 8) or w.stride(1) % 8 or (G > 1 and w.stride(0) % 8):
        raise ValueError("grouped_gemm_nn: row and expert strides must be multiples of 8 elements (16 bytes)")
    if w.stride(1) < K:
        raise ValueError("grouped_gemm_nn: the rows of w must not overlap")
    if dy.data_ptr() % 16 or w.data_ptr() % 16:
        raise ValueError("grouped_gemm_nn: operands must be 16-B aligned")
    if counts.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"grouped_gemm_nn: counts must be int32 or int64, got {counts.dtype}")
    if counts.dim() != 1 or counts.shape[0] != G or not counts.is_contiguous():
        raise ValueError(f"grouped_gemm_nn: counts must be a contiguous [{G}] tensor, got {tuple(counts.shape)}")
    if counts.device != dy.device or w.device != dy.device:
        raise ValueError("grouped_gemm_nn: dy, w and counts must be on the same device")
    if out is not None:
        if out.dtype not in (torch.bfloat16, torch.float32):
            raise TypeError("grouped_gemm_nn output must be bf16 or fp32")
        if out.shape != (cap, K) or out.stride(1) != 1 or out.device != dy.device:
            raise ValueError("grouped_gemm_nn output must be [cap, K] with unit column stride on dy's device")
        if out.data_ptr() % 16 or (cap > 1 and (out.stride(0) * out.element_size()) % 16):
            raise ValueError("grouped_gemm_nn output rows must be 16-B aligned")
    elif out_dtype not in (torch.bfloat16, torch.float32):
        raise TypeError("grouped_gemm_nn output must be bf16 or fp32")
    return int(cap), int(G), int(N), int(K)


def grouped_gemm_nn(dy: torch.Tensor, w: torch.Tensor, counts: torch.Tensor, out: Optional[torch.Tensor] = None,
                    alpha: float = 1.0, out_dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    """Input gradient of ``grouped_gemm_nt``: ``out[r] = alpha * dy[r] @ w[g]`` for every row r
    of expert g, with ``w`` [G, N, K] read as the forward takes it (no transposed copy): the
    kernel stages 64 reduction rows x 128 columns of ``w[g]`` as they lie and reads its MFMA
    operand through ds_read_b64_tr_b16.

    dy: [cap, N] bf16 (row stride free), counts: [G] int32 / int64 on the device, out:
    [cap, K] bf16 or fp32.  The row rules are ``grouped_gemm_nt``'s: no host synchronisation,
    a grid sized from cap, G and K alone, rows at or past ``sum(c_g)`` left untouched.  The
    reduction stops at N exactly: what lies past column N of a strided ``dy`` or past row N of
    ``w[g]`` (the next expert, the end of the allocation) never reaches a result."""
    cap, G, N, K = grouped_nn_validate(dy, w, counts, out, out_dtype)
    if out is None:
        out = torch.empty((cap, K), dtype=out_dtype, device=dy.device)
    _D().grouped_gemm_nn(dy.data_ptr(), w.data_ptr(), out.data_ptr(), counts.data_ptr(), cap, N, K, G,
                         dy.stride(0) if cap > 1 else N, w.stride(1), w.stride(0), out.stride(0) if cap > 1 else K,
                         float(alpha), out.dtype == torch.bfloat16, counts.dtype == torch.int64, _stream(dy))
    return out


def grouped_swiglu_validate(x, w, counts, h=None, glu=None, bias=None):
    """Argument rules of ``grouped_gemm_nt_swiglu`` that need no GPU: ``grouped_validate``'s for
    ``x``, ``w``, ``counts``, ``bias`` and a bf16 ``h``, and for ``glu`` bf16 ``[cap, N / 2]`` with
    unit column stride, an 8-B aligned start and a row stride that is a multiple of 4 elements
    and at least ``N / 2``.  Returns ``(cap, G, N, K)``."""
    cap, G, N, K = grouped_validate(x, w, counts, h, bias, torch.bfloat16)
    if h is not None and h.dtype != torch.bfloat16:
        raise TypeError("grouped_gemm_nt_swiglu: h must be bf16")
    if glu is not None:
        if glu.dtype != torch.bfloat16:
            raise TypeError("grouped_gemm_nt_swiglu: glu must be bf16")
        if glu.shape != (cap, N // 2) or glu.stride(1) != 1 or glu.device != x.device:
            raise ValueError("grouped_gemm_nt_swiglu: glu must be [cap, N / 2] with unit column stride on x's device")
        if glu.data_ptr() % 8 or (cap > 1 and glu.stride(0) % 4):
            raise ValueError("grouped_gemm_nt_swiglu: glu rows must be 8-B aligned")
        if cap > 1 and glu.stride(0) < N // 2:
            raise ValueError("grouped_gemm_nt_swiglu: the rows of glu must not overlap (row stride >= N / 2)")
    return cap, G, N, K


def grouped_gemm_nt_swiglu(x: torch.Tensor, w: torch.Tensor, counts: torch.Tensor, h: Optional[torch.Tensor] = None,
                           glu: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None,
                           alpha: float = 1.0):
    """``grouped_gemm_nt`` of an interleaved gate|up weight with the SwiGLU gate in its
    epilogue: returns ``(h, glu)``, ``h`` [cap, N] bf16 exactly what ``grouped_gemm_nt(x, w,
    counts, bias=bias, alpha=alpha)`` writes and ``glu[r, j] = silu(h[r, 2j]) * h[r, 2j + 1]``
    ([cap, N / 2] bf16, bit for bit ``swiglu_pairs(h)``), written by the same kernel for the
    same rows.  Rows at or past ``sum(counts)`` of both outputs are left untouched."""
    cap, G, N, K = grouped_swiglu_validate(x, w, counts, h, glu, bias)
    if h is None:
        h = torch.empty((cap, N), dtype=torch.bfloat16, device=x.device)
    if glu is None:
        glu = torch.empty((cap, N // 2), dtype=torch.bfloat16, device=x.device)
    bias_kind = 0 if bias is None else (1 if bias.dtype == torch.float32 else 2)
    _D().grouped_gemm_nt_swiglu(x.data_ptr(), w.data_ptr(), h.data_ptr(), glu.data_ptr(),
                                0 if bias is None else bias.data_ptr(), counts.data_ptr(), cap, N, K, G,
                                x.stride(0) if cap > 1 else K, w.stride(1), w.stride(0),
                                h.stride(0) if cap > 1 else N, glu.stride(0) if cap > 1 else N // 2, N, float(alpha),
                                bias_kind, counts.dtype == torch.int64, _stream(x))
    return h, glu


def _transposed_experts(w: torch.Tensor) -> torch.Tensor:
    """``[G, K, N]`` view of one transposed copy of ``w`` [G, N, K]: the existing 2-D transpose
    kernel turns the [G * N, K] matrix into [K, G * N]; expert g's w[g].T is its column block
    g (row stride G * N), which ``grouped_gemm_nt`` reads through w's strides."""
    G, N, K = w.shape
    wt = transpose(w.contiguous().view(G * N, K))
    return wt.view(K, G, N).permute(1, 0, 2)


def grouped_dx_route() -> str:
    """How ``grouped_linear`` and ``GroupedExpertsMLP`` compute dX, read from the environment at
    call time: ``"nn"`` (default, ``grouped_gemm_nn`` on the weights as they lie) or
    ``"transpose"`` (``CCMPI_GROUPED_DX=transpose``: ``grouped_gemm_nt`` on a transposed copy
    of every expert's weights, kept for A/B runs)."""
    v = os.environ.get("CCMPI_GROUPED_DX", "nn")
    if v not in ("nn", "transpose"):
        raise ValueError(f"CCMPI_GROUPED_DX must be 'nn' or 'transpose', got {v!r}")
    return v


def grouped_swiglu_route() -> str:
    """How ``GroupedExpertsMLP`` applies the gate, read from the environment at call time:
    ``"fused"`` (default, ``grouped_gemm_nt_swiglu``) or ``"unfused"``
    (``CCMPI_GROUPED_SWIGLU=unfused``: ``grouped_linear``, ``swiglu_pairs``, ``grouped_linear``)."""
    v = os.environ.get("CCMPI_GROUPED_SWIGLU", "fused")
    if v not in ("fused", "unfused"):
        raise ValueError(f"CCMPI_GROUPED_SWIGLU must be 'fused' or 'unfused', got {v!r}")
    return v


def grouped_grad_rows(dy: torch.Tensor) -> torch.Tensor:
    """``dy`` as the grouped backward kernels read it (unit inner stride, 16-B aligned rows)."""
    ok = dy.stride(1) == 1 and (dy.shape[0] <= 1 or dy.stride(0) % 8 == 0) and dy.data_ptr() % 16 == 0
    return dy if ok else dy.contiguous()


def grouped_dx(dy: torch.Tensor, wb: torch.Tensor, counts: torch.Tensor, out_dtype: torch.dtype) -> torch.Tensor:
    """``dy . w[g]`` over the rows of every expert by the route ``grouped_dx_route`` names."""
    if grouped_dx_route() == "transpose":
        return grouped_gemm_nt(dy, _transposed_experts(wb), counts, out_dtype=out_dtype)
    return grouped_gemm_nn(dy, wb, counts, out_dtype=out_dtype)


class _GroupedLinear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, counts):
        wb = w if w.dtype == torch.bfloat16 else w.to(torch.bfloat16)
        ctx.save_for_backward(x, wb, counts)
        ctx.w_dtype = w.dtype
        return grouped_gemm_nt(x, wb, counts)

    @staticmethod
    def backward(ctx, dy):
        x, wb, counts = ctx.saved_tensors
        dy = grouped_grad_rows(dy)
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = grouped_dx(dy, wb, counts, x.dtype)
        if ctx.needs_input_grad[1]:
            dw = grouped_gemm_tn(dy, x, counts).to(ctx.w_dtype)
        return dx, dw, None


def grouped_linear(x: torch.Tensor, w: torch.Tensor, counts: torch.Tensor) -> torch.Tensor:
    """Differentiable ``grouped_gemm_nt(x, w, counts)`` (bf16 out).  ``w`` is bf16, or fp32
    master weights (rounded to bf16 for the kernels; their gradient then keeps the fp32 the
    weight-gradient kernel computes).  Backward: dX is ``grouped_gemm_nn`` on the weights as
    they lie (``CCMPI_GROUPED_DX=transpose``, read at call time, selects the earlier route: one
    ``transpose`` launch over [G * N, K] and the forward kernel on the copy), dW is
    ``grouped_gemm_tn`` in w's dtype; ``counts`` gets no gradient.  Neither
    direction synchronises with the host.  Like the forward's output, dX is written for the
    rows of the experts only: gradient rows at or past ``sum(counts)`` are unspecified
    (uninitialised memory), as are the output's."""
    if w.dtype not in (torch.bfloat16, torch.float32):
        raise TypeError("grouped_linear weights must be bf16 or fp32")
    return _GroupedLinear.apply(x, w, counts)


# ---------------------------------------------------------------------------
# fused top-k router (csrc/device/moe_gate.hip)
# ---------------------------------------------------------------------------
MOE_GATE_MAX_EXPERTS = 256  # = device.MOE_MAX_EXPERTS
MOE_GATE_MAX_TOPK = 8       # = device.MOE_MAX_TOPK
MOE_GATE_CHUNK = 64         # tokens per CTA (csrc/device/moe_gate.hpp kGateChunk): fixes prob_sum's summation order


def moe_gate_validate(logits, top_k: int):
    """Argument rules of ``moe_gate`` that need no GPU; raises TypeError (dtypes) / ValueError
    (shapes, bounds) and returns ``(T, E, K)``: ``logits`` [T, E] fp32 and contiguous,
    ``1 <= E <= 256``, ``1 <= top_k <= min(8, E)``, ``T >= 0``."""
    if logits.dtype != torch.float32:
        raise TypeError(f"moe_gate expects fp32 logits, got {logits.dtype}")
    if logits.dim() != 2:
        raise ValueError(f"moe_gate: logits must be [T, E], got {tuple(logits.shape)}")
    T, E = logits.shape
    K = int(top_k)
    if E < 1 or E > MOE_GATE_MAX_EXPERTS:
        raise ValueError(f"moe_gate: the number of experts must be in [1, {MOE_GATE_MAX_EXPERTS}], got {E}")
    if K < 1 or K > min(MOE_GATE_MAX_TOPK, E):
        raise ValueError(f"moe_gate: top_k must be in [1, min({MOE_GATE_MAX_TOPK}, E = {E})], got {K}")
    if not logits.is_contiguous():
        raise ValueError("moe_gate: logits must be contiguous")
    if T >= (1 << 31) - MOE_GATE_CHUNK:
        raise ValueError("moe_gate: T must be below 2^31 - 64")
    return int(T), int(E), K


def moe_gate_forward(logits: torch.Tensor, top_k: int, renormalize: bool = True):
    """The router in one pass over ``logits`` [T, E] (``k_moe_gate_fwd`` + the partial
    reduction): returns ``(weights [T, K] fp32, idx [T, K] int32, prob_sum [E] fp32,
    expert_tokens [E] int64)``, plain tensors, no autograd.  ``idx`` is the first K entries of a
    stable sort of the row by (-logit, index), in that order; ``weights`` are the softmax
    probabilities of those experts, divided by their sum when ``renormalize``;
    ``prob_sum[e] = sum_t p[t, e]``; ``expert_tokens[e]`` counts the (t, k) with ``idx == e``.
    ``-inf`` logits are legal (probability 0) while every row has a finite one.  No host
    synchronisation, no atomics: bitwise reproducible and capturable in a graph."""
    T, E, K = moe_gate_validate(logits, top_k)
    dev = logits.device
    chunks = (T + MOE_GATE_CHUNK - 1) // MOE_GATE_CHUNK
    weights = torch.empty((T, K), dtype=torch.float32, device=dev)
    idx = torch.empty((T, K), dtype=torch.int32, device=dev)
    prob_sum = torch.empty(E, dtype=torch.float32, device=dev)
    expert_tokens = torch.empty(E, dtype=torch.int64, device=dev)
    part_p = torch.empty((max(chunks, 1), E), dtype=torch.float32, device=dev)
    part_c = torch.empty((max(chunks, 1), E), dtype=torch.int32, device=dev)
    _D().moe_gate_fwd(logits.data_ptr(), weights.data_ptr(), idx.data_ptr(), part_p.data_ptr(), part_c.data_ptr(),
                      prob_sum.data_ptr(), expert_tokens.data_ptr(), T, E, K, bool(renormalize), _stream(logits))
    return weights, idx, prob_sum, expert_tokens


def moe_gate_backward(logits: torch.Tensor, idx: torch.Tensor, dweights: torch.Tensor,
                      dprob_sum: Optional[torch.Tensor] = None, renormalize: bool = True) -> torch.Tensor:
    """``dlogits`` [T, E] of ``moe_gate_forward`` (``k_moe_gate_bwd``): the probabilities are
    recomputed from ``logits``; ``idx`` [T, K] int32 is the forward's, ``dweights`` [T, K] fp32
    the gradient of its weights, ``dprob_sum`` [E] fp32 that of ``prob_sum`` (None: zero)."""
    T, E, _ = moe_gate_validate(logits, idx.shape[1] if idx.dim() == 2 else 0)
    K = idx.shape[1]
    if idx.dtype != torch.int32 or dweights.dtype != torch.float32:
        raise TypeError("moe_gate_backward expects int32 idx and fp32 dweights")
    if tuple(idx.shape) != (T, K) or tuple(dweights.shape) != (T, K) or not idx.is_contiguous() \
            or not dweights.is_contiguous():
        raise ValueError("moe_gate_backward: idx and dweights must be contiguous [T, K]")
    if dprob_sum is not None:
        if dprob_sum.dtype != torch.float32:
            raise TypeError("moe_gate_backward expects fp32 dprob_sum")
        if tuple(dprob_sum.shape) != (E,) or not dprob_sum.is_contiguous():
            raise ValueError("moe_gate_backward: dprob_sum must be a contiguous [E] tensor")
    for t in (idx, dweights, dprob_sum):
        if t is not None and t.device != logits.device:
            raise ValueError("moe_gate_backward: every tensor must be on the logits' device")
    dlogits = torch.empty_like(logits)
    _D().moe_gate_bwd(logits.data_ptr(), idx.data_ptr(), dweights.data_ptr(),
                      0 if dprob_sum is None else dprob_sum.data_ptr(), dlogits.data_ptr(), T, E, K,
                      bool(renormalize), _stream(logits))
    return dlogits


class _MoEGate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, top_k, renormalize):
        weights, idx, prob_sum, expert_tokens = moe_gate_forward(logits, top_k, renormalize)
        ctx.save_for_backward(logits, idx)
        ctx.renormalize = renormalize
        ctx.mark_non_differentiable(idx, expert_tokens)
        return weights, idx, prob_sum, expert_tokens

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dweights, _didx, dprob_sum, _dtokens):
        logits, idx = ctx.saved_tensors
        dweights = torch.zeros_like(idx, dtype=torch.float32) if dweights is None else dweights.contiguous()
        if dprob_sum is not None:
            dprob_sum = dprob_sum.contiguous()
        return moe_gate_backward(logits, idx, dweights, dprob_sum, ctx.renormalize), None, None


def moe_gate(logits: torch.Tensor, top_k: int, renormalize: bool = True):
    """Differentiable ``moe_gate_forward``: ``(weights, idx, prob_sum, expert_tokens)`` of the
    router ``logits`` [T, E] fp32, differentiable in ``logits`` through ``weights`` and
    ``prob_sum`` (one ``k_moe_gate_bwd`` launch, which recomputes the softmax from the saved
    logits: nothing else of size [T, E] is kept).  ``prob_sum`` and ``expert_tokens`` are the
    statistics of a load-balancing loss (``RoutedMoE.aux_loss``)."""
    moe_gate_validate(logits, top_k)
    return _MoEGate.apply(logits, int(top_k), bool(renormalize))


# ---------------------------------------------------------------------------
# router logits on the matrix cores (csrc/device/moe_router.hip)
# ---------------------------------------------------------------------------
def split_bf16x3(w: torch.Tensor, planes: int = 3, transpose: bool = False, out: Optional[torch.Tensor] = None, *,
                 concat=None, pad: int = 8) -> torch.Tensor:
    """An fp32 matrix ``w`` [R, C] as bf16 planes whose sum is ``w``: plane 0 is ``bf16(w)``, plane
    i is ``bf16(w - the earlier planes)``, every subtraction in fp32 and every rounding to nearest
    even; bit for bit ``p0 = w.bfloat16(); p1 = (w - p0.float()).bfloat16(); p2 = (w - p0.float()
    - p1.float()).bfloat16()``.  Three planes hold a finite fp32 number exactly.  Returns bf16
    ``[planes, R, C]``, or ``[planes, C, R]`` with ``transpose``.

    ``concat``: a sequence of 1 to 4 plane numbers, e.g. ``(0, 0, 1)``; the result is then 2-D, the
    named planes side by side along the last axis, ``[R, len(concat) * C']`` (``[C, len(concat) *
    R']`` with ``transpose``), every block's width rounded up to a multiple of ``pad`` and the
    padding zero: the operand of a GEMM that reduces over the planes in one pass.  ``planes`` is
    ignored then.  Inputs must be finite.  One kernel, no host synchronisation."""
    if w.dtype != torch.float32:
        raise TypeError(f"split_bf16x3 expects an fp32 tensor, got {w.dtype}")
    if w.dim() != 2 or not w.is_contiguous():
        raise ValueError("split_bf16x3 expects a contiguous 2-D tensor")
    R, C = w.shape
    slow, fast = (C, R) if transpose else (R, C)
    if concat is None:
        if not 1 <= int(planes) <= 3:
            raise ValueError(f"split_bf16x3: planes must be 1, 2 or 3, got {planes}")
        slots = list(range(int(planes)))
        shape, slot_stride, ld, fpad = (len(slots), slow, fast), slow * fast, fast, fast
    else:
        slots = [int(p) for p in concat]
        if not 1 <= len(slots) <= 4 or any(p < 0 or p > 2 for p in slots) or int(pad) < 1:
            raise ValueError("split_bf16x3: concat names 1 to 4 planes out of 0, 1, 2; pad >= 1")
        fpad = (fast + int(pad) - 1) // int(pad) * int(pad)
        shape, slot_stride, ld = (slow, len(slots) * fpad), fpad, len(slots) * fpad
    if not w.is_cuda:
        raise ValueError("split_bf16x3 runs on the GPU: w is on " + str(w.device))
    if out is None:
        out = torch.empty(shape, dtype=torch.bfloat16, device=w.device)
    elif out.dtype != torch.bfloat16 or tuple(out.shape) != tuple(shape) or not out.is_contiguous() \
            or out.device != w.device:
        raise ValueError(f"split_bf16x3: out must be a contiguous bf16 {tuple(shape)} tensor on w's device")
    if R and C:
        _D().split_bf16x3(w.data_ptr(), out.data_ptr(), R, C, len(slots), sum(p << (2 * s) for s, p in enumerate(slots)),
                          slot_stride, ld, fpad, bool(transpose), _stream(w))
    elif out.numel():
        out.zero_()
    return out


def moe_router_logits_validate(x, router):
    """Argument rules of ``moe_router_logits`` that need no GPU; raises TypeError (dtypes) /
    ValueError (shapes, strides, alignment) and returns ``(T, D, E)``: ``x`` [T, D] bf16 with unit
    column stride, a row stride that is a multiple of 8 and a 16-byte aligned base, ``D % 8 == 0``,
    ``0 <= T < 2^31 - 64``; ``router`` [E, D] fp32 and contiguous, ``1 <= E <= 256``."""
    if x.dtype != torch.bfloat16:
        raise TypeError(f"moe_router_logits expects bf16 activations, got {x.dtype}")
    if router.dtype != torch.float32:
        raise TypeError(f"moe_router_logits expects an fp32 router, got {router.dtype}")
    if x.dim() != 2 or router.dim() != 2:
        raise ValueError(f"moe_router_logits: x must be [T, D] and router [E, D], got {tuple(x.shape)} and "
                         f"{tuple(router.shape)}")
    T, D = x.shape
    E = router.shape[0]
    if router.shape[1] != D:
        raise ValueError(f"moe_router_logits: x has D = {D}, the router {router.shape[1]}")
    if D < 8 or D % 8:
        raise ValueError(f"moe_router_logits: D must be a positive multiple of 8, got {D}")
    if E < 1 or E > MOE_GATE_MAX_EXPERTS:
        raise ValueError(f"moe_router_logits: the number of experts must be in [1, {MOE_GATE_MAX_EXPERTS}], got {E}")
    if T >= (1 << 31) - MOE_GATE_CHUNK:
        raise ValueError("moe_router_logits: T must be below 2^31 - 64")
    if not router.is_contiguous():
        raise ValueError("moe_router_logits: the router must be contiguous")
    if x.stride(1) != 1 or (T > 1 and (x.stride(0) % 8 or x.stride(0) < D)):
        raise ValueError("moe_router_logits: x needs unit column stride and a row stride that is a multiple of 8")
    if x.data_ptr() % 16:
        raise ValueError("moe_router_logits: x must be 16-byte aligned")
    return int(T), int(D), int(E)


def _router_planes_check(planes, E: int, D: int, device) -> None:
    if planes.dtype != torch.bfloat16:
        raise TypeError("moe_router_logits: planes must be bf16 (split_bf16x3 of the router)")
    if tuple(planes.shape) != (3, E, D) or not planes.is_contiguous() or planes.data_ptr() % 16 \
            or planes.device != device:
        raise ValueError(f"moe_router_logits: planes must be a contiguous, 16-byte aligned [3, {E}, {D}] tensor on "
                         "x's device")


def moe_router_logits_forward(x: torch.Tensor, router: torch.Tensor, planes: Optional[torch.Tensor] = None,
                              out: Optional[torch.Tensor] = None, row_tile: Optional[int] = None) -> torch.Tensor:
    """``logits`` [T, E] fp32 ``= x . router^T`` on the matrix cores (``k_moe_router_logits``): the
    fp32 ``router`` [E, D] enters as its three bf16 planes (``split_bf16x3``; pass an earlier
    result as ``planes`` to skip the split), ``x`` [T, D] bf16 is read once, every product is exact
    and only the fp32 accumulation rounds.  One element is accumulated in an order that depends on
    D alone: no split-K, no atomics, so the result is bitwise reproducible and a token's logits do
    not depend on the other rows (``forward(x[:n]) == forward(x)[:n]``).  ``row_tile`` (128, 64 or
    32 rows per workgroup; None: the largest that gives every CU a workgroup) is a scheduling
    choice for tests and benchmarks: the bits do not depend on it.  Plain tensors, no autograd;
    no host synchronisation, and with ``planes`` and ``out`` no allocation."""
    T, D, E = moe_router_logits_validate(x, router)
    if not x.is_cuda or router.device != x.device:
        raise ValueError("moe_router_logits: x and the router must be on one GPU")
    if planes is None:
        planes = split_bf16x3(router)
    _router_planes_check(planes, E, D, x.device)
    if out is None:
        out = torch.empty((T, E), dtype=torch.float32, device=x.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (T, E) or not out.is_contiguous() or out.device != x.device:
        raise ValueError(f"moe_router_logits: out must be a contiguous fp32 [{T}, {E}] tensor on x's device")
    if row_tile not in (None, 32, 64, 128):
        raise ValueError(f"moe_router_logits: row_tile must be None, 32, 64 or 128, got {row_tile!r}")
    if T:
        _D().moe_router_logits_fwd(x.data_ptr(), planes.data_ptr(), out.data_ptr(), T, E, D, x.stride(0) if T > 1 else D,
                                   int(row_tile or 0), _stream(x))
    return out


def moe_router_logits_backward(dlogits: torch.Tensor, x: torch.Tensor, router_planes: torch.Tensor,
                               need_dx: bool = True, need_drouter: bool = True):
    """``(dx, drouter)`` of ``moe_router_logits_forward``: ``dx`` [T, D] bf16 ``= dlogits @ router``
    and ``drouter`` [E, D] fp32 ``= dlogits^T @ x`` (None where not needed), without an fp32 tensor
    of size [T, D].  ``dlogits`` [T, E] fp32 is split into bf16 planes d0, d1, d2 by one
    ``split_bf16x3`` launch.  ``dx`` is one ``gemm_nt`` over ``[d0 | d0 | d1] . [R0 | R1 | R0]^T``
    (``R`` the router planes; the dropped terms are below 2^-16 relative, under the bf16 rounding
    of the result); ``drouter`` is one ``gemm_tn`` of ``[d0 | d1 | d2]`` against ``x`` through the
    workspace reduction, its three [E, D] blocks summed in plane order 2, 1, 0.  No atomics."""
    if dlogits.dtype != torch.float32:
        raise TypeError(f"moe_router_logits_backward expects fp32 dlogits, got {dlogits.dtype}")
    if x.dtype != torch.bfloat16:
        raise TypeError(f"moe_router_logits_backward expects bf16 activations, got {x.dtype}")
    if dlogits.dim() != 2 or x.dim() != 2 or dlogits.shape[0] != x.shape[0]:
        raise ValueError("moe_router_logits_backward: dlogits must be [T, E] and x [T, D]")
    T, E = dlogits.shape
    D = x.shape[1]
    if not x.is_cuda or dlogits.device != x.device:
        raise ValueError("moe_router_logits_backward: dlogits and x must be on one GPU")
    _router_planes_check(router_planes, E, D, x.device)
    if x.stride(1) != 1 or (T > 1 and x.stride(0) % 8) or x.data_ptr() % 16:
        raise ValueError("moe_router_logits_backward: x needs unit column stride, a row stride that is a multiple of "
                         "8 and a 16-byte aligned base")
    if T == 0:
        return (torch.empty((0, D), dtype=torch.bfloat16, device=x.device) if need_dx else None,
                torch.zeros((E, D), dtype=torch.float32, device=x.device) if need_drouter else None)
    if not (need_dx or need_drouter):
        return None, None
    Ep = (E + 7) // 8 * 8
    # one split for both products: dx reads [d0 | d0 | d1], drouter [d0 | d1 | d2]
    slots = (0, 0, 1, 2) if need_dx and need_drouter else (0, 0, 1) if need_dx else (0, 1, 2)
    dl = split_bf16x3(dlogits.contiguous(), concat=slots, pad=8)
    dx = drouter = None
    if need_dx:
        alloc = torch.zeros if Ep != E else torch.empty
        rt = alloc((D, 3 * Ep), dtype=torch.bfloat16, device=x.device)
        for s, p in enumerate((0, 1, 0)):
            transpose(router_planes[p], out=rt[:, s * Ep:s * Ep + E])
        dx = gemm_nt(dl[:, :3 * Ep], rt, out_dtype=torch.bfloat16, splitk=1)
    if need_drouter:
        part = gemm_tn(dl[:, (len(slots) - 3) * Ep:], x, workspace=True)  # [3 E', D]
        drouter = (part[2 * Ep:2 * Ep + E] + part[Ep:Ep + E]) + part[:E]
    return dx, drouter


class _MoERouterLogits(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, router):
        planes = split_bf16x3(router)
        ctx.save_for_backward(x, planes)
        return moe_router_logits_forward(x, router, planes=planes)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dlogits):
        x, planes = ctx.saved_tensors
        return moe_router_logits_backward(dlogits, x, planes, ctx.needs_input_grad[0], ctx.needs_input_grad[1])


def moe_router_logits(x: torch.Tensor, router: torch.Tensor) -> torch.Tensor:
    """Differentiable ``moe_router_logits_forward``: ``x`` [T, D] bf16 and the fp32 ``router``
    [E, D] give fp32 ``logits`` [T, E], as exact as an fp32 GEMM, on the bf16 matrix cores.
    Autograd keeps ``x`` as the bf16 tensor it was given and the router's three bf16 planes; no
    fp32 copy of the activations exists in the forward or the backward
    (``moe_router_logits_backward``), and gradients are computed only for the inputs that ask."""
    moe_router_logits_validate(x, router)
    return _MoERouterLogits.apply(x, router)


# ---------------------------------------------------------------------------
# flash attention (csrc/device/flash_attn.hip)
# ---------------------------------------------------------------------------
FLASH_BQ = 128  # query rows per workgroup of the forward / dQ kernels (csrc/device/flash_attn.hpp kFlashBQ)
FLASH_BK = 64   # keys per step of their key loop = keys per workgroup of the dK/dV kernel (kFlashBK)
FLASH_HEAD_DIMS = (64, 128)
_FLASH_MAX_GRID = 65535  # B and Hq are grid dimensions


_FLASH_MAX_POS = 1 << 30
FLASH_MAX_SEQS = 65536  # sequences of one packed call (kFlashMaxSeqs)
# The three public faces of the one implementation below: (name used in messages, self form).  The
# self form is the chunk form with one length, q_pos0 = 0, no segments and contiguous dk / dv; it
# runs the self-attention instantiations of the kernels.  The packed form is the self form on
# [T, H, D] operands with ``cu_seqlens``: it runs the varlen instantiations.
_FLASH_SELF = ("flash_attention", True)
_FLASH_CHUNK = ("flash_attention_chunk", False)
_FLASH_VARLEN = ("flash_attention_varlen", True)


def flash_is_view(t) -> bool:
    """Whether a [B, S, H, D] (packed: [T, H, D]) tensor can be read as it is (the stride rules of
    ``_flash_view_check``)."""
    return (t.stride(-1) == 1 and all(t.shape[ax] == 1 or t.stride(ax) % 8 == 0 for ax in range(t.dim() - 1))
            and t.data_ptr() % 16 == 0)


def _flash_view_check(public: str, name: str, t) -> None:
    """The stride rules of an operand read as a view, [B, S, H, D], packed [T, H, D] or segmented [n, B, L, H, D]:
    unit stride on D, every other stride (of an axis longer than 1) a multiple of 8 elements,
    16-byte-aligned base."""
    shape, stride = t.shape, t.stride()
    if stride[-1] != 1:
        raise ValueError(f"{public}: {name} must have unit stride on the head dim, got strides {stride}")
    for ax in range(len(shape) - 1):
        if shape[ax] > 1 and stride[ax] % 8:
            what = f"the segment stride {stride[ax]}" if len(shape) == 5 and ax == 0 else f"stride {stride[ax]} of axis {ax}"
            raise ValueError(f"{public}: {what} of {name} is not a multiple of 8 elements")
    if t.data_ptr() % 16:
        raise ValueError(f"{public}: {name} must start at a 16-byte-aligned address")


def _flash_view(t):
    """A view as the extension takes it: (address, segment, batch, row, head stride) in elements;
    0 for an axis of length 1 and for the axes a 4-D (no segments) or packed 3-D (one batch entry)
    tensor does not have."""
    st = [s if n > 1 else 0 for n, s in zip(t.shape[:-1], t.stride())]
    return (t.data_ptr(), *[0] * (4 - len(st)), *st)


def _flash_validate(public: str, self_form: bool, q, k, v, q_pos0=0, kv_segment=None, cu_seqlens=None):
    """The one rule list behind ``flash_attention_validate``, ``flash_attention_chunk_validate`` and
    ``flash_attention_varlen_validate``; returns ``(B, Sq, Sk, L, Hq, Hkv, D)``.  The self form adds
    one rule: k and v have the length of q.  With ``cu_seqlens`` the operands are packed [T, H, D]:
    they go through the rules as the one batch entry [1, T, H, D] they are (B = 1, Sq = Sk = T)."""
    for name, t in (("q", q), ("k", k), ("v", v)):
        if t.dtype != torch.bfloat16:
            raise TypeError(f"{public} expects bf16 {name}, got {t.dtype}")
    if cu_seqlens is not None:
        if not isinstance(cu_seqlens, torch.Tensor) or cu_seqlens.dtype != torch.int32:
            raise TypeError(f"{public}: cu_seqlens must be an int32 tensor, got "
                            f"{getattr(cu_seqlens, 'dtype', type(cu_seqlens).__name__)}")
        for name, t in (("q", q), ("k", k), ("v", v)):
            if t.dim() != 3:
                raise ValueError(f"{public}: {name} must be [T, H, D], got {tuple(t.shape)}")
        if cu_seqlens.dim() != 1 or cu_seqlens.shape[0] < 2 or not cu_seqlens.is_contiguous():
            raise ValueError(f"{public}: cu_seqlens must be a contiguous [n + 1] tensor with n >= 1, got shape "
                             f"{tuple(cu_seqlens.shape)}, strides {cu_seqlens.stride()}")
        if cu_seqlens.shape[0] - 1 > FLASH_MAX_SEQS:
            raise ValueError(f"{public}: at most {FLASH_MAX_SEQS} sequences, got {cu_seqlens.shape[0] - 1}")
        if cu_seqlens.device != q.device:
            raise ValueError(f"{public}: cu_seqlens must be on the device of q ({q.device}), got {cu_seqlens.device}")
        q, k, v = q.unsqueeze(0), k.unsqueeze(0), v.unsqueeze(0)
    if isinstance(q_pos0, bool) or not isinstance(q_pos0, int):
        raise ValueError(f"{public}: q_pos0 must be an int, got {q_pos0!r}")
    segmented = kv_segment is not None
    if segmented and (isinstance(kv_segment, bool) or not isinstance(kv_segment, int) or kv_segment < 1):
        raise ValueError(f"{public}: kv_segment must be None or a positive int, got {kv_segment!r}")
    for name, t in (("q", q), ("k", k), ("v", v)):
        if segmented and name != "q":
            if t.dim() != 5:
                raise ValueError(f"{public}: with kv_segment, {name} must be [n, B, L, Hkv, D], got {tuple(t.shape)}")
        elif t.dim() != 4:
            raise ValueError(f"{public}: {name} must be [B, S, H, D], got {tuple(t.shape)}")
    B, Sq, Hq, D = q.shape
    if segmented:
        n, _, L, Hkv, _ = k.shape
        want = (n, B, kv_segment, Hkv, D)
        if L != kv_segment or tuple(k.shape) != want or tuple(v.shape) != want:
            raise ValueError(f"{public}: k and v must both be [n, B = {B}, L = {kv_segment}, Hkv, D = {D}], "
                             f"got {tuple(k.shape)} and {tuple(v.shape)}")
        Sk = n * L
    else:
        _, Sk, Hkv, _ = k.shape
        L = Sk
        if tuple(k.shape) != (B, Sk, Hkv, D) or tuple(v.shape) != (B, Sk, Hkv, D):
            raise ValueError(f"{public}: k and v must both be [B = {B}, Sk, Hkv, D = {D}], got "
                             f"{tuple(k.shape)} and {tuple(v.shape)}")
    if self_form and Sk != Sq:
        raise ValueError(f"{public}: k and v must be [B = {B}, S = {Sq}, Hkv, D = {D}] like q, got "
                         f"{tuple(k.shape)} and {tuple(v.shape)}")
    if D not in FLASH_HEAD_DIMS:
        raise ValueError(f"{public}: the head dim must be one of {FLASH_HEAD_DIMS}, got {D}")
    if Sq < 1 or Sk < 1:
        raise ValueError(f"{public}: q and k must have at least one position")
    if Sk > _FLASH_MAX_POS:
        raise ValueError(f"{public}: {'S' if self_form else 'Sk'} must be at most 2^30")
    if q_pos0 < 0:
        raise ValueError(f"{public}: q_pos0 must be >= 0 (key 0 is visible to every row), got {q_pos0}")
    if q_pos0 + Sq > _FLASH_MAX_POS:
        raise ValueError(f"{public}: q_pos0 + Sq must be at most 2^30")
    if Hkv < 1 or Hq % Hkv:
        raise ValueError(f"{public}: Hq = {Hq} must be a multiple of Hkv = {Hkv}")
    if not (1 <= B <= _FLASH_MAX_GRID and Hq <= _FLASH_MAX_GRID):
        raise ValueError(f"{public}: B and Hq must be in [1, {_FLASH_MAX_GRID}], got {B} and {Hq}")
    if k.device != q.device or v.device != q.device:
        raise ValueError(f"{public}: q, k and v must be on one device")
    for name, t in (("q", q), ("k", k), ("v", v)):
        _flash_view_check(public, name, t)
    return int(B), int(Sq), int(Sk), int(L), int(Hq), int(Hkv), int(D)


def flash_attention_validate(q, k, v):
    """Argument rules of ``flash_attention`` that need no GPU; raises TypeError (dtypes) /
    ValueError (shapes, strides, alignment) and returns ``(B, S, Hq, Hkv, D)``.  ``q`` is
    [B, S, Hq, D], ``k`` and ``v`` [B, S, Hkv, D], all bf16, taken as views: unit stride on D,
    batch / sequence / head strides multiples of 8 elements, 16-byte-aligned base.
    ``Hq % Hkv == 0``, ``D`` in {64, 128}, ``S >= 1``."""
    B, S, _, _, Hq, Hkv, D = _flash_validate(*_FLASH_SELF, q, k, v)
    return B, S, Hq, Hkv, D


def flash_attention_chunk_validate(q, k, v, q_pos0: int = 0, kv_segment: Optional[int] = None):
    """Argument rules of ``flash_attention_chunk`` that need no GPU; raises TypeError (dtypes) /
    ValueError (everything else) and returns ``(B, Sq, Sk, L, Hq, Hkv, D)``.

    ``q`` is [B, Sq, Hq, D]: query row ``i`` sits at position ``q_pos0 + i`` of the key sequence
    (``q_pos0 >= 0``, ``q_pos0 + Sq <= 2^30``).  ``kv_segment=None``: ``k`` and ``v`` are
    [B, Sk, Hkv, D].  ``kv_segment=L``: they are 5-D views [n, B, L, Hkv, D] -- segment ``i`` holds
    keys ``[i L, (i + 1) L)``, ``Sk = n L`` -- the rank-major layout an all-gather of per-rank
    [B, L, Hkv, D] shards produces; the segment stride is ``k.stride(0)``.  All bf16 views: unit
    stride on D, every other stride a multiple of 8 elements, 16-byte-aligned base.  ``Sq`` and
    ``Sk`` are independent; ``1 <= Sk <= 2^30``."""
    return _flash_validate(*_FLASH_CHUNK, q, k, v, q_pos0, kv_segment)


def _flash_result(name: str, t, shape, dtype, like):
    """A caller's output / workspace: the exact shape, dtype and device, contiguous, aligned."""
    if t is None:
        return torch.empty(shape, dtype=dtype, device=like.device)
    if t.dtype != dtype:
        raise TypeError(f"flash_attention: {name} must be {dtype}, got {t.dtype}")
    if tuple(t.shape) != tuple(shape) or not t.is_contiguous() or t.device != like.device:
        raise ValueError(f"flash_attention: {name} must be a contiguous {tuple(shape)} tensor on {like.device}")
    if t.data_ptr() % 16:
        raise ValueError(f"flash_attention: {name} must start at a 16-byte-aligned address")
    return t


def _flash_kv_result(name: str, t, like_k):
    """A caller's dk / dv of the chunk form: the shape of ``k`` (5-D on the segmented path), bf16,
    on its device, under the view rules of ``k``; allocated contiguous when not given."""
    if t is None:
        return torch.empty(like_k.shape, dtype=torch.bfloat16, device=like_k.device)
    if t.dtype != torch.bfloat16:
        raise TypeError(f"flash_attention_chunk: {name} must be bf16, got {t.dtype}")
    if tuple(t.shape) != tuple(like_k.shape) or t.device != like_k.device:
        raise ValueError(f"flash_attention_chunk: {name} must be a {tuple(like_k.shape)} tensor on {like_k.device}, got "
                         f"{tuple(t.shape)}")
    _flash_view_check("flash_attention_chunk", name, t)
    return t


def _flash_scale(scale, D: int) -> float:
    s = D ** -0.5 if scale is None else float(scale)
    if not (s == s and abs(s) != float("inf")):
        raise ValueError("flash_attention: scale must be finite")
    return s


def _flash_packing(cu_seqlens):
    """The extension's last two arguments: (address of the boundaries, sequences), (0, 0) when not packed."""
    return (0, 0) if cu_seqlens is None else (cu_seqlens.data_ptr(), cu_seqlens.shape[0] - 1)


def _flash_forward(public, self_form, q, k, v, causal, scale, out, lse, q_pos0=0, kv_segment=None, cu_seqlens=None):
    B, Sq, Sk, L, Hq, Hkv, D = _flash_validate(public, self_form, q, k, v, q_pos0, kv_segment, cu_seqlens)
    sc = _flash_scale(scale, D)
    lead = (B,) if cu_seqlens is None else ()  # packed: out [T, Hq, D], lse [Hq, T]
    out = _flash_result("out", out, (*lead, Sq, Hq, D), torch.bfloat16, q)
    lse = _flash_result("lse", lse, (*lead, Hq, Sq), torch.float32, q)
    _D().flash_attn_fwd(_flash_view(q), _flash_view(k), _flash_view(v), out.data_ptr(), lse.data_ptr(), B, Sq, Sk, L,
                        q_pos0, Hq, Hkv, D, bool(causal), sc, self_form and cu_seqlens is None, _stream(q),
                        *_flash_packing(cu_seqlens))
    return out, lse


def _flash_backward(public, self_form, dout, q, k, v, out, lse, causal, scale, dq, dk, dv, delta, q_pos0=0,
                    kv_segment=None, cu_seqlens=None):
    B, Sq, Sk, L, Hq, Hkv, D = _flash_validate(public, self_form, q, k, v, q_pos0, kv_segment, cu_seqlens)
    sc = _flash_scale(scale, D)
    lead = (B,) if cu_seqlens is None else ()  # packed: [T, Hq, D] and [Hq, T]
    if dout.dtype != torch.bfloat16:
        raise TypeError(f"{public} expects bf16 dout, got {dout.dtype}")
    if tuple(dout.shape) != (*lead, Sq, Hq, D) or dout.device != q.device:
        raise ValueError(f"{public}: dout must be {(*lead, Sq, Hq, D)} on {q.device}, got {tuple(dout.shape)}")
    _flash_view_check(public, "dout", dout)
    if out is None or lse is None:
        raise ValueError(f"{public}_backward needs the forward's out and lse")
    out = _flash_result("out", out, (*lead, Sq, Hq, D), torch.bfloat16, q)
    lse = _flash_result("lse", lse, (*lead, Hq, Sq), torch.float32, q)

    def result(name, t):
        if name == "dq":
            return _flash_result(name, t, (*lead, Sq, Hq, D), torch.bfloat16, q)
        if name == "delta":
            return _flash_result(name, t, (*lead, Hq, Sq), torch.float32, q)
        # dk / dv: contiguous in the self form (its kernels ignore their strides), views like k in the chunk form
        return _flash_result(name, t, k.shape, torch.bfloat16, q) if self_form else _flash_kv_result(name, t, k)

    given = {"dq": dq, "dk": dk, "dv": dv, "delta": delta}
    # every caller-provided result is checked before anything is allocated or launched; which
    # error wins when two apply is each form's own order
    for name in ("dq", "dk", "dv", "delta") if self_form else ("dk", "dv", "dq", "delta"):
        if given[name] is not None:
            result(name, given[name])
    dq, dk, dv, delta = (result(name, t) for name, t in given.items())
    _D().flash_attn_bwd(_flash_view(dout), _flash_view(q), _flash_view(k), _flash_view(v), out.data_ptr(),
                        lse.data_ptr(), delta.data_ptr(), dq.data_ptr(), _flash_view(dk), _flash_view(dv), B, Sq, Sk, L,
                        q_pos0, Hq, Hkv, D, bool(causal), sc, self_form and cu_seqlens is None, _stream(q),
                        *_flash_packing(cu_seqlens))
    return dq, dk, dv


class _FlashAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, causal, scale, form, q_pos0, kv_segment, cu_seqlens=None):
        out, lse = _flash_forward(*form, q, k, v, causal, scale, None, None, q_pos0, kv_segment, cu_seqlens)
        ctx.save_for_backward(q, k, v, out, lse)
        ctx.cu_seqlens = cu_seqlens  # an index tensor, no gradient: the backward reads it as it is then
        ctx.args = (form, causal, scale, q_pos0, kv_segment)
        ctx.mark_non_differentiable(lse)
        return out, lse

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout, _dlse):
        q, k, v, out, lse = ctx.saved_tensors
        form, causal, scale, q_pos0, kv_segment = ctx.args
        if not flash_is_view(dout):  # e.g. an expanded or transposed gradient
            dout = dout.contiguous()
        dq, dk, dv = _flash_backward(*form, dout, q, k, v, out, lse, causal, scale, None, None, None, None, q_pos0,
                                     kv_segment, ctx.cu_seqlens)
        return dq, dk, dv, None, None, None, None, None, None


def flash_attention_forward(q, k, v, causal: bool = True, scale: Optional[float] = None, out=None, lse=None):
    """``softmax(scale * q k^T [+ causal mask]) v`` per (batch, query head), GQA without expanding
    K or V (``k_flash_fwd``): returns ``(out [B, S, Hq, D] bf16 contiguous, lse [B, Hq, S] fp32)``,
    ``lse`` the natural log of each row's sum of ``exp(scale * score)``.  Operands as
    ``flash_attention_validate`` describes (views: no transposed copy); ``scale`` defaults to
    ``1 / sqrt(D)``.  Plain tensors, no autograd; no host synchronisation, and no allocation
    when ``out`` and ``lse`` are passed, so the call can be captured in a graph."""
    return _flash_forward(*_FLASH_SELF, q, k, v, causal, scale, out, lse)


def flash_attention_backward(dout, q, k, v, out, lse, causal: bool = True, scale: Optional[float] = None,
                             dq=None, dk=None, dv=None, delta=None):
    """``(dq, dk, dv)`` of ``flash_attention_forward``: P is recomputed from ``q``, ``k`` and
    ``lse``; ``delta = rowsum(dout * out)`` is taken from the stored bf16 ``out`` (``delta``
    [B, Hq, S] fp32 is its workspace).  ``dout`` follows the stride rules of ``q``; ``dq`` is
    bf16 contiguous in the layout of ``out``, ``dk`` and ``dv`` bf16 contiguous [B, S, Hkv, D].
    Three launches (delta, dK/dV, dQ): one workgroup owns each dK/dV key block and sums over its
    query heads and query blocks in a fixed order, one owns each dQ block, so there are no
    atomics and the gradients are bitwise reproducible."""
    return _flash_backward(*_FLASH_SELF, dout, q, k, v, out, lse, causal, scale, dq, dk, dv, delta)


def flash_attention(q, k, v, causal: bool = True, scale: Optional[float] = None):
    """Differentiable ``flash_attention_forward``: ``out`` [B, S, Hq, D] bf16 of the bf16 views
    ``q`` [B, S, Hq, D], ``k`` / ``v`` [B, S, Hkv, D] (GQA: query head h reads kv head
    ``h // (Hq / Hkv)``), differentiable in all three.  Autograd keeps ``q``, ``k``, ``v``,
    ``out`` and ``lse``; nothing of size S x S exists."""
    flash_attention_validate(q, k, v)
    return _FlashAttention.apply(q, k, v, bool(causal), scale, _FLASH_SELF, 0, None)[0]


# The chunk form: a query chunk at an offset into a longer, possibly segmented key sequence.
def flash_attention_chunk_forward(q, k, v, causal: bool = True, scale: Optional[float] = None, out=None, lse=None, *,
                                  q_pos0: int = 0, kv_segment: Optional[int] = None):
    """``flash_attention_forward`` for a query chunk ``q`` [B, Sq, Hq, D] whose row 0 sits at
    position ``q_pos0`` of a key sequence of its own length ``Sk``: with ``causal``, key ``j`` is
    visible to row ``i`` iff ``j <= q_pos0 + i`` (``q_pos0`` is ignored without).  ``k`` / ``v`` as
    ``flash_attention_chunk_validate`` describes, segmented or not.  Returns ``(out [B, Sq, Hq, D]
    bf16 contiguous, lse [B, Hq, Sq] fp32)``; for a chunk of a self-attention call these are bitwise
    the full call's rows.  No host synchronisation, and no allocation when ``out`` and ``lse`` are
    passed."""
    return _flash_forward(*_FLASH_CHUNK, q, k, v, causal, scale, out, lse, q_pos0, kv_segment)


def flash_attention_chunk_backward(dout, q, k, v, out, lse, causal: bool = True, scale: Optional[float] = None,
                                   dq=None, dk=None, dv=None, delta=None, *, q_pos0: int = 0,
                                   kv_segment: Optional[int] = None):
    """``(dq, dk, dv)`` of ``flash_attention_chunk_forward``.  ``dq`` [B, Sq, Hq, D] bf16
    contiguous; ``dk`` / ``dv`` have the shape of ``k`` (5-D on the segmented path) and are written
    through their own strides under the view rules of ``k``, so they may be views of a larger
    buffer (the send buffer of a reduce-scatter); they hold this chunk's share only, and a key
    that no query of the chunk sees gets exact zeros.  ``delta`` [B, Hq, Sq] fp32 is the
    workspace.  With ``dq``, ``dk``, ``dv`` and ``delta`` passed the call allocates nothing."""
    return _flash_backward(*_FLASH_CHUNK, dout, q, k, v, out, lse, causal, scale, dq, dk, dv, delta, q_pos0, kv_segment)


def flash_attention_chunk(q, k, v, causal: bool = True, scale: Optional[float] = None, *, q_pos0: int = 0,
                          kv_segment: Optional[int] = None):
    """Differentiable ``flash_attention_chunk_forward``: ``out`` [B, Sq, Hq, D] bf16, differentiable
    in ``q``, ``k`` and ``v``; the gradients of ``k`` and ``v`` have their shape (5-D when
    segmented) and are this chunk's share."""
    flash_attention_chunk_validate(q, k, v, q_pos0, kv_segment)
    return _FlashAttention.apply(q, k, v, bool(causal), scale, _FLASH_CHUNK, q_pos0, kv_segment)[0]


# The packed form: sequences of different lengths back to back on one token axis.
def flash_attention_varlen_validate(q, k, v, cu_seqlens):
    """Argument rules of ``flash_attention_varlen`` that need no GPU; raises TypeError (dtypes,
    ``cu_seqlens`` included) / ValueError (everything else) and returns ``(T, n, Hq, Hkv, D)``.

    ``q`` is [T, Hq, D], ``k`` and ``v`` [T, Hkv, D], all bf16 views under the rules of
    ``flash_attention_validate`` (column slices of a fused [T, (Hq + 2 Hkv) D] buffer qualify),
    ``1 <= T <= 2^30``.  ``cu_seqlens`` is a contiguous int32 [n + 1] tensor on the device of ``q``,
    ``1 <= n <= 65536``: sequence ``i`` owns rows ``[cu[i], cu[i + 1])`` of all three operands.  Its
    CONTENTS are the caller's promise (``cu[0] = 0``, nondecreasing, ``cu[n] <= T``; zero lengths
    are legal) and are read on the device only: the kernels clamp them, so nothing outside the
    tensors is touched whatever they hold, ``cu[n] > T`` truncates the last sequence at ``T``,
    and any other broken promise gives unspecified values."""
    _, T, _, _, Hq, Hkv, D = _flash_validate(*_FLASH_VARLEN, q, k, v, cu_seqlens=_flash_boundaries(cu_seqlens))
    return T, int(cu_seqlens.shape[0]) - 1, Hq, Hkv, D


def _flash_boundaries(cu_seqlens):
    """``cu_seqlens`` of a packed call: never None, which would select the self form."""
    if cu_seqlens is None:
        raise TypeError("flash_attention_varlen: cu_seqlens must be an int32 tensor, got None")
    return cu_seqlens


def flash_varlen_tile_map(cu_seqlens, block: int, T: Optional[int] = None):
    """Host mirror of the packed kernels' slot map: one entry per slot of the grid's x axis,
    ``(sequence, tile, begin, end)`` for the workgroup that computes rows (``block = FLASH_BQ``:
    forward, dQ) or keys (``block = FLASH_BK``: dK/dV) ``[tile * block, (tile + 1) * block)`` of the
    sequence on rows ``[begin, end)`` of the token axis, ``None`` for a spare slot, which leaves at
    once.  ``cu_seqlens`` is a CPU tensor or a list of n + 1 boundaries, ``T`` the length of the
    token axis (default ``cu_seqlens[-1]``).  As in the kernel: ``begin = clamp(cu[i], 0, T)``,
    ``end = clamp(cu[i + 1], begin, T)``, sequence ``i`` owns the slots from ``begin // block + i``
    on, there are ``T // block + n`` slots, and a slot's sequence is found by bisection."""
    cu = [int(x) for x in (cu_seqlens.tolist() if isinstance(cu_seqlens, torch.Tensor) else cu_seqlens)]
    block, n = int(block), len(cu) - 1
    if block < 1 or n < 1:
        raise ValueError("flash_varlen_tile_map: block must be positive and cu_seqlens hold at least 2 boundaries")
    T = cu[-1] if T is None else int(T)
    if T < 1:
        raise ValueError(f"flash_varlen_tile_map: T must be positive, got {T}")

    def at(i):
        return min(max(cu[i], 0), T)

    slots = []
    for slot in range(T // block + n):
        lo, hi = 0, n
        while hi - lo > 1:
            mid = (lo + hi) >> 1
            if at(mid) // block + mid <= slot:
                lo = mid
            else:
                hi = mid
        begin = at(lo)
        end = max(at(lo + 1), begin)
        tile = slot - (begin // block + lo)
        slots.append(None if tile < 0 or tile * block >= end - begin else (lo, tile, begin, end))
    return slots


def flash_attention_varlen_forward(q, k, v, cu_seqlens, causal: bool = True, scale: Optional[float] = None, out=None,
                                   lse=None):
    """``flash_attention_forward`` inside every sequence of a packed token axis: ``q`` [T, Hq, D],
    ``k`` / ``v`` [T, Hkv, D] and ``cu_seqlens`` as ``flash_attention_varlen_validate`` describes.
    A row sees the keys of its own sequence only (those up to itself with ``causal``).  Returns
    ``(out [T, Hq, D] bf16 contiguous, lse [Hq, T] fp32)``; the rows of a sequence are bitwise what
    ``flash_attention_forward`` returns for that sequence alone, and rows from ``cu[n]`` on are not
    written.  The boundaries are read on the device: no host synchronisation, no allocation when
    ``out`` and ``lse`` are passed, and a captured graph follows the contents of ``cu_seqlens``."""
    return _flash_forward(*_FLASH_VARLEN, q, k, v, causal, scale, out, lse, cu_seqlens=_flash_boundaries(cu_seqlens))


def flash_attention_varlen_backward(dout, q, k, v, cu_seqlens, out, lse, causal: bool = True,
                                    scale: Optional[float] = None, dq=None, dk=None, dv=None, delta=None):
    """``(dq, dk, dv)`` of ``flash_attention_varlen_forward``: ``dq`` [T, Hq, D], ``dk`` / ``dv``
    [T, Hkv, D] bf16 contiguous, ``delta`` [Hq, T] fp32 the workspace; ``dout`` follows the stride
    rules of ``q``.  The rows of a sequence are bitwise ``flash_attention_backward`` of that
    sequence alone; rows from ``cu[n]`` on are not written.  With ``dq``, ``dk``, ``dv`` and
    ``delta`` passed the call allocates nothing and never synchronises with the host."""
    return _flash_backward(*_FLASH_VARLEN, dout, q, k, v, out, lse, causal, scale, dq, dk, dv, delta,
                           cu_seqlens=_flash_boundaries(cu_seqlens))


def flash_attention_varlen(q, k, v, cu_seqlens, causal: bool = True, scale: Optional[float] = None):
    """Differentiable ``flash_attention_varlen_forward``: ``out`` [T, Hq, D] bf16, differentiable in
    ``q``, ``k`` and ``v``.  Rows from ``cu_seqlens[n]`` on belong to no sequence: they are left
    unwritten and their gradients too, so the caller keeps them out of the loss and of the
    parameters' gradients (pack to ``cu_seqlens[n] = T``)."""
    flash_attention_varlen_validate(q, k, v, cu_seqlens)
    return _FlashAttention.apply(q, k, v, bool(causal), scale, _FLASH_VARLEN, 0, None, cu_seqlens)[0]


# ---------------------------------------------------------------------------
# fused cross-entropy over a shard of the vocabulary (csrc/device/xent.hip)
# ---------------------------------------------------------------------------
XENT_SWEEP = 2048  # columns one workgroup covers per sweep (csrc/device/xent.hpp kXentSweep): 256 threads x 8 bf16
XENT_CHUNK = 256   # rows per workgroup of the combine kernel (kXentChunk): fixes loss_sum's summation order
XENT_MAX_PARTIALS = 1024  # partials of one row: 16 ranks x 64 splits
_XENT_TARGET_GROUPS = 1024  # kXentTargetGroups
_XENT_MIN_SWEEPS = 4        # kXentMinSweeps
_XENT_MAX_SPLITS = 64       # kXentMaxSplits


def _xent_split_sweeps(T: int, Vloc: int) -> int:
    n = (Vloc + XENT_SWEEP - 1) // XENT_SWEEP
    want = 1 if T >= _XENT_TARGET_GROUPS else (_XENT_TARGET_GROUPS + T - 1) // T
    want = max(1, min(want, n // _XENT_MIN_SWEEPS, _XENT_MAX_SPLITS))
    return (n + want - 1) // want


def xent_row_splits(T: int, Vloc: int) -> int:
    """Column splits of one row in the cross-entropy kernels: split ``i`` covers the columns
    ``[i w, min((i + 1) w, Vloc))`` with ``w`` a whole number of ``XENT_SWEEP`` sweeps.  A pure
    function of ``(T, Vloc)`` (the mirror of csrc/device/xent.hpp, which the launcher checks) --
    never of the device or the grid: every split writes a partial of its own and the merge order
    is part of the result's bits.  1 whenever ``T >= 1024`` or ``Vloc <= 7 XENT_SWEEP``."""
    T, Vloc = int(T), int(Vloc)
    if T < 1 or Vloc < 1:
        raise ValueError(f"xent_row_splits: T and Vloc must be positive, got {T}, {Vloc}")
    per = _xent_split_sweeps(T, Vloc)
    return ((Vloc + XENT_SWEEP - 1) // XENT_SWEEP + per - 1) // per


def _xent_logits_rules(name: str, t) -> None:
    """[T, Vloc] bf16, unit column stride, row stride and Vloc multiples of 8, 16-byte-aligned base."""
    if t.dtype != torch.bfloat16:
        raise TypeError(f"cross_entropy expects bf16 {name}, got {t.dtype}")
    if t.dim() != 2:
        raise ValueError(f"cross_entropy: {name} must be [T, Vloc], got {tuple(t.shape)}")
    T, V = t.shape
    if T < 1:
        raise ValueError(f"cross_entropy: {name} needs at least one row (T >= 1)")
    if T >= 1 << 31:
        raise ValueError("cross_entropy: T must be below 2^31")
    if V < 8 or V % 8 or V >= (1 << 31) - XENT_SWEEP:
        raise ValueError(f"cross_entropy: Vloc must be a positive multiple of 8 below 2^31 - {XENT_SWEEP}, got {V}")
    if t.stride(1) != 1:
        raise ValueError(f"cross_entropy: {name} must have unit column stride, got {t.stride(1)}")
    if t.stride(0) % 8 or (T > 1 and t.stride(0) < V):
        raise ValueError(f"cross_entropy: the row stride of {name} must be a multiple of 8 and at least Vloc, got "
                         f"{t.stride(0)}")
    if t.data_ptr() % 16:
        raise ValueError(f"cross_entropy: {name} must start at a 16-byte-aligned address")


def cross_entropy_validate(logits, targets, vocab_start: int = 0):
    """Argument rules of the cross-entropy ops that need no GPU; raises TypeError (dtypes) /
    ValueError (the rest) and returns ``(T, Vloc)``: ``logits`` [T, Vloc] bf16 with unit column
    stride, row stride and ``Vloc`` multiples of 8, a 16-byte-aligned base and ``T >= 1`` (the
    head GEMM's output as it is, or a column / row view of a larger buffer); ``targets`` [T] int64,
    contiguous, on the logits' device, in GLOBAL vocabulary numbering; ``vocab_start >= 0`` the
    global index of column 0."""
    if targets.dtype != torch.int64:
        raise TypeError(f"cross_entropy expects int64 targets, got {targets.dtype}")
    _xent_logits_rules("logits", logits)
    T, V = logits.shape
    if targets.dim() != 1 or targets.shape[0] != T or not targets.is_contiguous():
        raise ValueError(f"cross_entropy: targets must be a contiguous [{T}] tensor, got {tuple(targets.shape)}")
    if targets.device != logits.device:
        raise ValueError(f"cross_entropy: targets are on {targets.device}, logits on {logits.device}")
    if int(vocab_start) < 0 or int(vocab_start) > 1 << 62:
        raise ValueError(f"cross_entropy: vocab_start must be in [0, 2^62], got {vocab_start}")
    return int(T), int(V)


def _xent_buffer(name: str, t, shape, dtype, device, align: int = 1):
    """A caller's buffer (exact shape, dtype, contiguous, on ``device``) or a fresh one."""
    if t is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if t.dtype != dtype:
        raise TypeError(f"cross_entropy: {name} must be {dtype}, got {t.dtype}")
    if tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError(f"cross_entropy: {name} must be a contiguous {tuple(shape)} tensor, got {tuple(t.shape)}")
    if t.device != device:
        raise ValueError(f"cross_entropy: {name} is on {t.device}, expected {device}")
    if t.data_ptr() % align:
        raise ValueError(f"cross_entropy: {name} must start at a {align}-byte-aligned address")
    return t


def cross_entropy_stats(logits, targets, vocab_start: int = 0, stats=None):
    """One read pass over ``logits`` (``k_xent_stats``): ``stats`` [splits, T, 4] fp32 with
    ``splits = xent_row_splits(T, Vloc)``, row ``t`` of split ``i`` holding ``(m, s, zt, hit)``:
    the max over the split's columns, the sum of ``exp(z - m)``, the target's logit when
    ``vocab_start <= target < vocab_start + Vloc`` lies in the split (else 0) and 1.0 / 0.0 for
    that test.  ``-inf`` logits are legal; an all ``-inf`` split gives ``(-inf, 0)``.  With
    ``stats`` passed the call allocates nothing and never synchronises with the host."""
    T, V = cross_entropy_validate(logits, targets, vocab_start)
    splits = xent_row_splits(T, V)
    stats = _xent_buffer("stats", stats, (splits, T, 4), torch.float32, logits.device, align=16)
    _D().xent_stats(logits.data_ptr(), targets.data_ptr(), stats.data_ptr(), T, V, logits.stride(0), int(vocab_start),
                    splits, _stream(logits))
    return stats


def cross_entropy_combine(stats, targets, ignore_index: int = -100, lse=None, row_loss=None, loss_sum=None,
                          n_valid=None, *, mean=None, work=None):
    """Merge the rows' partials (``k_xent_combine`` + ``k_xent_sum``): ``stats`` [P, T, 4] fp32
    (TP ranks x splits, rank-major), merged IN INDEX ORDER: ``M = max m_i``, ``S = sum s_i
    exp(m_i - M)``, ``lse = M + log S``, ``zt = sum zt_i``.  Returns ``(lse [T], row_loss [T],
    loss_sum [1])`` fp32 and ``n_valid [1]`` int64: ``row_loss = lse - zt``, exactly 0 where
    ``target == ignore_index``; ``loss_sum`` adds the rows of each ``XENT_CHUNK`` chunk in a fixed
    tree and the chunks in a fixed order (no atomics: the bits depend on T alone).  ``mean`` [1]
    fp32 (optional) receives ``loss_sum / n_valid``, 0 when no row is valid; ``work``
    [ceil(T / XENT_CHUNK), 2] fp32 is the chunk workspace.  A target that is neither
    ``ignore_index`` nor in the vocabulary is the caller's broken promise: values unspecified,
    addresses safe.  With every buffer passed the call allocates nothing and never synchronises."""
    if stats.dtype != torch.float32:
        raise TypeError(f"cross_entropy_combine expects fp32 stats, got {stats.dtype}")
    if targets.dtype != torch.int64:
        raise TypeError(f"cross_entropy_combine expects int64 targets, got {targets.dtype}")
    if stats.dim() != 3 or stats.shape[2] != 4 or stats.shape[0] < 1 or stats.shape[1] < 1 or not stats.is_contiguous():
        raise ValueError("cross_entropy_combine: stats must be a contiguous [P, T, 4] tensor, got "
                         f"{tuple(stats.shape)}")
    P, T = int(stats.shape[0]), int(stats.shape[1])
    if P > XENT_MAX_PARTIALS:
        raise ValueError(f"cross_entropy_combine: at most {XENT_MAX_PARTIALS} partials per row, got {P}")
    if stats.data_ptr() % 16:
        raise ValueError("cross_entropy_combine: stats must start at a 16-byte-aligned address")
    if tuple(targets.shape) != (T,) or not targets.is_contiguous() or targets.device != stats.device:
        raise ValueError(f"cross_entropy_combine: targets must be a contiguous [{T}] tensor on {stats.device}")
    dev = stats.device
    lse = _xent_buffer("lse", lse, (T,), torch.float32, dev)
    row_loss = _xent_buffer("row_loss", row_loss, (T,), torch.float32, dev)
    loss_sum = _xent_buffer("loss_sum", loss_sum, (1,), torch.float32, dev)
    n_valid = _xent_buffer("n_valid", n_valid, (1,), torch.int64, dev)
    if mean is not None:
        mean = _xent_buffer("mean", mean, (1,), torch.float32, dev)
    work = _xent_buffer("work", work, ((T + XENT_CHUNK - 1) // XENT_CHUNK, 2), torch.float32, dev)
    _D().xent_combine(stats.data_ptr(), targets.data_ptr(), lse.data_ptr(), row_loss.data_ptr(), loss_sum.data_ptr(),
                      n_valid.data_ptr(), 0 if mean is None else mean.data_ptr(), work.data_ptr(), P, T,
                      int(ignore_index), _stream(stats))
    return lse, row_loss, loss_sum, n_valid


def cross_entropy_backward(logits, targets, lse, n_valid, grad=None, vocab_start: int = 0, ignore_index: int = -100,
                           dlogits=None):
    """``dlogits[t, j] = (exp(z[t, j] - lse[t]) - [vocab_start + j == target[t]]) * g / n_valid``
    (``k_xent_backward``: one read pass, one write pass), the product in fp32, rounded once to
    bf16.  ``grad`` (``g``, one fp32 element; None: 1) and ``n_valid`` [1] int64 are read on the
    device.  Ignored rows store exact zeros; with ``n_valid == 0`` the mean loss is defined as 0
    and every ``dlogits`` is 0 (torch gives NaN there).  ``dlogits`` is [T, Vloc] bf16 under the
    rules of ``logits`` and may BE ``logits``.  With ``grad`` and ``dlogits`` passed the call
    allocates nothing and never synchronises with the host."""
    T, V = cross_entropy_validate(logits, targets, vocab_start)
    dev = logits.device
    if lse.dtype != torch.float32 or n_valid.dtype != torch.int64 or (grad is not None and grad.dtype != torch.float32):
        raise TypeError("cross_entropy_backward expects fp32 lse and grad and int64 n_valid")
    if tuple(lse.shape) != (T,) or not lse.is_contiguous():
        raise ValueError(f"cross_entropy_backward: lse must be a contiguous [{T}] tensor, got {tuple(lse.shape)}")
    if n_valid.numel() != 1 or (grad is not None and grad.numel() != 1):
        raise ValueError("cross_entropy_backward: n_valid and grad hold one element each")
    for t in (lse, n_valid, grad, dlogits):
        if t is not None and t.device != dev:
            raise ValueError("cross_entropy_backward: every tensor must be on the logits' device")
    if dlogits is None:
        dlogits = torch.empty((T, V), dtype=torch.bfloat16, device=dev)
    else:
        _xent_logits_rules("dlogits", dlogits)
        if tuple(dlogits.shape) != (T, V):
            raise ValueError(f"cross_entropy_backward: dlogits must be {(T, V)}, got {tuple(dlogits.shape)}")
    if grad is None:
        grad = torch.ones(1, dtype=torch.float32, device=dev)
    _D().xent_backward(logits.data_ptr(), targets.data_ptr(), lse.data_ptr(), n_valid.data_ptr(), grad.data_ptr(),
                       dlogits.data_ptr(), T, V, logits.stride(0), dlogits.stride(0), int(vocab_start),
                       int(ignore_index), _stream(logits))
    return dlogits


class _CrossEntropy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, targets, ignore_index):
        stats = cross_entropy_stats(logits, targets)
        mean = torch.empty(1, dtype=torch.float32, device=logits.device)
        lse, _, _, n_valid = cross_entropy_combine(stats, targets, ignore_index, mean=mean)
        ctx.save_for_backward(logits, targets, lse, n_valid)
        ctx.ignore_index = ignore_index
        return mean.view(())

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dloss):
        logits, targets, lse, n_valid = ctx.saved_tensors
        g = dloss.to(torch.float32).reshape(1)  # stays on the device: no host synchronisation
        return cross_entropy_backward(logits, targets, lse, n_valid, g, 0, ctx.ignore_index), None, None


def cross_entropy(logits, targets, ignore_index: int = -100):
    """Differentiable mean cross-entropy of ``logits`` [T, V] bf16 against ``targets`` [T] int64
    over the rows whose target is not ``ignore_index`` (fp32 scalar; 0, with zero gradients, when
    no row is valid -- torch gives NaN there).  Saves ``logits``, ``lse`` [T] and ``n_valid``; the
    backward is one ``k_xent_backward`` launch.  No fp32 [T, V] tensor exists at any point.  Sum
    and per-token reductions: build them from ``cross_entropy_combine``'s ``row_loss``."""
    cross_entropy_validate(logits, targets)
    return _CrossEntropy.apply(logits, targets, int(ignore_index))


def cross_entropy_merge_reference(stats, targets, ignore_index: int = -100):
    """The merge rule of ``cross_entropy_combine`` in torch fp64, partials in index order:
    ``(lse, row_loss, loss_sum, n_valid)``."""
    st = stats.double()
    M = st[:, :, 0].max(dim=0).values
    S = torch.zeros_like(M)
    zt = torch.zeros_like(M)
    for i in range(st.shape[0]):
        m, s = st[i, :, 0], st[i, :, 1]
        live = m != float("-inf")
        S = S + torch.where(live, s * torch.exp(torch.where(live, m - M, torch.zeros_like(m))), torch.zeros_like(s))
        zt = zt + st[i, :, 2]
    lse = M + torch.log(S)
    valid = targets != ignore_index
    row_loss = torch.where(valid, lse - zt, torch.zeros_like(lse))
    return lse, row_loss, row_loss.sum(), valid.sum()


def cross_entropy_reference(logits, targets, vocab_start: int = 0, ignore_index: int = -100, *, grad: float = 1.0,
                            lse=None, n_valid=None):
    """The cross-entropy ops in torch fp64 (any device): returns ``(stats [splits, T, 4], lse [T],
    row_loss [T], dlogits [T, Vloc])``, ``dlogits`` before its rounding to bf16.  ``stats`` follows
    ``xent_row_splits``; ``lse`` and ``row_loss`` are those of this shard alone (the unsplit
    ``logsumexp``).  ``dlogits`` uses ``grad``, and the whole vocabulary's ``lse`` / ``n_valid``
    when they are passed (a shard of a vocab-parallel loss) instead of this shard's own."""
    z = logits.double()
    T, V = z.shape
    col = targets - int(vocab_start)
    hit = (col >= 0) & (col < V)
    safe = torch.where(hit, col, torch.zeros_like(col))
    splits = xent_row_splits(T, V)
    width = _xent_split_sweeps(T, V) * XENT_SWEEP
    stats = torch.zeros((splits, T, 4), dtype=torch.float64, device=z.device)
    for i in range(splits):
        c0, c1 = i * width, min((i + 1) * width, V)
        m = z[:, c0:c1].max(dim=1).values
        live = m != float("-inf")
        base = torch.where(live, m, torch.zeros_like(m))
        here = hit & (col >= c0) & (col < c1)
        stats[i, :, 0] = m
        stats[i, :, 1] = torch.exp(z[:, c0:c1] - base[:, None]).sum(dim=1)
        stats[i, :, 2] = torch.where(here, z.gather(1, safe[:, None])[:, 0], torch.zeros_like(m))
        stats[i, :, 3] = here.double()
    own_lse = torch.logsumexp(z, dim=1)
    valid = targets != ignore_index
    zt = torch.where(hit, z.gather(1, safe[:, None])[:, 0], torch.zeros_like(own_lse))
    row_loss = torch.where(valid, own_lse - zt, torch.zeros_like(own_lse))
    L = own_lse if lse is None else lse.double()
    n = int(valid.sum()) if n_valid is None else int(n_valid)
    onehot = torch.zeros_like(z)
    onehot.scatter_(1, safe[:, None], hit.double()[:, None])
    scale = float(grad) / n if n > 0 else 0.0
    dlogits = torch.where(valid[:, None] & (n > 0), (torch.exp(z - L[:, None]) - onehot) * scale, torch.zeros_like(z))
    return stats, own_lse, row_loss, dlogits


# ---------------------------------------------------------------------------
# rotary position embedding (csrc/device/rope.hip)
# ---------------------------------------------------------------------------
ROPE_MAX_SEQS = 65536  # sequences of one packed call (csrc/device/rope.hpp kRopeMaxSeqs)
ROPE_MAX_TOKENS = 1 << 30
ROPE_MAX_HEADS = 65535  # of q and of k, each (the extension's limit)
ROPE_MAX_LANES = 64  # head lanes of a token (csrc/device/rope.hpp kRopeMaxLanes)
ROPE_MAX_THREADS = 256 * (2 ** 31 - 1)  # tokens x D / 16 x head lanes: workgroups of 256 threads on a 31-bit grid


def rope_table(n_pos: int, D: int, theta: float = 500000.0, inv_freq=None, device=None):
    """The ``[n_pos, 2, D / 2]`` fp32 table ``ops.rope_apply`` reads: ``table[p, 0, j] = cos(p f_j)``,
    ``table[p, 1, j] = sin(p f_j)`` with ``f_j = theta^(-2 j / D)``, computed in fp64 on the CPU and
    rounded once to fp32.  ``inv_freq`` ([D / 2] float64) replaces the formula: any frequency
    scaling is a matter of the table, the kernel never sees an angle."""
    if isinstance(n_pos, bool) or not isinstance(n_pos, int) or n_pos < 1:
        raise ValueError(f"rope_table: n_pos must be a positive int, got {n_pos!r}")
    if isinstance(D, bool) or not isinstance(D, int) or D < 2 or D % 2:
        raise ValueError(f"rope_table: D must be a positive even int, got {D!r}")
    if inv_freq is None:
        if not theta > 0:
            raise ValueError(f"rope_table: theta must be positive, got {theta!r}")
        inv_freq = torch.tensor([float(theta) ** (-2.0 * j / D) for j in range(D // 2)], dtype=torch.float64)
    else:
        if not isinstance(inv_freq, torch.Tensor) or inv_freq.dtype != torch.float64:
            raise TypeError(f"rope_table: inv_freq must be a float64 tensor, got {getattr(inv_freq, 'dtype', type(inv_freq).__name__)}")
        if tuple(inv_freq.shape) != (D // 2,):
            raise ValueError(f"rope_table: inv_freq must be [D / 2 = {D // 2}], got {tuple(inv_freq.shape)}")
        inv_freq = inv_freq.detach().cpu()
    ang = torch.arange(n_pos, dtype=torch.float64)[:, None] * inv_freq[None, :]
    table = torch.stack((torch.cos(ang), torch.sin(ang)), dim=1).to(torch.float32).contiguous()
    return table if device is None else table.to(device)


def _rope_same_or_apart(name: str, x, out) -> None:
    """An output is its input (the same address AND strides: in place) or lies elsewhere."""
    if out.data_ptr() == x.data_ptr() and out.stride() != x.stride():
        raise ValueError(f"rope_apply: {name}_out starts at the address of {name} with other strides "
                         f"({out.stride()} against {x.stride()}): in place means the same view")


def rope_validate(q, k, table, pos0: int = 0, cu_seqlens=None, q_out=None, k_out=None):
    """Argument rules of ``rope_apply`` / ``rope`` that need no GPU; raises TypeError (dtypes, those
    of ``table`` and ``cu_seqlens`` included) / ValueError (everything else) and returns
    ``(B, S, Hq, Hkv, D, P)`` -- ``B = 1``, ``S = T`` in the packed form, ``Hkv = 0`` without ``k``.

    Batched (``cu_seqlens=None``): ``q`` [B, S, Hq, D], ``k`` [B, S, Hkv, D] or None; row ``s`` sits
    at position ``pos0 + s``, ``pos0 >= 0`` and ``pos0 + S <= P``.  Packed: ``q`` [T, Hq, D], ``k``
    [T, Hkv, D] or None, ``cu_seqlens`` a contiguous int32 [n + 1] tensor on the device of ``q``,
    ``1 <= n <= 65536``, under the promises of ``flash_attention_varlen_validate`` (its contents are
    read on the device only), ``pos0 = 0``.  ``q`` and ``k`` agree in every dimension but the heads,
    which are independent.  All bf16 views: unit stride on D, every other stride a multiple of 8
    elements, 16-byte-aligned base; ``D % 16 == 0``, ``16 <= D <= 256``.  ``table`` is a contiguous,
    16-byte-aligned fp32 [P, 2, D / 2] tensor on that device.  ``q_out`` / ``k_out``: the shape,
    dtype and device of their input under the same view rules, each with strides of its own; an
    output may be its input (the same view).  Beyond that the caller promises what is not checked: an
    output overlaps no operand other than the input it replaces, not in part and not at another
    base address, and no output view overlaps itself (a stride of 0 on an axis longer than 1);
    threads would race on such memory, at addresses inside the tensors.  ``tokens x D / 16 x
    min(Hq + Hkv, 64)`` is at most ``256 x (2^31 - 1)`` (the grid)."""
    pub = "rope_apply"
    for name, t in (("q", q), ("k", k), ("q_out", q_out), ("k_out", k_out)):
        if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != torch.bfloat16):
            raise TypeError(f"{pub} expects bf16 {name}, got {getattr(t, 'dtype', type(t).__name__)}")
    if not isinstance(q, torch.Tensor):
        raise TypeError(f"{pub} expects a bf16 tensor q, got {type(q).__name__}")
    if not isinstance(table, torch.Tensor) or table.dtype != torch.float32:
        raise TypeError(f"{pub}: table must be an fp32 tensor, got {getattr(table, 'dtype', type(table).__name__)}")
    packed = cu_seqlens is not None
    if packed and (not isinstance(cu_seqlens, torch.Tensor) or cu_seqlens.dtype != torch.int32):
        raise TypeError(f"{pub}: cu_seqlens must be an int32 tensor, got "
                        f"{getattr(cu_seqlens, 'dtype', type(cu_seqlens).__name__)}")
    if isinstance(pos0, bool) or not isinstance(pos0, int):
        raise ValueError(f"{pub}: pos0 must be an int, got {pos0!r}")
    if k is None and k_out is not None:
        raise ValueError(f"{pub}: k_out without k")
    rank = 3 if packed else 4
    form = "[T, H, D] (with cu_seqlens)" if packed else "[B, S, H, D] (with pos0)"
    if q.dim() != rank:
        raise ValueError(f"{pub}: q must be {form}, got {tuple(q.shape)}")
    if packed:
        if pos0 != 0:
            raise ValueError(f"{pub}: cu_seqlens and a non-zero pos0 ({pos0}) exclude each other")
        if cu_seqlens.dim() != 1 or cu_seqlens.shape[0] < 2 or not cu_seqlens.is_contiguous():
            raise ValueError(f"{pub}: cu_seqlens must be a contiguous [n + 1] tensor with n >= 1, got shape "
                             f"{tuple(cu_seqlens.shape)}, strides {cu_seqlens.stride()}")
        if cu_seqlens.shape[0] - 1 > ROPE_MAX_SEQS:
            raise ValueError(f"{pub}: at most {ROPE_MAX_SEQS} sequences, got {cu_seqlens.shape[0] - 1}")
        if cu_seqlens.device != q.device:
            raise ValueError(f"{pub}: cu_seqlens must be on the device of q ({q.device}), got {cu_seqlens.device}")
    elif pos0 < 0:
        raise ValueError(f"{pub}: pos0 must be >= 0, got {pos0}")
    *lead, Hq, D = (int(x) for x in q.shape)
    B, S = (1, lead[0]) if packed else lead
    Hkv = 0
    if k is not None:
        if k.dim() != rank or tuple(k.shape[:-2]) != tuple(q.shape[:-2]) or k.shape[-1] != D:
            raise ValueError(f"{pub}: k must agree with q {tuple(q.shape)} in every dimension but the heads, got "
                             f"{tuple(k.shape)}")
        Hkv = int(k.shape[-2])
        if k.device != q.device:
            raise ValueError(f"{pub}: q and k must be on one device")
    if D < 16 or D > 256 or D % 16:
        raise ValueError(f"{pub}: the head dim must be a multiple of 16 in [16, 256], got {D}")
    if B < 1 or S < 1 or B * S > ROPE_MAX_TOKENS:
        raise ValueError(f"{pub}: 1 <= tokens <= 2^30 required, got {tuple(q.shape)}")
    if not (1 <= Hq <= ROPE_MAX_HEADS) or (k is not None and not (1 <= Hkv <= ROPE_MAX_HEADS)):
        raise ValueError(f"{pub}: the heads must be in [1, {ROPE_MAX_HEADS}], got {Hq}" + (f" and {Hkv}" if k is not None else ""))
    if B * S * (D // 16) * min(Hq + Hkv, ROPE_MAX_LANES) > ROPE_MAX_THREADS:
        raise ValueError(f"{pub}: tokens x D / 16 x min(heads, {ROPE_MAX_LANES}) = {B * S} x {D // 16} x "
                         f"{min(Hq + Hkv, ROPE_MAX_LANES)} exceeds the grid (256 x (2^31 - 1) threads)")
    if table.dim() != 3 or table.shape[0] < 1 or tuple(table.shape[1:]) != (2, D // 2):
        raise ValueError(f"{pub}: table must be [P, 2, D / 2 = {D // 2}], got {tuple(table.shape)}")
    P = int(table.shape[0])
    if P > ROPE_MAX_TOKENS:
        raise ValueError(f"{pub}: at most 2^30 table rows, got {P}")
    if not table.is_contiguous() or table.data_ptr() % 16:
        raise ValueError(f"{pub}: table must be contiguous and start at a 16-byte-aligned address")
    if table.device != q.device:
        raise ValueError(f"{pub}: table must be on the device of q ({q.device}), got {table.device}")
    if not packed and pos0 + S > P:
        raise ValueError(f"{pub}: pos0 + S = {pos0} + {S} exceeds the table's {P} positions")
    for name, x, out in (("q", q, q_out), ("k", k, k_out)):
        if x is None:
            continue
        _flash_view_check(pub, name, x)
        if out is not None:
            if tuple(out.shape) != tuple(x.shape) or out.device != x.device:
                raise ValueError(f"{pub}: {name}_out must be a {tuple(x.shape)} tensor on {x.device}, got "
                                 f"{tuple(out.shape)} on {out.device}")
            _flash_view_check(pub, name + "_out", out)
            _rope_same_or_apart(name, x, out)
    return B, S, Hq, Hkv, D, P


def _rope_view(t):
    """A view as the extension takes it: (address, batch, token, head stride) in elements; 0 for an
    axis of length 1 and for the batch axis a packed [T, H, D] tensor does not have."""
    st = [s if n > 1 else 0 for n, s in zip(t.shape[:-1], t.stride())]
    return (t.data_ptr(), *[0] * (3 - len(st)), *st)


def rope_apply(q, k, table, pos0: int = 0, cu_seqlens=None, interleaved: bool = False, inverse: bool = False,
               q_out=None, k_out=None, *, _lanes: int = 0):
    """Rotate ``q`` and, when given, ``k`` by their positions' angles in ONE launch; returns
    ``(q_out, k_out)``, ``(q_out, None)`` for ``k=None``.  Operands as ``rope_validate`` describes.

    Each pair ``(x1, x2)`` of a head becomes ``(x1 c - x2 s, x2 c + x1 s)`` with ``c`` / ``s`` the
    table's cos / sin of (position, frequency ``j``): the pair is ``(x[j], x[j + D/2])`` (half-split,
    the layout of Hugging Face Llama checkpoints) or, ``interleaved=True``, ``(x[2j], x[2j + 1])``
    (Meta's original layout).  fp32 arithmetic, one rounding to bf16.  ``inverse=True`` uses ``-s``:
    the transpose of the rotation, i.e. its backward.  The position of a row is ``pos0 + s``
    (``pos0 = r S_loc`` on rank ``r`` of a context-parallel group), or with ``cu_seqlens`` the
    token's index inside its document, the boundaries read -- and clamped as in
    ``flash_attention_varlen`` -- on the device; rows from ``cu_seqlens[n]`` on are not written.  The
    table row is clamped to ``P - 1`` on the device: a packed document longer than ``P`` gives
    unspecified values at safe addresses.

    With every output passed the call allocates nothing and never synchronises with the host, so
    it can be captured in a graph, and a replay follows the contents of ``cu_seqlens``.  An output
    may be its input.  Outputs the call allocates are contiguous.  ``v`` is none of its business.
    ``_lanes`` is private (the benchmark's sweep and one test): it overrides how the heads are dealt
    to a token's threads, 0 = the kernel's own choice; the results are bitwise the same for every value."""
    B, S, Hq, Hkv, D, P = rope_validate(q, k, table, pos0, cu_seqlens, q_out, k_out)
    if q_out is None:
        q_out = torch.empty(q.shape, dtype=torch.bfloat16, device=q.device)
    if k is not None and k_out is None:
        k_out = torch.empty(k.shape, dtype=torch.bfloat16, device=k.device)
    none = (0, 0, 0, 0)
    _D().rope_apply(_rope_view(q), _rope_view(q_out), Hq, none if k is None else _rope_view(k),
                    none if k is None else _rope_view(k_out), Hkv, table.data_ptr(), P, B, S, D, int(pos0),
                    *_flash_packing(cu_seqlens), bool(interleaved), bool(inverse), int(_lanes), _stream(q))
    return q_out, k_out


class _Rope(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, table, pos0, cu_seqlens, interleaved):
        ctx.save_for_backward(table)
        ctx.cu_seqlens = cu_seqlens  # an index tensor, no gradient: the backward reads it as it is then
        ctx.args = (pos0, interleaved, k is not None)
        q_out, k_out = rope_apply(q, k, table, pos0, cu_seqlens, interleaved)
        return q_out, k_out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dq, dk):
        (table,) = ctx.saved_tensors
        pos0, interleaved, has_k = ctx.args
        dq = dq if flash_is_view(dq) else dq.contiguous()
        if has_k:
            dk = dk if flash_is_view(dk) else dk.contiguous()
        dq, dk = rope_apply(dq, dk if has_k else None, table, pos0, ctx.cu_seqlens, interleaved, inverse=True)
        return dq, dk, None, None, None, None


def rope(q, k, table, pos0: int = 0, cu_seqlens=None, interleaved: bool = False):
    """Differentiable ``rope_apply``, out of place: ``(q_out, k_out)`` contiguous bf16,
    differentiable in ``q`` and ``k`` (``k`` may be None).  The backward is one
    ``rope_apply(..., inverse=True)`` launch on the incoming gradients (made contiguous when they
    do not follow the view rules).  In the packed form rows from ``cu_seqlens[n]`` on are left
    unwritten, and their gradients too."""
    rope_validate(q, k, table, pos0, cu_seqlens)
    return _Rope.apply(q, k, table, int(pos0), cu_seqlens, bool(interleaved))


def rope_reference(x, table, positions, interleaved: bool = False, inverse: bool = False):
    """The rotation in torch fp64 (any device), before any rounding: ``x`` [..., H, D],
    ``positions`` an int64 tensor over the token axes ``x.shape[:-2]``, ``table`` [P, 2, D / 2].
    Pair ``j`` of a head -- ``(x[j], x[j + D/2])``, interleaved ``(x[2j], x[2j + 1])`` -- becomes
    ``(x1 c - x2 s, x2 c + x1 s)`` with ``c, s = table[position, 0 / 1, j]`` (``-s`` for
    ``inverse``)."""
    x = x.double()
    D = x.shape[-1]
    if positions.dtype != torch.int64 or tuple(positions.shape) != tuple(x.shape[:-2]):
        raise ValueError(f"rope_reference: positions must be int64 {tuple(x.shape[:-2])}, got {positions.dtype} "
                         f"{tuple(positions.shape)}")
    rows = table.double()[positions.to(table.device)].to(x.device)  # [..., 2, D / 2]
    c, s = rows[..., 0, :].unsqueeze(-2), rows[..., 1, :].unsqueeze(-2)
    if inverse:
        s = -s
    x1, x2 = (x[..., 0::2], x[..., 1::2]) if interleaved else (x[..., : D // 2], x[..., D // 2:])
    y1, y2 = x1 * c - x2 * s, x2 * c + x1 * s
    if interleaved:
        return torch.stack((y1, y2), dim=-1).reshape(x.shape)
    return torch.cat((y1, y2), dim=-1)


# ---------------------------------------------------------------------------
# RMSNorm with the residual add in front of it (csrc/device/rmsnorm.hip)
# ---------------------------------------------------------------------------
RMS_NORM_MAX_D = 16384      # csrc/device/rmsnorm.hpp kRmsMaxD
RMS_NORM_MAX_ROWS = 1 << 30  # kRmsMaxRows
_RMS_MIN_CHUNK = 8          # kRmsMinChunk
_RMS_MAX_CHUNK = 32         # kRmsMaxChunk
_RMS_TARGET_GROUPS = 1024   # kRmsTargetGroups


def rms_norm_row_chunk(T: int, d: int) -> int:
    """Rows per workgroup of ``rms_norm_backward``: ``clamp(ceil(T / 1024), 8, 32)``, a pure
    function of ``(T, d)`` (the mirror of csrc/device/rmsnorm.hpp, which the launcher checks) and
    never of the device or the grid.  A chunk's rows are added into its ``dw`` partial in row
    order and the partials in a fixed order, so the rule is part of ``dw``'s bits; ``partials`` is
    ``[ceil(T / chunk), d]`` fp32."""
    T, d = int(T), int(d)
    if T < 1 or d < 1:
        raise ValueError(f"rms_norm_row_chunk: T and d must be positive, got {T}, {d}")
    return max(_RMS_MIN_CHUNK, min(_RMS_MAX_CHUNK, (T + _RMS_TARGET_GROUPS - 1) // _RMS_TARGET_GROUPS))


def _rms_rows_rules(name: str, t, shape=None, device=None) -> None:
    """[T, d] bf16, unit column stride, row stride a multiple of 8, 16-byte-aligned base."""
    if not isinstance(t, torch.Tensor) or t.dtype != torch.bfloat16:
        raise TypeError(f"rms_norm expects bf16 {name}, got {getattr(t, 'dtype', type(t).__name__)}")
    if t.dim() != 2:
        raise ValueError(f"rms_norm: {name} must be [T, d], got {tuple(t.shape)}")
    T, d = (int(n) for n in t.shape)
    if shape is not None and (T, d) != tuple(shape):
        raise ValueError(f"rms_norm: {name} must be {tuple(shape)}, got {(T, d)}")
    if d < 8 or d > RMS_NORM_MAX_D or d % 8:
        raise ValueError(f"rms_norm: d must be a multiple of 8 in [8, {RMS_NORM_MAX_D}], got {d}")
    if T < 1 or T > RMS_NORM_MAX_ROWS:
        raise ValueError(f"rms_norm: 1 <= T <= 2^30 required, got {T}")
    if t.stride(1) != 1:
        raise ValueError(f"rms_norm: {name} must have unit column stride, got {t.stride(1)}")
    if T > 1 and t.stride(0) % 8:
        raise ValueError(f"rms_norm: the row stride of {name} must be a multiple of 8 elements, got {t.stride(0)}")
    if t.data_ptr() % 16:
        raise ValueError(f"rms_norm: {name} must start at a 16-byte-aligned address")
    if device is not None and t.device != device:
        raise ValueError(f"rms_norm: {name} is on {t.device}, expected {device}")


def _rms_weight_rules(weight, d: int, device) -> None:
    if not isinstance(weight, torch.Tensor) or weight.dtype not in (torch.bfloat16, torch.float32):
        raise TypeError(f"rms_norm expects a bf16 or fp32 weight, got {getattr(weight, 'dtype', type(weight).__name__)}")
    if tuple(weight.shape) != (d,) or not weight.is_contiguous():
        raise ValueError(f"rms_norm: weight must be a contiguous [{d}] tensor, got shape {tuple(weight.shape)}, strides "
                         f"{weight.stride()}")
    if weight.data_ptr() % 16:
        raise ValueError("rms_norm: weight must start at a 16-byte-aligned address")
    if weight.device != device:
        raise ValueError(f"rms_norm: weight is on {weight.device}, expected {device}")


def _rms_same_or_apart(name: str, out, *inputs) -> None:
    """An output is an input (the same address AND strides: in place) or lies elsewhere."""
    for x in inputs:
        if x is not None and out.data_ptr() == x.data_ptr() and out.shape[0] > 1 and out.stride() != x.stride():
            raise ValueError(f"rms_norm: {name} starts at the address of an operand with other strides "
                             f"({out.stride()} against {x.stride()}): in place means the same view")


def rms_norm_validate(x, weight, residual=None, eps: float = 1e-5, h=None, y=None):
    """Argument rules of the RMSNorm forward ops that need no GPU; raises TypeError (dtypes) /
    ValueError (the rest) and returns ``(T, d)``.  ``x``, ``residual``, ``h``, ``y`` are [T, d]
    bf16 views of one shape on one device: unit column stride, a row stride that is a multiple of
    8 elements (each its own: a row view or a column slice of a larger buffer qualifies), a
    16-byte-aligned base; ``8 <= d <= 16384``, ``d % 8 == 0``, ``1 <= T <= 2^30``.  ``weight`` is
    [d] bf16 or fp32, contiguous, 16-byte aligned; ``eps`` a positive host float.  ``h`` needs
    ``residual`` and may BE ``x`` or ``residual`` (the same view).  The caller promises what is not
    checked: no output overlaps an operand in any other way, and no output view overlaps itself."""
    _rms_rows_rules("x", x)
    T, d = (int(n) for n in x.shape)
    if residual is not None:
        _rms_rows_rules("residual", residual, (T, d), x.device)
    _rms_weight_rules(weight, d, x.device)
    if isinstance(eps, bool) or not isinstance(eps, (int, float)) or not eps > 0 or eps == float("inf") \
            or not torch.tensor(float(eps), dtype=torch.float32).item() > 0:
        raise ValueError(f"rms_norm: eps must be a positive float, got {eps!r}")
    if h is not None:
        if residual is None:
            raise ValueError("rms_norm: h without residual")
        _rms_rows_rules("h", h, (T, d), x.device)
        _rms_same_or_apart("h", h, x, residual)
    if y is not None:
        _rms_rows_rules("y", y, (T, d), x.device)
    return T, d


def _rms_view(t):
    """A view as the extension takes it: (address, row stride in elements; 0 for one row)."""
    return (0, 0) if t is None else (t.data_ptr(), t.stride(0) if t.shape[0] > 1 else 0)


def _rms_buffer(name: str, t, shape, device, align: int):
    """A caller's fp32 buffer (exact shape, contiguous, on ``device``) or a fresh one."""
    if t is None:
        return torch.empty(shape, dtype=torch.float32, device=device)
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
        raise TypeError(f"rms_norm: {name} must be fp32, got {getattr(t, 'dtype', type(t).__name__)}")
    if tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError(f"rms_norm: {name} must be a contiguous {tuple(shape)} tensor, got {tuple(t.shape)}")
    if t.device != device:
        raise ValueError(f"rms_norm: {name} is on {t.device}, expected {device}")
    if t.data_ptr() % align:
        raise ValueError(f"rms_norm: {name} must start at a {align}-byte-aligned address")
    return t


def add_rms_norm_forward(x, residual, weight, eps: float, h=None, y=None, rstd=None):
    """``h = bf16(x + residual)`` -- one fp32 add, rounded once: the bits of torch's bf16 ``x +
    residual`` -- then, of the ROUNDED ``h``: ``rstd[t] = 1 / sqrt(mean_j h[t, j]^2 + eps)`` (fp32
    [T]) and ``y[t, j] = bf16(h[t, j] * rstd[t] * weight[j])`` (products in fp32, one rounding), in
    ONE launch (``k_rmsnorm_fwd``): each row is read once, kept in registers and written once
    (twice: ``h`` and ``y``).  Returns ``(h, y, rstd)``.  Operands as ``rms_norm_validate``
    describes; ``h`` may be ``x`` or ``residual``.  A row's results depend on that row and ``d``
    alone, never on ``T`` or the other rows.  With ``h``, ``y`` and ``rstd`` passed the call
    allocates nothing and never synchronises with the host; outputs it allocates are contiguous."""
    if residual is None:
        raise ValueError("rms_norm: add_rms_norm_forward needs a residual (rms_norm_forward takes none)")
    T, d = rms_norm_validate(x, weight, residual, eps, h, y)
    rstd = _rms_buffer("rstd", rstd, (T,), x.device, 4)
    if h is None:
        h = torch.empty((T, d), dtype=torch.bfloat16, device=x.device)
    if y is None:
        y = torch.empty((T, d), dtype=torch.bfloat16, device=x.device)
    _D().rms_norm_fwd(_rms_view(x), _rms_view(residual), _rms_view(h), _rms_view(y), weight.data_ptr(),
                      weight.dtype == torch.float32, rstd.data_ptr(), T, d, float(eps), _stream(x))
    return h, y, rstd


def rms_norm_forward(x, weight, eps: float, y=None, rstd=None):
    """``add_rms_norm_forward`` without a residual (``h`` is ``x``): returns ``(y, rstd)``."""
    T, d = rms_norm_validate(x, weight, None, eps, None, y)
    rstd = _rms_buffer("rstd", rstd, (T,), x.device, 4)
    if y is None:
        y = torch.empty((T, d), dtype=torch.bfloat16, device=x.device)
    _D().rms_norm_fwd(_rms_view(x), (0, 0), (0, 0), _rms_view(y), weight.data_ptr(), weight.dtype == torch.float32,
                      rstd.data_ptr(), T, d, float(eps), _stream(x))
    return y, rstd


def rms_norm_backward(dy, h, weight, rstd, dres=None, dh=None, dw=None, partials=None, need_dw: bool = True):
    """With ``n = h * rstd`` and ``g = dy * weight``: ``dh[t, j] = bf16(rstd[t] * (g[t, j] - n[t, j]
    * mean_k(g[t, k] n[t, k])) + dres[t, j])``, rounded once, and ``dw[j] = sum_t dy[t, j] *
    n[t, j]`` in fp32 ([d], whatever the weight's dtype).  ``dres`` is the gradient that reaches
    ``h`` through the residual stream (None: zeros, bit for bit).  Returns ``(dh, dw)``.

    ``dy``, ``h``, ``dres``, ``dh`` are [T, d] bf16 views under the rules of ``rms_norm_validate``;
    ``dh`` may BE ``dy`` or ``dres``.  ``rstd`` is the forward's [T] fp32.  ``k_rmsnorm_bwd`` gives a
    workgroup ``rms_norm_row_chunk(T, d)`` consecutive rows and writes their column sums, added in
    row order, into ``partials`` (fp32 ``[ceil(T / chunk), d]``); ``k_rmsnorm_dw`` adds the partials
    in a fixed order.  No atomics: ``dw`` is bitwise reproducible and does not depend on the
    device.  ``need_dw=False`` skips both (``dw`` and ``partials`` are not touched; ``(dh, None)``).
    With ``dh``, ``dw`` and ``partials`` passed the call allocates nothing and never synchronises."""
    _rms_rows_rules("dy", dy)
    T, d = (int(n) for n in dy.shape)
    dev = dy.device
    _rms_rows_rules("h", h, (T, d), dev)
    if dres is not None:
        _rms_rows_rules("dres", dres, (T, d), dev)
    _rms_weight_rules(weight, d, dev)
    if rstd is None:
        raise ValueError("rms_norm: rms_norm_backward needs the forward's rstd")
    rstd = _rms_buffer("rstd", rstd, (T,), dev, 4)
    if dh is not None:
        _rms_rows_rules("dh", dh, (T, d), dev)
        _rms_same_or_apart("dh", dh, dy, dres)
    chunk = rms_norm_row_chunk(T, d)
    if need_dw:
        dw = _rms_buffer("dw", dw, (d,), dev, 4)
        partials = _rms_buffer("partials", partials, ((T + chunk - 1) // chunk, d), dev, 16)
    if dh is None:
        dh = torch.empty((T, d), dtype=torch.bfloat16, device=dev)
    _D().rms_norm_bwd(_rms_view(dy), _rms_view(h), _rms_view(dres), _rms_view(dh), weight.data_ptr(),
                      weight.dtype == torch.float32, rstd.data_ptr(), partials.data_ptr() if need_dw else 0,
                      dw.data_ptr() if need_dw else 0, T, d, chunk, _stream(dy))
    return dh, (dw if need_dw else None)


def _rms_grad_rows(g):
    """An incoming gradient as the kernel reads it (made contiguous when it breaks the view
    rules, e.g. the expanded scalar of a sum); None stays None."""
    if g is None:
        return None
    ok = g.dim() == 2 and g.stride(1) == 1 and (g.shape[0] == 1 or g.stride(0) % 8 == 0) and g.data_ptr() % 16 == 0
    return g if ok else g.contiguous()


class _AddRMSNorm(torch.autograd.Function):
    """(x, residual or None, weight) -> (h, y); without a residual h is x and only y is returned."""

    @staticmethod
    def forward(ctx, x, residual, weight, eps):
        if residual is None:
            y, rstd = rms_norm_forward(x, weight, eps)
            h = x
        else:
            h, y, rstd = add_rms_norm_forward(x, residual, weight, eps)
        ctx.save_for_backward(h, weight, rstd)  # never y
        ctx.has_residual = residual is not None
        ctx.need_dw = weight.requires_grad
        return (h, y) if residual is not None else y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *grads):
        h, weight, rstd = ctx.saved_tensors
        dres, dy = grads if ctx.has_residual else (None, grads[0])
        dy = torch.zeros_like(h) if dy is None else _rms_grad_rows(dy)  # no dy: zeros for the norm path and dw
        dh, dw = rms_norm_backward(dy, h, weight, rstd, _rms_grad_rows(dres), need_dw=ctx.need_dw)
        if dw is not None:
            dw = dw.to(weight.dtype)
        return (dh if ctx.needs_input_grad[0] else None, dh if ctx.has_residual and ctx.needs_input_grad[1] else None,
                dw, None)


def rms_norm(x, weight, eps: float):
    """Differentiable ``rms_norm_forward``: ``y`` [T, d] bf16, contiguous, differentiable in ``x``
    and ``weight``.  Saves ``x``, ``weight`` and ``rstd``, never ``y``; the backward is one
    ``rms_norm_backward`` launch and returns ``dw`` cast to the weight's dtype."""
    rms_norm_validate(x, weight, None, eps)
    return _AddRMSNorm.apply(x, None, weight, float(eps))


def add_rms_norm(x, residual, weight, eps: float):
    """Differentiable ``add_rms_norm_forward``: ``(h, y)``, both differentiable, in ``x``,
    ``residual`` and ``weight``.  The backward receives the gradients of both outputs (either may
    be missing), makes ONE ``rms_norm_backward`` launch with the gradient of ``h`` as ``dres``,
    and returns the same ``dh`` tensor for ``x`` and for ``residual`` and ``dw`` cast to the
    weight's dtype.  Saves ``h``, ``weight`` and ``rstd``, never ``y``."""
    rms_norm_validate(x, weight, residual, eps)
    return _AddRMSNorm.apply(x, residual, weight, float(eps))


def rms_norm_reference(x, weight, eps: float, residual=None):
    """The forward in torch fp64 (any device), written from the formulas: returns ``(h, y, rstd)``
    with ``h = bf16(x + residual)`` (torch's own bf16 add; ``x`` without a residual), ``rstd = 1 /
    sqrt(mean_j h^2 + eps)`` and ``y = h * rstd * weight`` before its rounding, both fp64."""
    h = x if residual is None else x + residual
    hd = h.double()
    rstd = 1.0 / torch.sqrt((hd * hd).mean(dim=-1) + float(eps))
    return h, hd * rstd[:, None] * weight.double()[None, :], rstd


def rms_norm_backward_reference(dy, h, weight, eps: float, dres=None):
    """The backward in torch fp64 (any device): ``(dh, dw)`` before any rounding, ``rstd``
    recomputed from ``h`` in fp64: ``n = h * rstd``, ``g = dy * weight``, ``dh = rstd * (g - n *
    mean_k(g n)) + dres``, ``dw = sum_t dy * n``."""
    hd, dyd = h.double(), dy.double()
    rstd = 1.0 / torch.sqrt((hd * hd).mean(dim=-1, keepdim=True) + float(eps))
    n = hd * rstd
    g = dyd * weight.double()[None, :]
    dh = rstd * (g - n * (g * n).mean(dim=-1, keepdim=True))
    if dres is not None:
        dh = dh + dres.double()
    return dh, (dyd * n).sum(dim=0)


# ---------------------------------------------------------------------------
# AdamW with on-device gradient-norm clipping over flat buckets (csrc/device/optim.hip)
# ---------------------------------------------------------------------------
OPTIM_CHUNK = 2048          # elements per slot (csrc/device/optim.hpp kOptimChunk): 256 threads x 8
OPTIM_MAX_GRID = 4096       # kOptimMaxGrid
OPTIM_MAX_SEGS = 1 << 24    # kOptimMaxSegs
OPTIM_MAX_ELEMS = 1 << 40   # kOptimMaxElems
OPTIM_DECAY = 1             # seg_flags bit 0: weight decay applies
OPTIM_SHARDED = 2           # seg_flags bit 1: counted in the "sharded" norm sum
_OPTIM_DTYPES = (torch.bfloat16, torch.float32)


def optim_slots(n: int, S: int, chunk: int = OPTIM_CHUNK) -> int:
    """Slots of a bucket of ``n`` elements in ``S`` segments: ``n // chunk + S`` (the length of
    the ``partials`` workspace)."""
    return int(n) // int(chunk) + int(S)


def optim_tile_map(seg_off, chunk: int = OPTIM_CHUNK, slots=None):
    """Host mirror of the optimizer kernels' slot map: one entry per slot, ``(segment, begin,
    end)`` for the workgroup pass that covers elements ``[begin, end)`` of the bucket, all inside
    that segment, ``None`` for a spare slot.  ``seg_off`` is a CPU tensor or a list of ``S + 1``
    offsets.  As in the kernel: segment ``i`` owns the slots from ``seg_off[i] // chunk + i`` on,
    there are ``n // chunk + S`` slots, and a slot's segment is found by bisection.  ``slots``: an
    iterable of slot numbers to map instead of all of them (a table of 2^33 elements has 4 M)."""
    off = [int(x) for x in (seg_off.tolist() if isinstance(seg_off, torch.Tensor) else seg_off)]
    chunk, S = int(chunk), len(off) - 1
    if chunk < 1 or S < 1:
        raise ValueError("optim_tile_map: chunk must be positive and seg_off hold at least 2 offsets")
    n = off[-1]
    if off[0] != 0 or any(off[i + 1] <= off[i] for i in range(S)):
        raise ValueError("optim_tile_map: seg_off must start at 0 and increase strictly")
    total = n // chunk + S
    out = []
    for slot in (range(total) if slots is None else slots):
        slot = int(slot)
        if not 0 <= slot < total:
            raise ValueError(f"optim_tile_map: slot {slot} outside [0, {total})")
        lo, hi = 0, S
        while hi - lo > 1:
            mid = (lo + hi) >> 1
            if off[mid] // chunk + mid <= slot:
                lo = mid
            else:
                hi = mid
        b = off[lo] + (slot - (off[lo] // chunk + lo)) * chunk
        out.append(None if b >= off[lo + 1] else (lo, b, min(b + chunk, off[lo + 1])))
    return out


def _optim_flat(name: str, t, dtypes, n=None, device=None, align: int = 16):
    if not isinstance(t, torch.Tensor) or t.dtype not in dtypes:
        raise TypeError(f"optim: {name} must be {' or '.join(str(d) for d in dtypes)}, got "
                        f"{getattr(t, 'dtype', type(t).__name__)}")
    if t.dim() != 1 or not t.is_contiguous() or t.numel() < 1:
        raise ValueError(f"optim: {name} must be a contiguous 1-D tensor, got shape {tuple(t.shape)}")
    if n is not None and t.numel() != n:
        raise ValueError(f"optim: {name} must hold {n} elements, got {t.numel()}")
    if device is not None and t.device != device:
        raise ValueError(f"optim: {name} is on {t.device}, expected {device}")
    if t.data_ptr() % align:
        raise ValueError(f"optim: {name} must start at a {align}-byte-aligned address")


def _optim_small(name: str, t, dtype, shape, device):
    if not isinstance(t, torch.Tensor) or t.dtype != dtype:
        raise TypeError(f"optim: {name} must be {dtype}, got {getattr(t, 'dtype', type(t).__name__)}")
    if tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError(f"optim: {name} must be a contiguous {tuple(shape)} tensor, got {tuple(t.shape)}")
    if t.device != device:
        raise ValueError(f"optim: {name} is on {t.device}, expected {device}")


def _optim_sums_rules(sums, device, bucket=None):
    if not isinstance(sums, torch.Tensor) or sums.dtype != torch.float64:
        raise TypeError(f"optim: sums must be float64, got {getattr(sums, 'dtype', type(sums).__name__)}")
    if sums.dim() != 2 or sums.shape[0] != 2 or sums.shape[1] < 1 or sums.stride(1) != 1:
        raise ValueError(f"optim: sums must be [2, buckets] with unit column stride, got {tuple(sums.shape)}")
    if sums.shape[1] > (1 << 20):
        raise ValueError("optim: at most 2^20 buckets")
    if sums.device != device:
        raise ValueError(f"optim: sums is on {sums.device}, expected {device}")
    if bucket is not None and not (isinstance(bucket, int) and 0 <= bucket < sums.shape[1]):
        raise ValueError(f"optim: bucket {bucket!r} outside [0, {sums.shape[1]})")


def optim_validate(g, seg_off, seg_ptr=None, seg_flags=None, p32=None, m=None, v=None, partials=None, sums=None,
                   bucket: int = 0, clip=None, sched=None, betas=(0.9, 0.999), eps: float = 1e-8, max_grid: int = 0):
    """Argument rules of the optimizer ops that need no GPU; raises TypeError (dtypes) / ValueError
    (the rest) and returns ``(n, S)``.  ``g`` is the bucket: 1-D contiguous bf16 or fp32, 16-byte
    aligned, ``1 <= n <= 2^40``.  ``seg_off`` [S + 1] int64, ``seg_ptr`` [S] int64 and ``seg_flags``
    [S] int32 are contiguous tensors on ``g``'s device, ``1 <= S <= min(n, 2^24)``; a ``seg_off``
    that lives on the CPU is also read: it starts at 0, increases strictly and ends at ``n`` (a
    device table is the caller's promise: the call never synchronises).  ``p32`` (bf16 buckets
    only; an fp32 parameter is its own master), ``m``, ``v``: fp32 [n], contiguous, 16-byte aligned.
    ``partials``: fp32, at least ``n // OPTIM_CHUNK + S`` elements.  ``sums``: fp64 [2, buckets]
    with unit column stride, ``bucket`` a column of it.  ``clip``: fp32 [2]; ``sched``: fp32 [4].
    ``betas`` in [0, 1), ``eps`` non-negative and finite, ``max_grid`` in [0, 4096] (0: automatic)."""
    _optim_flat("the gradient bucket", g, _OPTIM_DTYPES)
    n, dev = g.numel(), g.device
    if n > OPTIM_MAX_ELEMS:
        raise ValueError(f"optim: 1 <= n <= 2^40 required, got {n}")
    if not isinstance(seg_off, torch.Tensor) or seg_off.dtype != torch.int64:
        raise TypeError(f"optim: seg_off must be int64, got {getattr(seg_off, 'dtype', type(seg_off).__name__)}")
    if seg_off.dim() != 1 or not seg_off.is_contiguous() or seg_off.numel() < 2:
        raise ValueError(f"optim: seg_off must be a contiguous [S + 1] tensor, got shape {tuple(seg_off.shape)}")
    S = seg_off.numel() - 1
    if S > min(n, OPTIM_MAX_SEGS):
        raise ValueError(f"optim: 1 <= S <= min(n, 2^24) required, got S = {S}, n = {n}")
    if seg_off.device.type == "cpu":
        off = seg_off.tolist()
        if off[0] != 0 or off[-1] != n or any(off[i + 1] <= off[i] for i in range(S)):
            raise ValueError(f"optim: seg_off must start at 0, increase strictly and end at n = {n}")
    if seg_off.device != dev:
        raise ValueError(f"optim: seg_off is on {seg_off.device}, expected {dev}")
    for name, t, dt in (("seg_ptr", seg_ptr, torch.int64), ("seg_flags", seg_flags, torch.int32)):
        if t is not None:
            _optim_small(name, t, dt, (S,), dev)
    f32 = g.dtype == torch.float32
    if f32 and p32 is not None:
        raise ValueError("optim: an fp32 bucket has no p32: the parameter is its own master")
    for name, t in (("p32", p32), ("m", m), ("v", v)):
        if t is not None:
            _optim_flat(name, t, (torch.float32,), n, dev)
    if partials is not None:
        _optim_flat("partials", partials, (torch.float32,), None, dev, 4)
        if partials.numel() < optim_slots(n, S):
            raise ValueError(f"optim: partials must hold n // {OPTIM_CHUNK} + S = {optim_slots(n, S)} elements, got "
                             f"{partials.numel()}")
    if sums is not None:
        _optim_sums_rules(sums, dev, bucket)
    if clip is not None:
        _optim_small("clip", clip, torch.float32, (2,), dev)
    if sched is not None:
        _optim_small("sched", sched, torch.float32, (4,), dev)
    _optim_hyper(betas, eps)
    if isinstance(max_grid, bool) or not isinstance(max_grid, int) or not 0 <= max_grid <= OPTIM_MAX_GRID:
        raise ValueError(f"optim: max_grid must be an int in [0, {OPTIM_MAX_GRID}], got {max_grid!r}")
    return n, S


def _optim_hyper(betas, eps) -> None:
    if len(betas) != 2 or not all(isinstance(b, (int, float)) and not isinstance(b, bool) and 0.0 <= b < 1.0
                                  for b in betas):
        raise ValueError(f"optim: betas must be two floats in [0, 1), got {betas!r}")
    if isinstance(eps, bool) or not isinstance(eps, (int, float)) or not 0.0 <= eps < float("inf"):
        raise ValueError(f"optim: eps must be a non-negative finite float, got {eps!r}")


def _optim_max_norm(max_norm) -> float:
    if isinstance(max_norm, bool) or not isinstance(max_norm, (int, float)) or not 0.0 < max_norm < float("inf") \
            or not 0.0 < torch.tensor(float(max_norm), dtype=torch.float32).item() < float("inf"):
        raise ValueError(f"optim: max_norm must be a positive finite float, got {max_norm!r}")
    return float(max_norm)


def optim_sqsum(g, seg_off, seg_flags, partials, sums, bucket: int = 0, max_grid: int = 0):
    """The first two levels of the gradient norm of one bucket.  ``k_optim_sqsum`` writes the fp32
    sum of squares of every slot's gradients into ``partials[slot]`` (a fixed chain of 16 dependent
    additions; a spare slot writes 0); ``k_optim_sums``, one workgroup, adds the partials in fp64 in
    a fixed order into ``sums[0, bucket]`` (segments with ``OPTIM_SHARDED``) and ``sums[1, bucket]``
    (the rest); ``sums=None`` stops after the first level.  No atomics: two calls give the same bits.  Every buffer is passed in: the call
    allocates nothing, never synchronises with the host and can be captured in a graph.  Operands
    as ``optim_validate`` describes; returns ``sums``."""
    if seg_flags is None or partials is None:
        raise ValueError("optim: optim_sqsum needs seg_flags and partials")
    n, S = optim_validate(g, seg_off, None, seg_flags, partials=partials, sums=sums, bucket=bucket, max_grid=max_grid)
    es = 8
    _D().optim_sqsum(g.data_ptr(), g.dtype == torch.float32, seg_off.data_ptr(), seg_flags.data_ptr(), S, n,
                     partials.data_ptr(), 0 if sums is None else sums.data_ptr() + bucket * es,
                     0 if sums is None else sums.data_ptr() + (sums.stride(0) + bucket) * es, max_grid, _stream(g))
    return sums


def optim_clip(sums, max_norm: float, clip):
    """``clip [2]`` fp32 = ``(norm, coef)`` from the ``[2, buckets]`` fp64 sums of squares (row 0
    sharded, row 1 replicated): each row is added in bucket order, then the two totals; ``norm =
    float(sqrt(total))`` and ``coef = min(1, max_norm / (norm + 1e-6))`` in fp32, the formula of
    ``clip_grad_norm_``.  One thread (``k_optim_clip``); no allocation, no host synchronisation."""
    if not isinstance(clip, torch.Tensor):
        raise TypeError(f"optim: clip must be float32, got {type(clip).__name__}")
    _optim_sums_rules(sums, clip.device)
    _optim_small("clip", clip, torch.float32, (2,), sums.device)
    max_norm = _optim_max_norm(max_norm)
    _D().optim_clip(sums.data_ptr(), sums.data_ptr() + sums.stride(0) * sums.element_size(), sums.shape[1], max_norm,
                    clip.data_ptr(), _stream(sums))
    return clip


def optim_adamw_update(g, seg_off, seg_ptr, seg_flags, p32, m, v, sched, clip=None, betas=(0.9, 0.999),
                       eps: float = 1e-8, max_grid: int = 0):
    """One AdamW step of a bucket (``k_optim_adamw``), per element, every operation rounded once::

        g'  = g * coef                      (coef = clip[1]; skipped when clip is None)
        m'  = (b1 * m) + (omb1 * g')
        v'  = (b2 * v) + ((omb2 * g') * g')
        p1  = p * decay if the segment has OPTIM_DECAY else p
        p'  = p1 - lr * ((m' / bc1) / (sqrt(v' / bc2) + eps))

    ``(lr, bc1, bc2, decay) = sched`` (``optim_sched``) and ``coef`` are read on the device, so a
    captured graph of the call stays valid across steps.  A bf16 bucket keeps its master weights in
    ``p32`` and the parameters at ``seg_ptr`` get ``bf16(p')``; an fp32 bucket (``p32=None``) updates
    the parameters themselves.  ``m``, ``v`` (and ``p32``) are indexed like the bucket.  The
    gradients are not written.  No allocation, no host synchronisation.  ``adamw_reference`` is the
    mirror."""
    if seg_ptr is None or seg_flags is None or m is None or v is None or sched is None:
        raise ValueError("optim: optim_adamw_update needs seg_ptr, seg_flags, m, v and sched")
    if isinstance(g, torch.Tensor) and g.dtype == torch.bfloat16 and p32 is None:
        raise ValueError("optim: a bf16 bucket needs its fp32 master weights p32")
    n, S = optim_validate(g, seg_off, seg_ptr, seg_flags, p32, m, v, clip=clip, sched=sched, betas=betas, eps=eps,
                          max_grid=max_grid)
    _D().optim_adamw(g.data_ptr(), g.dtype == torch.float32, seg_off.data_ptr(), seg_ptr.data_ptr(),
                     seg_flags.data_ptr(), S, n, 0 if p32 is None else p32.data_ptr(), m.data_ptr(), v.data_ptr(),
                     0 if clip is None else clip.data_ptr(), sched.data_ptr(), float(betas[0]), float(betas[1]),
                     float(eps), max_grid, _stream(g))


def optim_sched(lr: float, betas, weight_decay: float, t: int):
    """What changes per step, as the kernel reads it: ``(lr, bc1, bc2, decay)`` with ``bc_i = 1 -
    b_i^t`` and ``decay = 1 - lr * weight_decay``, each computed in fp64 and rounded once to fp32;
    a CPU fp32 [4] tensor.  ``t >= 1`` is the number of the step."""
    t = int(t)
    if t < 1:
        raise ValueError(f"optim_sched: t counts from 1, got {t}")
    _optim_hyper(betas, 0.0)
    lr, wd = float(lr), float(weight_decay)
    if not (0.0 <= lr < float("inf")) or not (0.0 <= wd < float("inf")):
        raise ValueError(f"optim_sched: lr and weight_decay must be non-negative and finite, got {lr}, {wd}")
    vals = [lr, 1.0 - float(betas[0]) ** t, 1.0 - float(betas[1]) ** t, 1.0 - lr * wd]
    return torch.tensor(vals, dtype=torch.float64).to(torch.float32)


def adamw_reference(g, p, m, v, sched, coef=None, betas=(0.9, 0.999), eps: float = 1e-8, decays=True,
                    dtype=torch.float32):
    """The formula of ``optim_adamw_update`` in separate torch operations, in ``dtype``: returns
    ``(p', m', v')``.  ``g``, ``p``, ``m``, ``v`` are tensors of one shape (any dtype: cast to
    ``dtype`` first, which is exact for bf16 and fp32 inputs), ``sched`` the four values of
    ``optim_sched`` (a tensor of any float dtype, cast to ``dtype``: fp64 values stay exact in the
    fp64 mirror), ``coef`` a scalar or None (no clipping), ``decays`` a bool or a bool tensor of
    that shape.  ``dtype=torch.float32`` on the CPU rounds every operation once, exactly like the
    kernel: the bit-exact mirror (the constants are the kernel's: ``fl32(b)``, ``fl32(1 - b)``,
    ``fl32(eps)``).  ``dtype=torch.float64`` is the exact formula from the same fp32 constants."""
    def c(x):
        return torch.tensor(float(x), dtype=torch.float64).to(torch.float32).to(dtype)

    lr, bc1, bc2, decay = (torch.as_tensor(sched)[i].to(dtype) for i in range(4))
    b1, omb1, b2, omb2, e = c(betas[0]), c(1.0 - betas[0]), c(betas[1]), c(1.0 - betas[1]), c(eps)
    g, p, m, v = (x.to(dtype) for x in (g, p, m, v))
    if coef is not None:
        g = g * (coef.to(dtype) if isinstance(coef, torch.Tensor) else torch.tensor(float(coef), dtype=torch.float64).to(dtype))
    m = (b1 * m) + (omb1 * g)
    v = (b2 * v) + ((omb2 * g) * g)
    if isinstance(decays, torch.Tensor):
        p1 = torch.where(decays, p * decay, p)
    else:
        p1 = p * decay if decays else p
    # torch's vectorised fp32 sqrt on the CPU is not correctly rounded (about 0.7 % of arguments are
    # one ulp off); the fp64 root of an fp32 number, rounded to fp32, is
    vh = v / bc2
    root = torch.sqrt(vh) if dtype == torch.float64 else torch.sqrt(vh.double()).to(dtype)
    p = p1 - lr * ((m / bc1) / (root + e))
    return p, m, v


def grad_norm_reference(grads, sharded=None):
    """The gradient norm in fp64: ``grads`` is a list of tensors, ``sharded`` None or one bool per
    tensor.  Returns ``(norm, sharded_sum, replicated_sum)`` as Python floats, the sums of squares."""
    sh = rep = 0.0
    for i, t in enumerate(grads):
        s = float((t.detach().double() ** 2).sum().item())
        if sharded is not None and sharded[i]:
            sh += s
        else:
            rep += s
    return (sh + rep) ** 0.5, sh, rep
