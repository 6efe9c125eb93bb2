"""Every grouped expert GEMM, bit for bit, on framed views.

The recipe and the frames are those of tests/test_gpu_gemm_views.py (imported, not copied):
integer-valued bf16 operands, so the fp32 result is exact in any summation order and a bf16
output is one round-to-nearest-even of it; operands are views of NaN-filled buffers, outputs
views of buffers filled with the sentinel.  No tolerance anywhere: each output is compared
bitwise with a per-expert fp64 reference.

Rows belong to experts through ``counts`` (a device tensor, int32 and int64 alternating across
the forms) and ``cap``; ``LAYOUTS`` holds the count edges.  In every call the operand rows at or
past ``min(total, cap)`` hold NaN like the operand frames, and the output rows at or past it
must still hold the sentinel: ``_check`` runs on the ``[0, total)`` row slice of the output
view, so the untouched rows count as frame.

Each checker takes the op as a callable and a device and returns a list of failure strings,
one or more per failing form.  The GPU cases below pass the HIP ops and ``"cuda"``;
tests/test_grouped_views_checkers.py passes plain-torch emulations and mutants of them on the
CPU, which is the evidence that these checks fail on a subtly wrong kernel.
"""
from collections import namedtuple

import pytest
import torch

from test_gpu_gemm_views import (BF16, F32, SENTINEL, SWIGLU_R, _check, _frame_damage, _framed, _int_values,  # noqa: F401
                                 _ints, _out_frame, _place, _rmax, _seed, _untouched)

pytestmark = pytest.mark.gpu

NAN = float("nan")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# ---------------------------------------------------------------------------
# row layouts
# ---------------------------------------------------------------------------
_LIMIT = [1 if g % 7 else 0 for g in range(256)]
#  id -> (counts, cap)
LAYOUTS = {
    "one": ([130], 130),                                   # two row tiles, no spare row
    "mixed": ([0, 1, 127, -4, 129, 128, 7], 392 + 43),     # empty first, negative, offsets 1 / 128 / 257 / 385
    "overflow": ([100, 100, 100, 5], 250),                 # third truncated to 50 rows, fourth starts at cap
    "huge": ([1000], 70),                                  # one count larger than cap
    "limit": (_LIMIT, sum(_LIMIT) + 3),                    # the 256-expert scan
    "long": ([320, 256, 64], 640),                         # TN only: 5, 4 and 1 reduction tiles of 64 rows
}
K_GLDS = (64, 128, 192, 256)  # 1, 2, an odd and an even count of 64-deep steps, LDS-DMA loops
K_REGS = (8, 72, 136, 200)    # the same counts for the register-staged loops, each with a zero-filled tail
COLS = (8, 72, 264)           # one partial column tile, and three tiles with a partial last one


def _bounds(counts, cap):
    """``(first, end)`` rows of every expert: the prefix sum of ``max(c, 0)``, clamped to ``cap``."""
    out, at = [], 0
    for c in counts:
        a = min(at, cap)
        at += max(int(c), 0)
        out.append((a, min(at, cap)))
    return out


def _layout(name):
    counts, cap = LAYOUTS[name]
    bounds = _bounds(counts, cap)
    return counts, cap, bounds, bounds[-1][1]


def _cnt(counts, i, device):
    return torch.tensor(counts, dtype=torch.int32 if i % 2 == 0 else torch.int64, device=device)


def _rows(shape, R, gen, total, device):
    """Integer-valued bf16 rows; the rows at or past ``total`` hold NaN."""
    t = _ints(shape, R, gen)
    t[total:] = NAN
    return t.to(device)


def _place_w(w, how):
    """Weights ``[G, N, K]`` as the form wants them.  ``padded``: the window ``[:, :N, 8:8 + K]``
    of a NaN ``[G, N + 8, K + 16]`` buffer (row stride K + 16, expert stride (N + 8)(K + 16), NaN
    rows behind every expert).  ``tail``: tight, as rows of a flat NaN buffer with NaN rows right
    behind the last expert (behind every other expert lies the next one)."""
    if how == "tight":
        return w.contiguous()
    G, N, K = w.shape
    if how == "padded":
        buf = torch.full((G, N + 8, K + 16), NAN, dtype=w.dtype, device=w.device)
        v = buf[:, :N, 8:8 + K]
    else:
        buf = torch.full((3 + G * N + 64, K), NAN, dtype=w.dtype, device=w.device)
        v = buf[3:3 + G * N].view(G, N, K)
    v.copy_(w)
    return v


def _expert_cat(bounds, fn):
    """``fn(g, first, end)`` of every expert that has rows, joined along the rows."""
    return torch.cat([fn(g, a, b) for g, (a, b) in enumerate(bounds) if b > a])


def _check_rows(buf, out, total, ref64, tag):
    """``_check`` on the rows below ``total``: the rows at or past it count as frame."""
    return _check(buf, out[:total], ref64, tag)


def _fail(errs):
    assert not errs, f"{len(errs)} failures:\n" + "\n".join(errs)


# ---------------------------------------------------------------------------
# grouped_gemm_nt
# ---------------------------------------------------------------------------
# out dtype, alpha, bias dtype, x placement, w placement, given (False: out=None with out_dtype)
NtForm = namedtuple("NtForm", "id out alpha bias x w given", defaults=(F32, 1.0, None, "tight", "tight", True))
NT_FORMS = [
    NtForm("f32"),
    NtForm("bf16", out=BF16),
    NtForm("f32-half-biasf32", alpha=0.5, bias=F32),
    NtForm("f32-biasbf16", bias=BF16),
    NtForm("bf16-half-biasbf16", out=BF16, alpha=0.5, bias=BF16),
    NtForm("bf16-biasf32", out=BF16, bias=F32),
    NtForm("bf16-half", out=BF16, alpha=0.5),
    NtForm("bf16-windowX-paddedW", out=BF16, x="window", w="padded"),
    NtForm("f32-half-rowsX-paddedW", alpha=0.5, x="rows", w="padded"),
    NtForm("f32-none", given=False),
    NtForm("bf16-none-half-biasf32", out=BF16, alpha=0.5, bias=F32, given=False),
]


def _layout_cases(layouts, cols, full):
    """``full`` runs every K of both loops; the other layouts run one K of each."""
    return [pytest.param(lay, n, k, id=f"{lay}-{n}-{k}") for lay in layouts for n in cols
            for k in (K_GLDS + K_REGS if lay == full else (128, 72))]


NT_CASES = _layout_cases(("mixed", "one", "overflow", "huge", "limit"), COLS, "mixed")


def _run_nt_forms(op, layout, N, K, forms, device, seed=0):
    counts, cap, bounds, total = _layout(layout)
    G = len(counts)
    gen = _seed(N, K, cap, G, seed)
    R = _rmax(K)
    x = _rows((cap, K), R, gen, total, device)
    w = _ints((G, N, K), R, gen).to(device)
    bias = _ints((G, N), 64, gen).to(device)
    P = _expert_cat(bounds, lambda g, a, b: x[a:b].double() @ w[g].double().T)
    B = _expert_cat(bounds, lambda g, a, b: bias[g].double().expand(b - a, N))
    errs = []
    for i, f in enumerate(forms):
        xv, wv = _place(x, f.x), _place_w(w, f.w)
        ref = f.alpha * P
        bias_t = None
        if f.bias is not None:
            bias_t = bias.to(f.bias).contiguous()
            ref = ref + B
        cnt = _cnt(counts, i, device)
        if f.given:
            buf, out = _out_frame(cap, N, f.out, device=device)
            y = op(xv, wv, cnt, out=out, bias=bias_t, alpha=f.alpha)
            if y is not out:
                errs.append(f"{f.id}: the op did not return its output")
            errs += _check_rows(buf, out, total, ref, f.id)
        else:  # rows at or past the total are uninitialised
            y = op(xv, wv, cnt, bias=bias_t, alpha=f.alpha, out_dtype=f.out)
            if y.shape != (cap, N) or y.dtype != f.out:
                errs.append(f"{f.id}: got {tuple(y.shape)} {y.dtype}")
                continue
            errs += _check(y[:total], y[:total], ref, f.id)
    return errs


@pytest.mark.parametrize("layout,N,K", NT_CASES)
def test_grouped_nt(layout, N, K):
    from collective_communication_mpi_amd.ops import grouped_gemm_nt

    _fail(_run_nt_forms(grouped_gemm_nt, layout, N, K, NT_FORMS, "cuda"))


# ---------------------------------------------------------------------------
# grouped_gemm_nt_swiglu: h exact, the gate bit for bit what swiglu_pairs makes of that h
# ---------------------------------------------------------------------------
GluForm = namedtuple("GluForm", "id alpha bias x w", defaults=(1.0, None, "tight", "tight"))
GLU_FORMS = [
    GluForm("plain"),
    GluForm("half-biasf32", alpha=0.5, bias=F32),
    GluForm("windowX-paddedW", x="window", w="padded"),
]
GLU_K = (64, 128, 192, 72, 136)  # the last two: the register loop, which the dense fused gate does not have
GLU_CASES = [pytest.param(lay, n, k, id=f"{lay}-{n}-{k}") for lay in ("mixed", "overflow") for n in (136, 264)
             for k in GLU_K]


def _run_swiglu_forms(op, gate, layout, N, K, forms, device, seed=0):
    """``op`` returns ``(h, glu)``; ``gate`` is the unfused ``swiglu_pairs``."""
    counts, cap, bounds, total = _layout(layout)
    G = len(counts)
    gen = _seed(N, K, cap, G, seed, 1)
    x = _rows((cap, K), SWIGLU_R, gen, total, device)
    w = _ints((G, N, K), SWIGLU_R, gen).to(device)
    bias = _ints((G, N), SWIGLU_R, gen).to(device)
    P = _expert_cat(bounds, lambda g, a, b: x[a:b].double() @ w[g].double().T)
    B = _expert_cat(bounds, lambda g, a, b: bias[g].double().expand(b - a, N))
    errs = []
    for i, f in enumerate(forms):
        xv, wv = _place(x, f.x), _place_w(w, f.w)
        ref = f.alpha * P
        bias_t = None
        if f.bias is not None:
            bias_t = bias.to(f.bias).contiguous()
            ref = ref + B
        hbuf, h = _out_frame(cap, N, BF16, device=device)
        gbuf, glu = _out_frame(cap, N // 2, BF16, col_off=4, device=device)  # 8-B aligned, row stride > N / 2
        hh, gg = op(xv, wv, _cnt(counts, i, device), h=h, glu=glu, bias=bias_t, alpha=f.alpha)
        if hh is not h or gg is not glu:
            errs.append(f"{f.id}: the op did not return its outputs")
        errs += _check_rows(hbuf, h, total, ref, f"{f.id} h")
        got = glu[:total]
        bad = _frame_damage(gbuf, got)
        if bad:
            errs.append(f"{f.id} glu: {bad} cells of the output frame were overwritten")
        if bool(torch.isnan(got.float()).any()):
            errs.append(f"{f.id} glu: NaN in the output")
        want = gate(h[:total])  # the unfused gate on the very h the kernel wrote
        ne = got.contiguous().view(torch.int16) != want.contiguous().view(torch.int16)
        if bool(ne.any()):  # report both against an fp64 gate of the bf16 h
            hd = h[:total].double()
            exact = hd[:, 0::2] * torch.sigmoid(hd[:, 0::2]) * hd[:, 1::2]
            e_fused = float((got.double() - exact).abs().max())
            e_unfused = float((want.double() - exact).abs().max())
            r, c = [int(v) for v in ne.nonzero()[0]]
            errs.append(f"{f.id} glu: {int(ne.sum())} of {ne.numel()} values differ from swiglu_pairs(h); first at "
                        f"({r}, {c}): fused {float(got[r, c])!r}, unfused {float(want[r, c])!r}, fp64 "
                        f"{float(exact[r, c])!r}; max error fused {e_fused:.6g}, unfused {e_unfused:.6g}")
    return errs


@pytest.mark.parametrize("layout,N,K", GLU_CASES)
def test_grouped_nt_swiglu(layout, N, K):
    from collective_communication_mpi_amd.ops import grouped_gemm_nt_swiglu, swiglu_pairs

    _fail(_run_swiglu_forms(grouped_gemm_nt_swiglu, swiglu_pairs, layout, N, K, GLU_FORMS, "cuda"))


# ---------------------------------------------------------------------------
# grouped_gemm_nn: out[r] = alpha * dy[r] @ w[g]; the reduction runs over N, the columns are K
# ---------------------------------------------------------------------------
# route "nn": the op on w as it lies; "nt": the forward op on the transposed copy of every expert
NnForm = namedtuple("NnForm", "id out alpha dy w route", defaults=(F32, 1.0, "tight", "tight", "nn"))
NN_FORMS = [
    NnForm("f32"),
    NnForm("bf16", out=BF16),
    NnForm("f32-half", alpha=0.5),
    NnForm("bf16-half", out=BF16, alpha=0.5),
    NnForm("bf16-windowDy-paddedW", out=BF16, dy="window", w="padded"),
    NnForm("f32-rowsDy-tailW", dy="rows", w="tail"),
    NnForm("bf16-half-rowsDy-tailW", out=BF16, alpha=0.5, dy="rows", w="tail"),
    NnForm("transposed-bf16", out=BF16, route="nt"),
    NnForm("transposed-f32-half-windowDy", alpha=0.5, dy="window", route="nt"),
]
# (layout, reduction N, columns K)
NN_CASES = [pytest.param(lay, n, k, id=f"{lay}-N{n}-K{k}") for lay in ("mixed", "one", "overflow", "huge", "limit")
            for k in COLS for n in (K_GLDS + K_REGS if lay == "mixed" else (128, 72))]


def _run_nn_forms(op, nt_op, transposed, layout, N, K, forms, device, seed=0):
    """``nt_op`` and ``transposed`` (``[G, N, K]`` -> the ``[G, K, N]`` view of one transposed
    copy) make the transposed-copy route; it runs on the same data against the same reference."""
    counts, cap, bounds, total = _layout(layout)
    G = len(counts)
    gen = _seed(N, K, cap, G, seed, 2)
    R = _rmax(N)
    dy = _rows((cap, N), R, gen, total, device)
    w = _ints((G, N, K), R, gen).to(device)
    P = _expert_cat(bounds, lambda g, a, b: dy[a:b].double() @ w[g].double())
    errs = []
    for i, f in enumerate(forms):
        dv = _place(dy, f.dy)
        buf, out = _out_frame(cap, K, f.out, device=device)
        cnt = _cnt(counts, i, device)
        if f.route == "nn":
            y = op(dv, _place_w(w, f.w), cnt, out=out, alpha=f.alpha)
        else:
            y = nt_op(dv, transposed(w), cnt, out=out, alpha=f.alpha)
        if y is not out:
            errs.append(f"{f.id}: the op did not return its output")
        errs += _check_rows(buf, out, total, f.alpha * P, f.id)
    return errs


@pytest.mark.parametrize("layout,N,K", NN_CASES)
def test_grouped_nn(layout, N, K):
    from collective_communication_mpi_amd.ops import grouped_gemm_nn, grouped_gemm_nt
    from collective_communication_mpi_amd.ops.kernels import _transposed_experts

    _fail(_run_nn_forms(grouped_gemm_nn, grouped_gemm_nt, _transposed_experts, layout, N, K, NN_FORMS, "cuda"))


# ---------------------------------------------------------------------------
# grouped_gemm_tn: out[g] = alpha * dy[rows of g].T @ x[rows of g], fp32 [G, N, K]
# ---------------------------------------------------------------------------
# c "window": the output is a window of a sentinel [G, N + 2, 4 + K + 8] buffer at column 4: a
# padded row stride and a padded expert stride
TnForm = namedtuple("TnForm", "id alpha dy x c", defaults=(1.0, "tight", "tight", "tight"))
TN_FORMS = [
    TnForm("plain"),
    TnForm("half", alpha=0.5),
    TnForm("windows", dy="window", x="window"),
    TnForm("outwindow", c="window"),
    TnForm("half-rowsDy-windowX-outwindow", alpha=0.5, dy="rows", x="window", c="window"),
]
TN_SHAPES = [(8, 8), (136, 72), (264, 136)]
TN_LAYOUTS = ("mixed", "long", "overflow", "huge", "limit")
TN_CASES = [pytest.param(lay, n, k, id=f"{lay}-{n}x{k}") for lay in TN_LAYOUTS for (n, k) in TN_SHAPES]


def _dw_frame(G, N, K, how, device):
    if how == "tight":
        buf = torch.full((G, N, K), SENTINEL, dtype=F32, device=device)
        return buf, buf
    buf = torch.full((G, N + 2, 4 + K + 8), SENTINEL, dtype=F32, device=device)
    return buf, buf[:, 1:N + 1, 4:4 + K]


def _check_dw(buf, out, ref64, tag):
    """``_check`` of a ``[G, N, K]`` output with its experts stacked; the frame is what ``buf``
    holds outside the window."""
    G, N, K = out.shape
    errs = []
    if out is not buf:
        chk = buf.clone()
        chk[:, 1:N + 1, 4:4 + K] = SENTINEL
        bad = int((chk != SENTINEL).sum())
        if bad:
            errs.append(f"{tag}: {bad} cells of the output frame were overwritten")
    flat = out.contiguous().view(G * N, K)
    return errs + _check(flat, flat, ref64.reshape(G * N, K), tag)


def _run_tn_forms(op, layout, N, K, forms, device, seed=0):
    """An expert with no rows must be exactly +0 over its whole block: the reference holds +0
    there and the comparison is bitwise."""
    counts, cap, bounds, total = _layout(layout)
    G = len(counts)
    gen = _seed(N, K, cap, G, seed, 3)
    R = _rmax(max(counts))
    dy = _rows((cap, N), R, gen, total, device)
    x = _rows((cap, K), R, gen, total, device)
    P = torch.stack([dy[a:b].double().T @ x[a:b].double() for (a, b) in bounds])
    errs = []
    for i, f in enumerate(forms):
        buf, out = _dw_frame(G, N, K, f.c, device)
        y = op(_place(dy, f.dy), _place(x, f.x), _cnt(counts, i, device), out=out, alpha=f.alpha)
        if y is not out:
            errs.append(f"{f.id}: the op did not return its output")
        errs += _check_dw(buf, out, f.alpha * P, f.id)
    return errs


@pytest.mark.parametrize("layout,N,K", TN_CASES)
def test_grouped_tn(layout, N, K):
    from collective_communication_mpi_amd.ops import grouped_gemm_tn

    _fail(_run_tn_forms(grouped_gemm_tn, layout, N, K, TN_FORMS, "cuda"))


# ---------------------------------------------------------------------------
# grouped_linear: forward, dX by both routes and dW, bf16 weights and fp32 master weights
# ---------------------------------------------------------------------------
LINEAR_SHAPES = [(136, 128), (72, 72)]  # (N, K): LDS-DMA loops both ways; register loops both ways


def _linear_r(N, K):
    counts, cap, bounds, _ = _layout("mixed")
    return min(_rmax(K), _rmax(N), _rmax(max(b - a for a, b in bounds)))


def _run_linear(linear, N, K, w_dtype, device, seed=0):
    """``y``, ``x.grad`` and ``w.grad`` of ``linear(x, w, counts)`` on ``mixed`` for the rows below
    the total.  The incoming gradient is a column window that starts one element in (2 B off a
    16-B boundary), which ``grouped_grad_rows`` has to copy."""
    counts, cap, bounds, total = _layout("mixed")
    G = len(counts)
    gen = _seed(N, K, cap, G, seed, 4)
    R = _linear_r(N, K)
    x = _rows((cap, K), R, gen, total, device).requires_grad_()
    w = _ints((G, N, K), R, gen).to(w_dtype).to(device).requires_grad_()
    gbuf = torch.full((cap, N + 8), NAN, dtype=BF16, device=device)
    dy = gbuf[:, 1:1 + N]
    dy[:total] = _ints((total, N), R, gen).to(device)
    xd, wd, dd = x.detach().double(), w.detach().double(), dy.double()
    y = linear(x, w, _cnt(counts, seed, device))
    y.backward(dy)
    errs = []
    if y.dtype != BF16 or x.grad.dtype != BF16 or w.grad.dtype != w_dtype:
        errs.append(f"dtypes: y {y.dtype}, x.grad {x.grad.dtype}, w.grad {w.grad.dtype}")
        return errs
    yv, dx = y.detach()[:total], x.grad[:total]
    errs += _check(yv, yv, _expert_cat(bounds, lambda g, a, b: xd[a:b] @ wd[g].T), "y")
    errs += _check(dx, dx, _expert_cat(bounds, lambda g, a, b: dd[a:b] @ wd[g]), "x.grad")
    dw = w.grad.view(G * N, K)  # fp32 weights: the exact product; bf16 weights: one rounding of it
    errs += _check(dw, dw, torch.cat([dd[a:b].T @ xd[a:b] for (a, b) in bounds]), "w.grad")
    return errs


@pytest.mark.parametrize("w_dtype", [BF16, F32], ids=["wbf16", "wf32"])
@pytest.mark.parametrize("route", ["nn", "transpose"])
@pytest.mark.parametrize("N,K", LINEAR_SHAPES)
def test_grouped_linear(monkeypatch, N, K, route, w_dtype):
    from collective_communication_mpi_amd.ops import grouped_dx_route, grouped_linear

    monkeypatch.setenv("CCMPI_GROUPED_DX", route)
    assert grouped_dx_route() == route
    _fail(_run_linear(grouped_linear, N, K, w_dtype, "cuda", seed=len(route)))


# ---------------------------------------------------------------------------
# refusals: ValueError (TypeError for a dtype), nothing launched, nothing written
# ---------------------------------------------------------------------------
Refusal = namedtuple("Refusal", "tag op exc args kwargs bufs")


def _shifted(t, col_off, col_pad, before=3):
    _, v = _framed(t.shape[0], t.shape[1], t.dtype, NAN, before, 3, col_off, col_pad, device=t.device)
    v.copy_(t)
    return v


def _refusals(device):
    """Every refused call of the issue's list: operands that break one rule each (asserted here),
    outputs in sentinel buffers."""
    counts, cap, N, K = [60, 70], 130, 72, 64
    G = len(counts)
    gen = _seed(cap, N, K, 77)
    x = _ints((cap, K), SWIGLU_R, gen).to(device)
    dy = _ints((cap, N), SWIGLU_R, gen).to(device)
    w = _ints((G, N, K), SWIGLU_R, gen).to(device)
    cnt = torch.tensor(counts, dtype=torch.int32, device=device)
    cnt_strided = torch.tensor([60, 0, 70, 0], dtype=torch.int32, device=device)[::2]
    cnt_float = torch.tensor(counts, dtype=F32, device=device)
    assert not cnt_strided.is_contiguous() and cnt_strided.tolist() == counts
    out = []

    def outs(op, how="aligned"):
        """kwargs with fresh sentinel outputs of ``op``, and their buffers"""
        if op == "nt":
            buf, o = _out_frame(cap, N, F32, how, device=device)
            return {"out": o}, [buf]
        if op == "nn":
            buf, o = _out_frame(cap, K, BF16, how, device=device)
            return {"out": o}, [buf]
        if op == "tn":
            buf, o = _dw_frame(G, N, K, "window", device)
            return {"out": o}, [buf]
        hbuf, h = _out_frame(cap, N, BF16, how, device=device)
        gbuf, glu = _out_frame(cap, N // 2, BF16, col_off=4, device=device)
        return {"h": h, "glu": glu}, [hbuf, gbuf]

    def add(tag, op, exc, args, kw=None, bufs=None, **more):
        if kw is None:
            kw, bufs = outs(op)
        out.append(Refusal(f"{op}: {tag}", op, exc, args, {**kw, **more}, bufs))

    firsts = {"nt": (x, w), "swiglu": (x, w), "nn": (dy, w), "tn": (dy, x)}
    for op, (a, b) in firsts.items():
        off8, ld4 = _shifted(a, 4, 4), _shifted(a, 0, 4, 4)
        assert off8.data_ptr() % 16 == 8 and off8.stride(0) % 8 == 0
        assert ld4.data_ptr() % 16 == 0 and ld4.stride(0) % 8 == 4
        add("first operand 8 B off", op, ValueError, (off8, b, cnt))
        add("first operand's row stride % 8", op, ValueError, (ld4, b, cnt))
        add("non-contiguous counts", op, ValueError, (a, b, cnt_strided))
        add("float counts", op, TypeError, (a, b, cnt_float))
        if op != "tn":
            kw, bufs = outs(op, "oddld")
            o = kw["h" if op == "swiglu" else "out"]
            assert o.data_ptr() % 16 == 0 and (o.stride(0) * o.element_size()) % 16
            add("output rows not 16-B aligned", op, ValueError, (a, b, cnt), kw, bufs)

    # w: an expert stride that is no multiple of 8; for nn, rows closer together than their K columns
    wbuf = torch.zeros(G * (N * K + 4), dtype=BF16, device=device)
    w_gs = torch.as_strided(wbuf, (G, N, K), (N * K + 4, K, 1))
    w_short = torch.as_strided(wbuf, (G, N, K), (N * K, K - 8, 1))
    assert w_gs.data_ptr() % 16 == 0 and w_gs.stride(0) % 8 == 4 and w_short.stride(1) % 8 == 0
    add("w expert stride % 8", "nt", ValueError, (x, w_gs, cnt))
    add("w expert stride % 8", "nn", ValueError, (dy, w_gs, cnt))
    add("w row stride < K", "nn", ValueError, (dy, w_short, cnt))
    bias = torch.zeros((G, 2 * N), dtype=F32, device=device)[:, ::2]
    assert bias.shape == (G, N) and not bias.is_contiguous()
    add("non-contiguous bias", "nt", ValueError, (x, w, cnt), bias=bias)

    # the gate's output
    def glu_case(tag, gbuf, glu):
        hbuf, h = _out_frame(cap, N, BF16, device=device)
        add(tag, "swiglu", ValueError, (x, w, cnt), {"h": h, "glu": glu}, [hbuf, gbuf])

    gbuf, glu = _out_frame(cap, N // 2, BF16, col_off=1, device=device)
    assert glu.data_ptr() % 8 == 2
    glu_case("glu 2 B off", gbuf, glu)
    gbuf, glu = _framed(cap, N // 2, BF16, SENTINEL, 4, 3, 4, 10, device=device)
    assert glu.data_ptr() % 8 == 0 and glu.stride(0) % 4 == 2
    glu_case("glu row stride % 4", gbuf, glu)
    gbuf = torch.full((cap * (N // 2),), SENTINEL, dtype=BF16, device=device)
    glu = torch.as_strided(gbuf, (cap, N // 2), (N // 2 - 4, 1))
    assert glu.data_ptr() % 8 == 0 and glu.stride(0) % 4 == 0
    glu_case("glu row stride < N / 2", gbuf, glu)

    # the weight gradient: the second operand, the output's strides, N % 8
    off8 = _shifted(x, 4, 4)
    assert off8.data_ptr() % 16 == 8 and off8.stride(0) % 8 == 0
    add("x 8 B off", "tn", ValueError, (dy, off8, cnt))
    buf = torch.full((G, N, K + 2), SENTINEL, dtype=F32, device=device)
    o = buf[:, :, :K]
    assert o.data_ptr() % 16 == 0 and o.stride(1) % 4 == 2 and o.stride(0) % 4 == 0
    add("output row stride % 4", "tn", ValueError, (dy, x, cnt), {"out": o}, [buf])
    buf = torch.full((G * (N * K + 2),), SENTINEL, dtype=F32, device=device)
    o = torch.as_strided(buf, (G, N, K), (N * K + 2, K, 1))
    assert o.data_ptr() % 16 == 0 and o.stride(1) % 4 == 0 and o.stride(0) % 4 == 2
    add("output expert stride % 4", "tn", ValueError, (dy, x, cnt), {"out": o}, [buf])
    dy12 = _place(dy[:, :12], "rows")  # 12 columns of 24: only N breaks a rule
    assert dy12.data_ptr() % 16 == 0 and dy12.stride(0) % 8 == 0
    buf = torch.full((G, 12, K), SENTINEL, dtype=F32, device=device)
    add("N % 8", "tn", ValueError, (dy12, x, cnt), {"out": buf}, [buf])
    return out


def _run_refusals(ops, device):
    """``ops``: name -> callable for ``nt``, ``swiglu``, ``nn``, ``tn``."""
    errs = []
    for r in _refusals(device):
        try:
            ops[r.op](*r.args, **r.kwargs)
            errs.append(f"{r.tag}: not refused")
        except (ValueError, TypeError) as e:
            if type(e) is not r.exc:
                errs.append(f"{r.tag}: raised {type(e).__name__}, expected {r.exc.__name__}")
        for b in r.bufs:
            errs += _untouched(b, r.tag)
    return errs


def test_grouped_refusals():
    from collective_communication_mpi_amd import ops

    _fail(_run_refusals({"nt": ops.grouped_gemm_nt, "swiglu": ops.grouped_gemm_nt_swiglu, "nn": ops.grouped_gemm_nn,
                         "tn": ops.grouped_gemm_tn}, "cuda"))


# every (K, R) of this module whose output is rounded to bf16, and the reduction lengths of the
# weight gradient (the experts' row counts; fp32 outputs), for the CPU recipe test
RECIPE_KR = sorted({(k, _rmax(k)) for k in K_GLDS + K_REGS} | {(k, SWIGLU_R) for k in GLU_K}
                   | {(k, _linear_r(n, k)) for (n, k) in LINEAR_SHAPES} | {(n, _linear_r(n, k)) for (n, k) in LINEAR_SHAPES})
RECIPE_TN_RED = sorted({(b - a, _rmax(max(LAYOUTS[lay][0]))) for lay in TN_LAYOUTS
                        for (a, b) in _bounds(*LAYOUTS[lay]) if b > a})
