"""RMSNorm with the residual add in front of it on the GPU (``ops.rms_norm*`` / ``ops.add_rms_norm*``,
csrc/device/rmsnorm.hip).

Accuracy, forward, against ``ops.rms_norm_reference`` (fp64) on the same bf16 inputs: ``h`` is
torch's ``x + residual`` bit for bit; ``|y - exact| <= (2^-8 + 2^-16) |exact|`` -- bf16's unit
roundoff for the single rounding, and ``2^-16`` for a sum of at most 128 dependent fp32 additions
of positive terms (relative ``2^-17``), halved by the square root, plus the root, the division and
two products, with more than a factor of two to spare; ``|rstd - exact| <= 2^-16 |exact|``.
Accuracy, backward, against ``ops.rms_norm_backward_reference`` on the kernel's own ``h``, with
``n = h rstd`` and ``g = dy w``: ``|dh - exact| <= 2^-8 |exact| + 2^-16 rstd (|g_j| + |n_j| mean_k
|g_k n_k|) + 2^-22 |dres_j|`` and ``|dw_j - exact| <= 2^-16 sum_t |dy[t, j] n[t, j]|`` (fewer than
256 dependent additions in every shape used here), plus ``2^-8 |exact|`` after the autograd form's
cast to a bf16 weight.
Bitwise contracts, framed views, 64-bit row strides, the adjoint, graph replay and refusals
follow, then the model."""
import functools

import pytest
import torch

from collective_communication_mpi_amd import _native, ops

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
F32 = torch.float32
EPS = 1e-5
SENTINEL = -7.0
DIMS = (8, 64, 136, 4096, 16384)  # 136: 17 slices, fewer than a wave has lanes; 4096: the model's; 16384: 8 slices per thread
CHUNK = ops.rms_norm_row_chunk(1, 8)  # rows per workgroup of the backward at every T below
LENGTHS = (1, 3, CHUNK - 1, CHUNK + 1, 257)
WEIGHTS = {"bf16": BF, "fp32": F32}


def _randn(*shape, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(*shape, device="cuda", generator=g).to(BF)


@functools.lru_cache(maxsize=None)
def _rows(T, d, salt):
    """[T, d] bf16; shared between tests and never written."""
    return _randn(T, d, seed=11 + 1000003 * salt + 131 * T + d)


@functools.lru_cache(maxsize=None)
def _weight(d, dtype):
    g = torch.Generator(device="cuda").manual_seed(5 + d)
    return (0.5 + torch.rand(d, device="cuda", generator=g)).to(dtype)  # random: all ones would hide a wrong column


def _inputs(T, d):
    return tuple(_rows(T, d, salt) for salt in range(4))  # x, residual, dy, dres


def _worst(err, tol):
    return (err / tol.clamp_min(1e-300)).max().item()


def _forward_ratios(x, r, w, h, y, rstd, eps=EPS):
    eh, ey, er = ops.rms_norm_reference(x, w, eps, r)
    assert torch.equal(h, eh), "h is not torch's bf16 x + residual"
    ry = _worst((y.double() - ey).abs(), (2.0 ** -8 + 2.0 ** -16) * ey.abs())
    rr = _worst((rstd.double() - er).abs(), 2.0 ** -16 * er)
    return ry, rr


def _backward_bounds(dy, h, w, dres, eps=EPS):
    """(exact dh, exact dw, tolerance of dh, tolerance of the fp32 dw)."""
    dh, dw = ops.rms_norm_backward_reference(dy, h, w, eps, dres)
    hd = h.double()
    rstd = 1.0 / torch.sqrt((hd * hd).mean(dim=1, keepdim=True) + eps)
    n, g = hd * rstd, dy.double() * w.double()[None, :]
    tol_dh = 2.0 ** -8 * dh.abs() + 2.0 ** -16 * rstd * (g.abs() + n.abs() * (g * n).abs().mean(dim=1, keepdim=True))
    if dres is not None:
        tol_dh = tol_dh + 2.0 ** -22 * dres.double().abs()
    return dh, dw, tol_dh, 2.0 ** -16 * (dy.double() * n).abs().sum(dim=0)


# --- accuracy ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("wname", sorted(WEIGHTS))
@pytest.mark.parametrize("d", DIMS)
def test_forward_accuracy_and_h_is_torchs_sum(d, wname):
    w = _weight(d, WEIGHTS[wname])
    worst_y = worst_r = 0.0
    for T in LENGTHS:
        x, r, _, _ = _inputs(T, d)
        y, rstd = ops.rms_norm_forward(x, w, EPS)
        assert y.shape == (T, d) and y.dtype == BF and y.is_contiguous() and rstd.shape == (T,) and rstd.dtype == F32
        ry, rr = _forward_ratios(x, None, w, x, y, rstd)
        h, y2, rstd2 = ops.add_rms_norm_forward(x, r, w, EPS)
        assert h.is_contiguous() and y2.is_contiguous()
        ry2, rr2 = _forward_ratios(x, r, w, h, y2, rstd2)
        worst_y, worst_r = max(worst_y, ry, ry2), max(worst_r, rr, rr2)
        assert max(ry, ry2) <= 1.0 and max(rr, rr2) <= 1.0, f"T={T}: y {max(ry, ry2):.3f}, rstd {max(rr, rr2):.3f} x the tolerance"
    print(f"[rms_norm forward d={d} weight={wname}] worst error / tolerance: y {worst_y:.3f} rstd {worst_r:.3f}")


@pytest.mark.parametrize("wname", sorted(WEIGHTS))
def test_forward_accuracy_of_tiny_and_large_rows(wname):
    """Rows scaled by 2^-20 (mean h^2 ~ 2^-40: eps decides rstd) and by 2^10 (nothing overflows)."""
    T, d = CHUNK + 1, 136
    w = _weight(d, WEIGHTS[wname])
    x, r, dy, dres = _inputs(T, d)
    scale = torch.where(torch.arange(T, device="cuda") % 2 == 0, 2.0 ** -20, 2.0 ** 10)[:, None]
    xs, rs = (x.float() * scale).to(BF), (r.float() * scale).to(BF)  # powers of two: exact
    h, y, rstd = ops.add_rms_norm_forward(xs, rs, w, EPS)
    assert torch.isfinite(y.float()).all() and torch.isfinite(rstd).all()
    ry, rr = _forward_ratios(xs, rs, w, h, y, rstd)
    assert (rstd[0::2] > 300).all() and (rstd[1::2] < 2.0 ** -9).all()  # 1 / sqrt(eps) = 316
    dh, dw = ops.rms_norm_backward(dy, h, w, rstd, dres)
    edh, edw, tol_dh, tol_dw = _backward_bounds(dy, h, w, dres)
    rdh, rdw = _worst((dh.double() - edh).abs(), tol_dh), _worst((dw.double() - edw).abs(), tol_dw)
    print(f"[rms_norm scaled rows weight={wname}] worst error / tolerance: y {ry:.3f} rstd {rr:.3f} dh {rdh:.3f} dw {rdw:.3f}")
    assert max(ry, rr, rdh, rdw) <= 1.0


@pytest.mark.parametrize("wname", sorted(WEIGHTS))
@pytest.mark.parametrize("d", DIMS)
def test_backward_accuracy(d, wname):
    w = _weight(d, WEIGHTS[wname])
    worst_dh = worst_dw = 0.0
    for T in LENGTHS:
        x, r, dy, dres = _inputs(T, d)
        h, _, rstd = ops.add_rms_norm_forward(x, r, w, EPS)
        for dr in (None, dres):
            dh, dw = ops.rms_norm_backward(dy, h, w, rstd, dr)
            assert dh.shape == (T, d) and dh.dtype == BF and dh.is_contiguous() and dw.shape == (d,) and dw.dtype == F32
            edh, edw, tol_dh, tol_dw = _backward_bounds(dy, h, w, dr)
            rdh, rdw = _worst((dh.double() - edh).abs(), tol_dh), _worst((dw.double() - edw).abs(), tol_dw)
            worst_dh, worst_dw = max(worst_dh, rdh), max(worst_dw, rdw)
            assert rdh <= 1.0 and rdw <= 1.0, f"T={T} dres={'yes' if dr is not None else 'no'}: dh {rdh:.3f}, dw {rdw:.3f} x the tolerance"
    print(f"[rms_norm backward d={d} weight={wname}] worst error / tolerance: dh {worst_dh:.3f} dw {worst_dw:.3f}")


def test_backward_accuracy_where_the_row_chunk_grows():
    """T = 9000: chunks of 9 rows, 1000 partials, 32 per lane of the second kernel -- 73 dependent
    additions per column, inside the 2^-16 of the bound."""
    T, d = 9000, 64
    assert ops.rms_norm_row_chunk(T, d) == 9
    w = _weight(d, F32)
    x, _, dy, dres = _inputs(T, d)
    y, rstd = ops.rms_norm_forward(x, w, EPS)
    dh, dw = ops.rms_norm_backward(dy, x, w, rstd, dres)
    edh, edw, tol_dh, tol_dw = _backward_bounds(dy, x, w, dres)
    rdh, rdw = _worst((dh.double() - edh).abs(), tol_dh), _worst((dw.double() - edw).abs(), tol_dw)
    print(f"[rms_norm backward T={T} d={d}] worst error / tolerance: dh {rdh:.3f} dw {rdw:.3f}")
    assert rdh <= 1.0 and rdw <= 1.0


# --- bitwise contracts -----------------------------------------------------------------------------------

@pytest.mark.parametrize("wname", sorted(WEIGHTS))
@pytest.mark.parametrize("d", DIMS)
def test_bitwise_contracts(d, wname):
    T = 257
    w = _weight(d, WEIGHTS[wname])
    x, r, dy, dres = _inputs(T, d)
    h, y, rstd = ops.add_rms_norm_forward(x, r, w, EPS)
    dh, dw = ops.rms_norm_backward(dy, h, w, rstd, dres)
    same = lambda a, b: all(torch.equal(p, q) for p, q in zip(a, b))
    # two calls agree, dw included
    assert same(ops.add_rms_norm_forward(x, r, w, EPS), (h, y, rstd))
    assert same(ops.rms_norm_backward(dy, h, w, rstd, dres), (dh, dw))
    # the fused add is the add
    assert same(ops.rms_norm_forward(x + r, w, EPS), (y, rstd))
    # a row alone, as a T = 1 view
    for t in (0, CHUNK, T - 1):
        h1, y1, rstd1 = ops.add_rms_norm_forward(x[t:t + 1], r[t:t + 1], w, EPS)
        dh1, _ = ops.rms_norm_backward(dy[t:t + 1], h[t:t + 1], w, rstd[t:t + 1], dres[t:t + 1], need_dw=False)
        assert same((h1, y1, rstd1, dh1), (h[t:t + 1], y[t:t + 1], rstd[t:t + 1], dh[t:t + 1])), f"row {t} alone"
    # a row-permuted batch
    perm = torch.randperm(T, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    hp, yp, rstdp = ops.add_rms_norm_forward(x[perm], r[perm], w, EPS)
    dhp, _ = ops.rms_norm_backward(dy[perm], hp, w, rstdp, dres[perm], need_dw=False)
    assert same((hp, yp, rstdp, dhp), (h[perm], y[perm], rstd[perm], dh[perm])), "rows depend on their neighbours"
    # dres = 0 gives the bits of dres = None
    dh0, dw0 = ops.rms_norm_backward(dy, h, w, rstd)
    assert same(ops.rms_norm_backward(dy, h, w, rstd, torch.zeros_like(dy)), (dh0, dw0))
    assert torch.equal(dw0, dw) and not torch.equal(dh0, dh)
    # in place: h over x, h over residual, dh over dy, dh over dres
    for over in ("x", "residual"):
        xc, rc = x.clone(), r.clone()
        out = ops.add_rms_norm_forward(xc, rc, w, EPS, h=xc if over == "x" else rc)
        assert out[0] is (xc if over == "x" else rc) and same(out, (h, y, rstd)), f"h over {over}"
        assert torch.equal(rc if over == "x" else xc, r if over == "x" else x)
    for over in ("dy", "dres"):
        dyc, drc = dy.clone(), dres.clone()
        out = ops.rms_norm_backward(dyc, h, w, rstd, drc, dh=dyc if over == "dy" else drc)
        assert out[0] is (dyc if over == "dy" else drc) and same(out, (dh, dw)), f"dh over {over}"
    # need_dw = False: the same dh, dw and partials untouched
    chunks = (T + CHUNK - 1) // CHUNK
    dws, parts = torch.full((d,), SENTINEL, device="cuda"), torch.full((chunks, d), SENTINEL, device="cuda")
    dhn, none = ops.rms_norm_backward(dy, h, w, rstd, dres, dw=dws, partials=parts, need_dw=False)
    assert none is None and torch.equal(dhn, dh) and (dws == SENTINEL).all() and (parts == SENTINEL).all()
    # caller-owned buffers are the ones written
    dhb = torch.empty_like(dh)
    out = ops.rms_norm_backward(dy, h, w, rstd, dres, dh=dhb, dw=dws, partials=parts)
    assert out[0] is dhb and out[1] is dws and same(out, (dh, dw))


@pytest.mark.parametrize("wname", sorted(WEIGHTS))
@pytest.mark.parametrize("d", (64, 4096))
def test_autograd_forms_equal_the_raw_forms(d, wname):
    T = CHUNK + 1
    w = _weight(d, WEIGHTS[wname])
    x, r, dy, dres = _inputs(T, d)
    h, y, rstd = ops.add_rms_norm_forward(x, r, w, EPS)
    dh, dw = ops.rms_norm_backward(dy, h, w, rstd, dres)
    xl, rl, wl = x.clone().requires_grad_(), r.clone().requires_grad_(), w.clone().requires_grad_()
    ha, ya = ops.add_rms_norm(xl, rl, wl, EPS)
    assert torch.equal(ha, h) and torch.equal(ya, y)
    gx, gr, gw = torch.autograd.grad((ha, ya), (xl, rl, wl), (dres, dy))
    assert gx.data_ptr() == gr.data_ptr(), "x and residual must receive the same dh tensor, not a copy"
    assert torch.equal(gx, dh) and gw.dtype == w.dtype and torch.equal(gw, dw.to(w.dtype))
    # either gradient may be missing
    ha, ya = ops.add_rms_norm(xl, rl, wl, EPS)
    gx, gw = torch.autograd.grad(ya, (xl, wl), dy)
    assert torch.equal(gx, ops.rms_norm_backward(dy, h, w, rstd)[0]) and torch.equal(gw, dw.to(w.dtype))
    ha, ya = ops.add_rms_norm(xl, rl, wl, EPS)
    gx, gw = torch.autograd.grad(ha, (xl, wl), dres, allow_unused=True)
    zero = torch.zeros_like(dy)
    assert torch.equal(gx, ops.rms_norm_backward(zero, h, w, rstd, dres)[0]) and not gw.any()
    # without a residual; a gradient that breaks the view rules (the expanded scalar of a sum) is made contiguous
    y1, rstd1 = ops.rms_norm_forward(x, w, EPS)
    ya = ops.rms_norm(xl, wl, EPS)
    assert torch.equal(ya, y1)
    gx, gw = torch.autograd.grad(ya.sum(), (xl, wl))
    want = ops.rms_norm_backward(torch.ones_like(x), x, w, rstd1)
    assert torch.equal(gx, want[0]) and torch.equal(gw, want[1].to(w.dtype))
    # a frozen weight: no dw
    ya = ops.rms_norm(xl, w, EPS)
    (gx,) = torch.autograd.grad(ya, (xl,), dy)
    assert torch.equal(gx, ops.rms_norm_backward(dy, x, w, rstd1, need_dw=False)[0])


# --- adjoint -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("wname", sorted(WEIGHTS))
@pytest.mark.parametrize("d", (136, 4096))
def test_adjoint_against_autograd_through_the_fp64_mirror(d, wname):
    """L = <y, dy> + <h, dres> differentiated through ``ops.add_rms_norm`` against
    ``torch.autograd.grad`` of the fp64 mirror at the kernel's (rounded) ``h``, within the bounds
    of the backward accuracy test."""
    T = 257
    w = _weight(d, WEIGHTS[wname])
    x, r, dy, dres = _inputs(T, d)
    xl, rl, wl = x.clone().requires_grad_(), r.clone().requires_grad_(), w.clone().requires_grad_()
    h, y = ops.add_rms_norm(xl, rl, wl, EPS)
    L = (y.float() * dy.float()).sum() + (h.float() * dres.float()).sum()
    gx, gr, gw = torch.autograd.grad(L, (xl, rl, wl))
    assert gx.data_ptr() == gr.data_ptr()
    hd, wd = h.detach().double().requires_grad_(), w.double().requires_grad_()
    _, y64, _ = ops.rms_norm_reference(hd, wd, EPS)
    L64 = (y64 * dy.double()).sum() + (hd * dres.double()).sum()
    eh, ew = torch.autograd.grad(L64, (hd, wd))
    _, _, tol_dh, tol_dw = _backward_bounds(dy, h.detach(), w, dres)
    if w.dtype == BF:
        tol_dw = tol_dw + 2.0 ** -8 * ew.abs()
    rdh, rdw = _worst((gx.double() - eh).abs(), tol_dh), _worst((gw.double() - ew).abs(), tol_dw)
    print(f"[rms_norm adjoint d={d} weight={wname}] worst error / tolerance: dh {rdh:.3f} dw {rdw:.3f}")
    assert rdh <= 1.0 and rdw <= 1.0


# --- safety --------------------------------------------------------------------------------------------------

def _framed(T, d, stride, offset, contents=None):
    """A [T, d] view with that row stride inside a sentinel-filled buffer, and a mask of what it covers."""
    numel = offset + T * stride + 8
    buf = torch.full((numel,), SENTINEL, dtype=BF, device="cuda")
    view = buf.as_strided((T, d), (stride, 1), offset)
    mask = torch.zeros(numel, dtype=torch.bool, device="cuda")
    mask.as_strided((T, d), (stride, 1), offset).fill_(True)
    if contents is not None:
        view.copy_(contents)
    return buf, view, mask


@pytest.mark.parametrize("wname", sorted(WEIGHTS))
def test_framed_views(wname):
    """Every operand and output is a column slice / row view with a row stride of its own inside a
    sentinel-filled buffer: the contiguous call's bits, and not one sentinel outside the views changes."""
    T, d = CHUNK + 1, 136
    w = _weight(d, WEIGHTS[wname])
    x, r, dy, dres = _inputs(T, d)
    h, y, rstd = ops.add_rms_norm_forward(x, r, w, EPS)
    dh, dw = ops.rms_norm_backward(dy, h, w, rstd, dres)
    bx, vx, mx = _framed(T, d, 3 * d + 8, 8, x)      # a column slice of a fused buffer
    br, vr, _ = _framed(T, d, 2 * d, 16 + d, r)      # every other row
    bh, vh, mh = _framed(T, d, d + 8, 24)
    by, vy, my = _framed(T, d, 2 * d + 16, 8)
    keep_x, keep_r = bx.clone(), br.clone()
    out = ops.add_rms_norm_forward(vx, vr, w, EPS, h=vh, y=vy)
    assert torch.equal(out[0], h) and torch.equal(out[1], y) and torch.equal(out[2], rstd)
    assert torch.equal(bx, keep_x) and torch.equal(br, keep_r), "the forward changed its inputs' buffers"
    assert (bh[~mh] == SENTINEL).all() and (by[~my] == SENTINEL).all(), "bytes outside the output views changed"
    y1 = ops.rms_norm_forward(vh, w, EPS, y=vy)[0]  # no residual, strided in and out
    assert torch.equal(y1, y) and (by[~my] == SENTINEL).all()
    # in place over a framed x
    ops.add_rms_norm_forward(vx, vr, w, EPS, h=vx, y=vy)
    assert torch.equal(vx, h) and torch.equal(bx[~mx], keep_x[~mx])
    # backward
    bg, vg, _ = _framed(T, d, 4 * d, 8 + d, dy)
    bd, vd, _ = _framed(T, d, d + 24, 16, dres)
    bo, vo, mo = _framed(T, d, 5 * d + 8, 32)
    keep_g, keep_d, keep_h = bg.clone(), bd.clone(), bh.clone()
    out = ops.rms_norm_backward(vg, vh, w, rstd, vd, dh=vo)
    assert torch.equal(out[0], dh) and torch.equal(out[1], dw)
    assert torch.equal(bg, keep_g) and torch.equal(bd, keep_d) and torch.equal(bh, keep_h)
    assert (bo[~mo] == SENTINEL).all(), "bytes outside dh's view changed"


def test_row_stride_of_2_to_the_30_elements():
    """Three rows 2^30 elements (2 GiB) apart: the last one's byte offset needs more than 32 bits.
    Only the rows in use are ever touched; the buffer is never filled."""
    d, step = 136, 1 << 30
    w = _weight(d, BF)
    x, r, dy, dres = _inputs(3, d)
    h, y, rstd = ops.add_rms_norm_forward(x, r, w, EPS)
    dh, dw = ops.rms_norm_backward(dy, h, w, rstd, dres)
    big = torch.empty(2 * step + d, dtype=BF, device="cuda")
    far = big.as_strided((3, d), (step, 1))
    far.copy_(x)
    out = ops.add_rms_norm_forward(far, r, w, EPS)  # strided in, contiguous out
    assert torch.equal(out[0], h) and torch.equal(out[1], y) and torch.equal(out[2], rstd)
    ops.add_rms_norm_forward(far, r, w, EPS, h=far)  # in place
    assert torch.equal(far, h)
    out = ops.rms_norm_backward(dy, far, w, rstd, dres)  # strided h
    assert torch.equal(out[0], dh) and torch.equal(out[1], dw)
    far.copy_(dy)
    out = ops.rms_norm_backward(far, h, w, rstd, dres, dh=far)  # strided dy, dh in place over it
    assert torch.equal(far, dh) and torch.equal(out[1], dw)
    del far, big, out
    torch.cuda.empty_cache()


def test_graph_replay_with_caller_owned_buffers():
    T, d = 257, 4096
    w = _weight(d, BF)
    chunks = (T + CHUNK - 1) // CHUNK
    x, r, dy, dres = (t.clone() for t in _inputs(T, d))
    h, y, dh = (torch.empty(T, d, dtype=BF, device="cuda") for _ in range(3))
    rstd, dw, parts = (torch.empty(s, dtype=F32, device="cuda") for s in ((T,), (d,), (chunks, d)))

    def run():
        ops.add_rms_norm_forward(x, r, w, EPS, h=h, y=y, rstd=rstd)
        ops.rms_norm_backward(dy, h, w, rstd, dres, dh=dh, dw=dw, partials=parts)

    cs = torch.cuda.Stream()
    cs.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(cs):
        with torch.cuda.graph(g, stream=cs):
            run()
    torch.cuda.current_stream().wait_stream(cs)
    torch.cuda.synchronize()
    contents = [(x.clone(), dy.clone()), (_rows(T, d, 7), _rows(T, d, 8))]
    want = []
    for nx, ndy in contents:
        eh, ey, er = ops.add_rms_norm_forward(nx, r, w, EPS)
        want.append((eh, ey, er, *ops.rms_norm_backward(ndy, eh, w, er, dres)))
    assert not torch.equal(want[0][1], want[1][1])
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    for (nx, ndy), expect in zip(contents, want):
        x.copy_(nx)
        dy.copy_(ndy)
        for t in (h, y, dh):
            t.fill_(SENTINEL)
        g.replay()
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == before, "a replay allocated"
        for name, got, e in zip(("h", "y", "rstd", "dh", "dw"), (h, y, rstd, dh, dw), expect):
            assert torch.equal(got, e), f"the replay's {name} differs from the eager call on the new contents"


def test_refused_calls_leave_the_outputs_untouched():
    T, d = CHUNK + 1, 64
    w = _weight(d, BF)
    x, r, dy, dres = _inputs(T, d)
    _, _, rstd_ok = ops.add_rms_norm_forward(x, r, w, EPS)
    full = lambda *shape, dtype=BF: torch.full(shape, SENTINEL, dtype=dtype, device="cuda")
    h, y, dh = full(T, d), full(T, d), full(T, d)
    rstd, dw, parts = full(T, dtype=F32), full(d, dtype=F32), full(2, d, dtype=F32)
    off = full(T * d + 8)
    y_off = off[4:4 + T * d].view(T, d)  # 8 bytes past a 16-byte boundary
    fwd = lambda *a, **kw: ops.add_rms_norm_forward(*a, **{"h": h, "y": y, "rstd": rstd, **kw})
    bwd = lambda *a, **kw: ops.rms_norm_backward(*a, **{"dh": dh, "dw": dw, "partials": parts, **kw})
    refused = [
        (TypeError, lambda: fwd(x.float(), r, w, EPS)),
        (TypeError, lambda: fwd(x, r, w.half(), EPS)),
        (TypeError, lambda: fwd(x, r, w, EPS, rstd=rstd.double())),
        (TypeError, lambda: bwd(dy, x, w, rstd_ok, dres, dw=dw.double())),
        (TypeError, lambda: bwd(dy.float(), x, w, rstd_ok)),
        (ValueError, lambda: fwd(x, r[:-1], w, EPS)),
        (ValueError, lambda: fwd(x, r, w, 0.0)),
        (ValueError, lambda: fwd(x, r, w.cpu(), EPS)),
        (ValueError, lambda: fwd(x, r, w, EPS, y=y_off)),
        (ValueError, lambda: fwd(x, r, w, EPS, y=y[:, :d - 8])),
        (ValueError, lambda: fwd(x, r, w, EPS, rstd=rstd[:-1])),
        (ValueError, lambda: fwd(x, None, w, EPS)),
        (ValueError, lambda: ops.rms_norm_forward(x[:, :12], w[:12], EPS, y=y[:, :12])),
        (ValueError, lambda: bwd(dy, x, w, rstd_ok[:-1])),
        (ValueError, lambda: bwd(dy, x, w, rstd_ok, dres[:, :d - 8])),
        (ValueError, lambda: bwd(dy, x, w, rstd_ok, partials=parts[:1])),
        (ValueError, lambda: bwd(dy, x, w, rstd_ok, dh=y_off)),
    ]
    for error, call in refused:
        with pytest.raises(error, match="rms_norm"):
            call()
    # the extension's own refusals, all on the host, before any launch
    dev = _native.device()
    stream = torch.cuda.current_stream().cuda_stream
    view = lambda t: (t.data_ptr(), t.stride(0))

    def raw_fwd(T_=T, d_=d, xv=None, rv=None, hv=None, yv=None, wp=None, rp=None, eps=EPS):
        dev.rms_norm_fwd(xv or view(x), rv or view(r), hv or view(h), yv or view(y), wp if wp is not None else w.data_ptr(),
                         False, rp if rp is not None else rstd.data_ptr(), T_, d_, eps, stream)

    def raw_bwd(T_=T, d_=d, gv=None, ov=None, rp=None, pp=None, dp=None, chunk=CHUNK):
        dev.rms_norm_bwd(gv or view(dy), view(x), view(dres), ov or view(dh), w.data_ptr(), False,
                         rp if rp is not None else rstd_ok.data_ptr(), pp if pp is not None else parts.data_ptr(),
                         dp if dp is not None else dw.data_ptr(), T_, d_, chunk, stream)

    for kw in (dict(d_=12), dict(d_=0), dict(d_=16392), dict(T_=0), dict(T_=(1 << 30) + 1), dict(eps=0.0), dict(eps=-1.0),
               dict(xv=(x.data_ptr() + 2, d)), dict(xv=(x.data_ptr(), d + 4)), dict(yv=(0, d)), dict(yv=(y.data_ptr() + 8, d)),
               dict(hv=(0, 0)), dict(rv=(0, 0)), dict(hv=(h.data_ptr(), d + 2)), dict(wp=0), dict(wp=w.data_ptr() + 2),
               dict(rp=0), dict(rp=rstd.data_ptr() + 2)):
        with pytest.raises(ValueError, match="rms_norm"):
            raw_fwd(**kw)
    for kw in (dict(d_=12), dict(d_=16392), dict(T_=0), dict(chunk=CHUNK + 1), dict(chunk=0),
               dict(gv=(dy.data_ptr() + 2, d)), dict(gv=(dy.data_ptr(), d + 4)), dict(ov=(0, d)), dict(ov=(dh.data_ptr(), d + 1)),
               dict(rp=0), dict(pp=0), dict(dp=0), dict(pp=parts.data_ptr() + 4), dict(dp=dw.data_ptr() + 2)):
        with pytest.raises(ValueError, match="rms_norm"):
            raw_bwd(**kw)
    torch.cuda.synchronize()
    for name, buf in (("h", h), ("y", y), ("dh", dh), ("rstd", rstd), ("dw", dw), ("partials", parts), ("misaligned y", off)):
        assert (buf == SENTINEL).all(), f"a refused call wrote {name}"


# --- the model -------------------------------------------------------------------------------------------------

TINY = dict(d=256, heads=4, kv_heads=2, ffn=256, vocab=512, layers=2)


def _tp():
    from collective_communication_mpi_amd import MPI, Communicator

    return Communicator(MPI.COMM_WORLD)  # one rank: the TP group of the layers


def _ids(B, S):
    return torch.randint(0, 512, (B, S), device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))


def _model(tp, **cfg):
    """Seed 3, and every norm weight overwritten with the same seeded values in [0.5, 1.5]."""
    from collective_communication_mpi_amd.parallel.llama_dp import LlamaConfig, LlamaModel

    model = LlamaModel(LlamaConfig(**TINY, **cfg), tp, torch.device("cuda"), seed=3)
    g = torch.Generator(device="cuda").manual_seed(77)
    norms = [p for name, p in model.named_parameters() if name.endswith("norm.weight")]
    assert len(norms) == 2 * TINY["layers"] + 1
    with torch.no_grad():
        for p in norms:
            p.copy_((0.5 + torch.rand(p.shape, device="cuda", generator=g)).to(p.dtype))
    return model


def _compare(tag, a_model, b_model, loss_a, loss_b):
    rel = abs(loss_a - loss_b) / abs(loss_b)
    worst = 1.0
    for (name, a), (_, b) in zip(a_model.named_parameters(), b_model.named_parameters()):
        assert a.grad is not None and b.grad is not None, name
        cos = torch.nn.functional.cosine_similarity(a.grad.double().flatten(), b.grad.double().flatten(), dim=0).item()
        worst = min(worst, cos)
    print(f"[rms_norm model] {tag}: losses {loss_a:.6f} / {loss_b:.6f} relative difference {rel:.3e}; worst gradient cosine {worst:.6f}")
    assert rel <= 2.0 ** -7
    assert worst >= 0.999


@pytest.mark.parametrize("case", ("sdpa", "flash", "flash packed"))
def test_model_fused_norm_matches_torch_norm(case):
    tp, ids = _tp(), _ids(2, 257)
    kw = {}
    if case == "flash packed":
        bounds = [0, 3, 3, 200, 514]
        targets = torch.roll(ids.reshape(1, -1), -1, dims=1).reshape(2, 257).clone()
        flat = targets.view(-1)
        for end in (3, 200, 514):
            flat[end - 1] = -100
        kw = dict(targets=targets, cu_seqlens=torch.tensor(bounds, dtype=torch.int32, device="cuda"))
    models, losses = {}, {}
    for norm in ("torch", "fused"):
        m = models[norm] = _model(tp, attention=case.split()[0], norm=norm)
        loss = m(ids, **kw)
        loss.backward()
        losses[norm] = loss.item()
    for a, b in zip(models["torch"].parameters(), models["fused"].parameters()):
        assert torch.equal(a, b)
    _compare(f"{case}: fused against torch", models["fused"], models["torch"], losses["fused"], losses["torch"])


def test_model_norm_switch():
    from collective_communication_mpi_amd.parallel.llama_dp import LlamaConfig, LlamaModel

    tp, ids = _tp(), _ids(2, 257)
    with pytest.raises(ValueError, match="norm"):
        LlamaModel(LlamaConfig(**TINY, norm="layer"), tp, torch.device("cuda"), seed=3)
    with torch.no_grad():
        explicit, default = _model(tp, norm="torch")(ids), _model(tp)(ids)
    assert torch.equal(explicit, default), 'norm="torch" is not the model without the field'
