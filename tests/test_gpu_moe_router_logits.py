"""Router logits on the matrix cores (csrc/device/moe_router.hip, ``ops.moe_router_logits``) on
one GPU: the fp32 router as three bf16 planes against the bf16 activations.

Inputs per shape (T, D, E): ``x = randn.bfloat16()``, ``router = randn / sqrt(D)`` in fp32,
``dlogits = 1e-2 * randn``; made once per shape and never written.

Exact checks: ``split_bf16x3`` equals the torch composition bit for bit (1 to 3 planes, both
orientations, and the side-by-side form with its zero padding) and the three planes add up to
the router; with one nonzero per row of ``x`` (1, -2 or 0.5 at column t % D, every column of D
hit) every logit is ``x[t, j] * router[e, j]`` bit for bit, which no one-plane or two-plane
shortcut and no K tail that drops or doubles a column passes; ``forward(x[:n])`` is
``forward(x)[:n]``; the three row tiles the launcher chooses between by T (128, 64, 32 rows
per workgroup) give the same bits; a row-strided ``x`` gives the bits of its contiguous copy; rows of ``out``
at or past T keep a sentinel; two calls (forward and backward) and a graph replay in front of
``ops.moe_gate_forward`` give the same bits.

Accuracy, by the rule of test_gpu_moe_gate.py: the error of the logits against the fp64 product
is at most 8 x the error ``x.float() @ router.t()`` makes against fp64 on that input, floor
2^-22 x the largest reference magnitude (both measured here, on the device); the same per
tensor for ``dx`` (yardstick: the torch path's bf16 ``x.grad``) and ``drouter`` (the torch
path's fp32 ``router.grad``).  The worst error / tolerance ratios are printed; measured values
are in profiles/moe/README.md.

Memory: at T = 2048, D = 1024, E = 64 the forward of ``ops.moe_router_logits`` with the graph
retained raises ``torch.cuda.memory_allocated`` by less than T * D * 2 bytes (half an fp32 copy
of ``x``); the torch form, measured the same way, by more."""
import pytest
import torch

from collective_communication_mpi_amd import ops

pytestmark = pytest.mark.gpu

SHAPES = [(0, 64, 8), (1, 8, 1), (5, 72, 8), (130, 200, 24), (257, 448, 96), (131, 1024, 200), (129, 7168, 256)]
FLOOR = 2.0 ** -22
SENTINEL = -12345.5
ROW_TILES = (None, 32, 64, 128)  # rows per workgroup: the launcher's choice by T, and each one forced


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _inputs(T, D, E, salt=0):
    g = torch.Generator(device="cuda").manual_seed(4001 + 131 * T + 17 * D + E + 7919 * salt)
    x = torch.randn(T, D, device="cuda", generator=g).bfloat16()
    router = torch.randn(E, D, device="cuda", generator=g) / D ** 0.5
    dlogits = 1e-2 * torch.randn(T, E, device="cuda", generator=g)
    return x, router, dlogits


_DATA = {}


def _data(shape):
    """Inputs and references of one shape: made once, never written."""
    if shape not in _DATA:
        x, router, dl = _inputs(*shape)
        d = {"x": x, "router": router, "dl": dl}
        d["logits64"] = x.double() @ router.double().t()
        d["dx64"] = dl.double() @ router.double()
        d["dr64"] = dl.double().t() @ x.double()
        xg, rg = x.clone().requires_grad_(), router.clone().requires_grad_()
        logits32 = xg.float() @ rg.t()
        logits32.backward(dl)
        d["logits32"], d["dx_torch"], d["dr_torch"] = logits32.detach(), xg.grad, rg.grad
        _DATA[shape] = d
    return _DATA[shape]


def _compose(w):
    p0 = w.bfloat16()
    p1 = (w - p0.float()).bfloat16()
    p2 = (w - p0.float() - p1.float()).bfloat16()
    return torch.stack([p0, p1, p2])


def _bits(a, b):
    """Same dtype, shape and bit pattern (torch.equal would let -0.0 pass for 0.0)."""
    as_int = {2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(as_int), b.view(as_int))


def _ratio(tag, got, ref64, yard):
    own = (yard.double() - ref64).abs().max().item()
    tol = max(8 * own, FLOOR * ref64.abs().max().item())
    err = (got.double() - ref64).abs().max().item()
    ratio = err / tol if tol > 0 else (0.0 if err == 0 else float("inf"))
    print(f"moe_router_logits {tag}: error {err:.3e}, torch error {own:.3e}, tolerance {tol:.3e}, "
          f"error / tolerance {ratio:.3f}")
    assert torch.isfinite(got).all(), tag
    assert err <= tol, f"{tag}: error {err:.3e} > tolerance {tol:.3e} (torch error {own:.3e})"
    return ratio


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_split_is_exact(shape):
    d = _data(shape)
    for w in (d["router"], d["dl"]):
        want = _compose(w)
        if w.numel():
            assert torch.equal((want[0].float() + want[1].float()) + want[2].float(), w)
        for planes in (1, 2, 3):
            assert _bits(ops.split_bf16x3(w, planes=planes), want[:planes])
            assert _bits(ops.split_bf16x3(w, planes=planes, transpose=True), want[:planes].transpose(1, 2).contiguous())
        R, C = w.shape
        for tr in (False, True):
            src = want.transpose(1, 2) if tr else want
            F = R if tr else C
            Fp = (F + 7) // 8 * 8
            got = ops.split_bf16x3(w, transpose=tr, concat=(0, 0, 1, 2), pad=8)
            exp = torch.zeros(src.shape[1], 4 * Fp, dtype=torch.bfloat16, device="cuda")
            for s, p in enumerate((0, 0, 1, 2)):
                exp[:, s * Fp:s * Fp + F] = src[p]
            assert _bits(got, exp)


def test_split_into_a_given_buffer():
    w = _data((130, 200, 24))["router"]
    out = torch.full((3, 24, 200), 7.0, dtype=torch.bfloat16, device="cuda")
    assert ops.split_bf16x3(w, out=out) is out
    assert _bits(out, _compose(w))


@pytest.mark.parametrize("D,E", [(72, 8), (200, 24), (128, 13)], ids=str)
def test_all_24_mantissa_bits_reach_the_logits(D, E):
    T = D + 3
    _, router, _ = _inputs(T, D, E, salt=3)
    vals = torch.tensor([1.0, -2.0, 0.5], device="cuda")[torch.arange(T, device="cuda") % 3]
    cols = torch.arange(T, device="cuda") % D
    x = torch.zeros(T, D, device="cuda")
    x[torch.arange(T, device="cuda"), cols] = vals
    x = x.bfloat16()
    want = vals[:, None] * router[:, cols].t()  # a power of two times the router: exact
    for row_tile in ROW_TILES:
        got = ops.moe_router_logits_forward(x, router, row_tile=row_tile)
        assert got.shape == (T, E) and got.dtype == torch.float32
        assert torch.equal(got, want), \
            f"row tile {row_tile}: {(got != want).sum().item()} of {T * E} logits are not x * router exactly"
    # the check can fail: two planes are not the router
    two = _compose(router)[:2].float().sum(0)
    assert not torch.equal(vals[:, None] * two[:, cols].t(), want)


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_forward_and_backward_against_fp64(shape):
    T, D, E = shape
    d = _data(shape)
    planes = ops.split_bf16x3(d["router"])
    logits = ops.moe_router_logits_forward(d["x"], d["router"])
    assert logits.shape == (T, E) and logits.dtype == torch.float32 and logits.is_contiguous()
    for row_tile in ROW_TILES[1:]:
        assert _bits(ops.moe_router_logits_forward(d["x"], d["router"], planes=planes, row_tile=row_tile), logits), row_tile
    dx, dr = ops.moe_router_logits_backward(d["dl"], d["x"], planes)
    assert dx.shape == (T, D) and dx.dtype == torch.bfloat16
    assert dr.shape == (E, D) and dr.dtype == torch.float32
    if T == 0:
        assert dr.abs().max().item() == 0
        return
    worst = {"logits": _ratio(f"{shape} logits", logits, d["logits64"], d["logits32"]),
             "dx": _ratio(f"{shape} dx", dx, d["dx64"], d["dx_torch"]),
             "drouter": _ratio(f"{shape} drouter", dr, d["dr64"], d["dr_torch"])}
    print(f"moe_router_logits {shape}: worst error / tolerance " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    only_dx = ops.moe_router_logits_backward(d["dl"], d["x"], planes, need_drouter=False)
    only_dr = ops.moe_router_logits_backward(d["dl"], d["x"], planes, need_dx=False)
    assert only_dx[1] is None and only_dr[0] is None
    assert _bits(only_dx[0], dx) and _bits(only_dr[1], dr)


def test_a_tokens_logits_do_not_depend_on_the_batch():
    d = _data((257, 448, 96))
    full = ops.moe_router_logits_forward(d["x"], d["router"])
    for n in (1, 64, 129):
        for row_tile in ROW_TILES:
            assert _bits(ops.moe_router_logits_forward(d["x"][:n], d["router"], row_tile=row_tile), full[:n]), (n, row_tile)


@pytest.mark.parametrize("shape", [(130, 200, 24), (257, 448, 96)], ids=str)
def test_row_strided_x_gives_the_bits_of_its_copy(shape):
    T, D, E = shape
    d = _data(shape)
    wide = torch.full((T, D + 24), 3.0, dtype=torch.bfloat16, device="cuda")
    view = wide[:, 8:8 + D]
    view.copy_(d["x"])
    assert not view.is_contiguous()
    assert _bits(ops.moe_router_logits_forward(view, d["router"]), ops.moe_router_logits_forward(d["x"], d["router"]))
    planes = ops.split_bf16x3(d["router"])
    for a, b in zip(ops.moe_router_logits_backward(d["dl"], view, planes),
                    ops.moe_router_logits_backward(d["dl"], d["x"], planes)):
        assert _bits(a, b)


@pytest.mark.parametrize("shape", [(1, 8, 1), (130, 200, 24), (131, 1024, 200), (129, 7168, 256)], ids=str)
def test_rows_past_T_are_not_written(shape):
    T, D, E = shape
    d = _data(shape)
    want = ops.moe_router_logits_forward(d["x"], d["router"])
    for row_tile in ROW_TILES:
        big = torch.full((T + 130, E), SENTINEL, device="cuda")
        out = ops.moe_router_logits_forward(d["x"], d["router"], out=big[:T], row_tile=row_tile)
        assert out.data_ptr() == big.data_ptr()
        assert (big[T:] == SENTINEL).all(), row_tile
        assert _bits(big[:T], want), row_tile


@pytest.mark.parametrize("shape", SHAPES[2:], ids=str)
def test_two_calls_give_the_same_bits(shape):
    d = _data(shape)
    planes = ops.split_bf16x3(d["router"])
    a = ops.moe_router_logits_forward(d["x"], d["router"], planes=planes)
    b = ops.moe_router_logits_forward(d["x"].clone(), d["router"].clone())
    assert _bits(a, b)
    ga = ops.moe_router_logits_backward(d["dl"], d["x"], planes)
    gb = ops.moe_router_logits_backward(d["dl"].clone(), d["x"].clone(), planes.clone())
    assert _bits(ga[0], gb[0]) and _bits(ga[1], gb[1])


def test_graph_replay_in_front_of_the_gate():
    shape, K = (131, 1024, 200), 8
    d = _data(shape)
    router = d["router"]
    planes = ops.split_bf16x3(router)
    news = [_inputs(*shape, salt=s)[0] for s in (1, 2)]
    want = []
    for n in news:
        lg = ops.moe_router_logits_forward(n, router)
        want.append((lg, *ops.moe_gate_forward(lg, K, True)))
    static = d["x"].clone()
    out = torch.empty(shape[0], shape[2], device="cuda")
    cs = torch.cuda.Stream()
    cs.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(cs):
        with torch.cuda.graph(g, stream=cs):
            ops.moe_router_logits_forward(static, router, planes=planes, out=out)
            gate = ops.moe_gate_forward(out, K, True)
    torch.cuda.current_stream().wait_stream(cs)
    for n, w in zip(news, want):
        static.copy_(n)
        g.replay()
        torch.cuda.synchronize()
        for got, exp in zip((out, *gate), w):
            assert _bits(got, exp)
    del g


@pytest.mark.parametrize("need_x,need_r", [(True, True), (True, False), (False, True), (False, False)])
def test_autograd_returns_gradients_only_where_asked(need_x, need_r):
    shape = (130, 200, 24)
    d = _data(shape)
    x = d["x"].clone().requires_grad_(need_x)
    r = d["router"].clone().requires_grad_(need_r)
    logits = ops.moe_router_logits(x, r)
    assert _bits(logits.detach(), ops.moe_router_logits_forward(d["x"], d["router"]))
    assert logits.requires_grad == (need_x or need_r)
    if not (need_x or need_r):
        return
    logits.backward(d["dl"])
    assert (x.grad is not None) == need_x and (r.grad is not None) == need_r
    if need_x:
        assert x.grad.dtype == torch.bfloat16
        _ratio(f"{shape} autograd dx", x.grad, d["dx64"], d["dx_torch"])
    if need_r:
        assert r.grad.dtype == torch.float32
        _ratio(f"{shape} autograd drouter", r.grad, d["dr64"], d["dr_torch"])


def test_no_fp32_copy_of_the_activations():
    T, D, E = 2048, 1024, 64
    x0, r0, _ = _inputs(T, D, E)
    limit = T * D * 2

    def rise(fn):
        x, r = x0.clone().requires_grad_(), r0.clone().requires_grad_()
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        logits = fn(x, r)  # alive, with its graph, while the second reading is taken
        torch.cuda.synchronize()
        after = torch.cuda.memory_allocated()
        assert logits.grad_fn is not None
        return after - before

    mfma = rise(ops.moe_router_logits)
    torch_form = rise(lambda x, r: x.float() @ r.t())
    print(f"moe_router_logits forward with the graph retained at {(T, D, E)}: {mfma} bytes, torch form {torch_form} "
          f"bytes, limit {limit}")
    assert torch_form > limit, "the torch form no longer keeps an fp32 copy: this test cannot fail"
    assert mfma < limit
