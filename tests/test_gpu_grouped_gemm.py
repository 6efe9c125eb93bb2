"""Grouped expert GEMM (csrc/device/grouped_gemm.hip) on one GPU against the per-expert
``x[rows].float() @ w[g].float().T`` loop in torch: forward in both output dtypes with
sentinel rows, isolation of an expert from the others (bitwise), counts that overflow the
buffer, int32 / int64 counts, the weight gradient with NaN outside the expert's rows,
``grouped_linear`` against torch autograd, a captured graph replayed with new counts, and
a single expert that owns every row against the dense 128x128 kernels (bitwise: both run
the tile of csrc/device/gemm_tile128.hpp).

Tolerances are those of tests/test_gpu_kernels.py for the same tile and randn inputs:
fp32 forward rtol 2e-3, atol 2e-3 sqrt(K); bf16 forward rtol 2e-2, atol 8e-2; weight
gradient rtol 2e-3, atol 2e-3 sqrt(largest count)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = -512.0


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _random_counts():
    c = np.random.default_rng(4242).integers(1, 200, size=8)
    c[2], c[5] = 0, 300
    return [int(v) for v in c]


#        name       counts                                      cap spare   N    K
CASES = {
    "edge": ([130], 0, 72, 72),
    "mixed": ([0, 1, 127, 129], 43, 136, 64),
    "exact": ([128, 0, 0, 256, 3], 0, 128, 192),
    "random": (_random_counts(), 17, 264, 520),
    "limit": ([1 if g % 7 else 0 for g in range(256)], 256 - sum(1 if g % 7 else 0 for g in range(256)), 64, 64),
}


def _bounds(counts, cap):
    e = np.minimum(np.cumsum([0] + [max(int(c), 0) for c in counts]), cap)
    return [(int(e[g]), int(e[g + 1])) for g in range(len(counts))]


def _ref_fwd(x, w, counts, cap, bias=None, alpha=1.0):
    """fp32 reference of the rows in [0, min(total, cap))."""
    parts = []
    for g, (a, b) in enumerate(_bounds(counts, cap)):
        y = alpha * (x[a:b].float() @ w[g].float().T)
        parts.append(y if bias is None else y + bias[g].float())
    return torch.cat(parts)


_DATA = {}


def _data(name):
    """(x, w, counts list, cap, N, K, fp32 reference): made once per case, never written."""
    if name not in _DATA:
        counts, spare, N, K = CASES[name]
        cap = sum(counts) + spare
        g = torch.Generator(device="cuda").manual_seed(1000 + len(name) * 31 + N + K)
        x = torch.randn(cap, K, device="cuda", generator=g).bfloat16()
        w = torch.randn(len(counts), N, K, device="cuda", generator=g).bfloat16()
        _DATA[name] = (x, w, counts, cap, N, K, _ref_fwd(x, w, counts, cap))
    return _DATA[name]


def _tol(dtype, K):
    return dict(rtol=2e-3, atol=2e-3 * K ** 0.5) if dtype == torch.float32 else dict(rtol=2e-2, atol=8e-2)


def _cnt(counts, dtype=torch.int64):
    return torch.tensor(counts, dtype=dtype, device="cuda")


def test_case_table_is_the_one_asked_for():
    assert sum(CASES["mixed"][0]) + CASES["mixed"][1] == 300 and sum(CASES["exact"][0]) == 387
    assert sum(CASES["limit"][0]) + CASES["limit"][1] == 256
    rc = CASES["random"][0]
    assert len(rc) == 8 and min(rc) == 0 and max(rc) > 256


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", list(CASES))
def test_forward(name, out_dtype):
    from collective_communication_mpi_amd.ops import grouped_gemm_nt

    x, w, counts, cap, N, K, ref = _data(name)
    total = sum(counts)
    out = torch.full((cap, N), SENTINEL, dtype=out_dtype, device="cuda")
    got = grouped_gemm_nt(x, w, _cnt(counts), out=out)
    assert got is out
    torch.testing.assert_close(out[:total].float(), ref, **_tol(out_dtype, K))
    assert torch.equal(out[total:], torch.full_like(out[total:], SENTINEL)), "rows past the total were written"


@pytest.mark.parametrize("bias_dtype", [torch.float32, torch.bfloat16], ids=["bias32", "bias16"])
def test_forward_bias_alpha_default_out(bias_dtype):
    from collective_communication_mpi_amd.ops import grouped_gemm_nt

    x, w, counts, cap, N, K, _ = _data("mixed")
    total = sum(counts)
    bias = torch.randn(len(counts), N, device="cuda").to(bias_dtype)
    y = grouped_gemm_nt(x, w, _cnt(counts), bias=bias, alpha=0.5, out_dtype=torch.float32)
    assert y.shape == (cap, N) and y.dtype == torch.float32
    torch.testing.assert_close(y[:total], _ref_fwd(x, w, counts, cap, bias, 0.5), **_tol(torch.float32, K))
    assert grouped_gemm_nt(x, w, _cnt(counts)).dtype == torch.bfloat16


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", ["mixed", "random"])
def test_isolation(name, out_dtype):
    """An expert's rows do not depend on the other experts or on where its rows start."""
    from collective_communication_mpi_amd.ops import grouped_gemm_nt

    x, w, counts, cap, N, K, _ = _data(name)
    cnt = _cnt(counts)
    full = grouped_gemm_nt(x, w, cnt, out_dtype=out_dtype).clone()
    for _ in range(3):
        again = grouped_gemm_nt(x, w, cnt, out_dtype=out_dtype)
        assert torch.equal(again[:sum(counts)], full[:sum(counts)]), "repeated launches differ"
    for g, (a, b) in enumerate(_bounds(counts, cap)):
        if a == b:
            continue
        alone = grouped_gemm_nt(x[a:b], w[g:g + 1], _cnt([b - a]), out_dtype=out_dtype)
        assert torch.equal(alone, full[a:b]), f"expert {g} differs from a G = 1 call on its slice"


def test_single_expert_is_the_dense_128_tile_bit_for_bit():
    """One expert that owns every row runs the dense 128x128 kernel's loop on the same
    operand order (csrc/device/gemm_tile128.hpp), so the results are equal bit for bit.
    Forward at K % 64 == 0 only: for other K the dense kernel uses the unpermuted
    staged-epilogue form by design."""
    from collective_communication_mpi_amd import _native
    from collective_communication_mpi_amd.ops import gemm_nt, gemm_tn, grouped_gemm_nt, grouped_gemm_tn

    D = _native.device()
    g = torch.Generator(device="cuda").manual_seed(128128)
    D.gemm_set_kernel(1)
    try:
        # two row tiles and two column tiles with masked tails; an even and an odd number of K tiles
        for cap, N, K in [(200, 136, 128), (200, 136, 192)]:
            x = torch.randn(cap, K, device="cuda", generator=g).bfloat16()
            w = torch.randn(N, K, device="cuda", generator=g).bfloat16()
            for dt in (torch.float32, torch.bfloat16):
                got = grouped_gemm_nt(x, w[None], _cnt([cap]), out_dtype=dt)
                assert torch.equal(got, gemm_nt(x, w, out_dtype=dt)), f"forward {(cap, N, K)} {dt}"
        bias = torch.randn(N, device="cuda", generator=g)
        got = grouped_gemm_nt(x, w[None], _cnt([cap]), bias=bias[None], out_dtype=torch.float32)
        assert torch.equal(got, gemm_nt(x, w, bias=bias, out_dtype=torch.float32)), "forward with an fp32 bias"
        D.gemm_tn_set_prefetch(2)
        # 4 row tiles, the last with 8 valid rows; 5 tiles, an odd count for the two-in-flight loop
        for rows, N, K in [(200, 136, 72), (320, 128, 72)]:
            dy = torch.randn(rows, N, device="cuda", generator=g).bfloat16()
            x = torch.randn(rows, K, device="cuda", generator=g).bfloat16()
            got = grouped_gemm_tn(dy, x, _cnt([rows]))[0]
            assert torch.equal(got, gemm_tn(dy, x, splitk=1)), f"weight gradient {(rows, N, K)}"
    finally:
        D.gemm_tn_set_prefetch(0)
        D.gemm_set_kernel(0)


def test_overflow():
    """counts = [100, 100, 100] on a 250-row view of 300 rows: the third expert is truncated
    to 50 rows and nothing at or past row 250 is read or written, forward, dX and dW."""
    from collective_communication_mpi_amd.ops import grouped_gemm_nt, grouped_gemm_tn, transpose

    N, K, G, cap = 136, 72, 3, 250
    counts = [100, 100, 100]
    g = torch.Generator(device="cuda").manual_seed(77)
    x_all = torch.randn(300, K, device="cuda", generator=g).bfloat16()
    dy_all = torch.randn(300, N, device="cuda", generator=g).bfloat16()
    x_all[cap:] = float("nan")          # a read past the view would poison the results
    dy_all[cap:] = float("nan")
    w = torch.randn(G, N, K, device="cuda", generator=g).bfloat16()
    x, dy, cnt = x_all[:cap], dy_all[:cap], _cnt(counts)
    for dt in (torch.float32, torch.bfloat16):
        out_all = torch.full((300, N), SENTINEL, dtype=dt, device="cuda")
        grouped_gemm_nt(x, w, cnt, out=out_all[:cap])
        torch.testing.assert_close(out_all[:cap].float(), _ref_fwd(x, w, counts, cap), **_tol(dt, K))
        assert torch.equal(out_all[cap:], torch.full_like(out_all[cap:], SENTINEL)), "guard rows of out written"
    # dX = dy . w[g]: the forward kernel on the [G, K, N] view of one transposed copy
    wt = transpose(w.view(G * N, K)).view(K, G, N).permute(1, 0, 2)
    dx_all = torch.full((300, K), SENTINEL, dtype=torch.bfloat16, device="cuda")
    grouped_gemm_nt(dy, wt, cnt, out=dx_all[:cap])
    ref_dx = torch.cat([dy[a:b].float() @ w[e].float() for e, (a, b) in enumerate(_bounds(counts, cap))])
    torch.testing.assert_close(dx_all[:cap].float(), ref_dx, **_tol(torch.bfloat16, N))
    assert torch.equal(dx_all[cap:], torch.full_like(dx_all[cap:], SENTINEL)), "guard rows of dx written"
    dw = grouped_gemm_tn(dy, x, cnt)
    ref_dw = torch.stack([dy[a:b].float().T @ x[a:b].float() for a, b in _bounds(counts, cap)])
    torch.testing.assert_close(dw, ref_dw, rtol=2e-3, atol=2e-3 * 100 ** 0.5)


@pytest.mark.parametrize("name", ["mixed", "random"])
def test_int32_and_int64_counts_give_the_same_bits(name):
    from collective_communication_mpi_amd.ops import grouped_gemm_nt, grouped_gemm_tn

    x, w, counts, cap, N, K, _ = _data(name)
    total = sum(counts)
    a = grouped_gemm_nt(x, w, _cnt(counts, torch.int32), out_dtype=torch.float32)
    b = grouped_gemm_nt(x, w, _cnt(counts, torch.int64), out_dtype=torch.float32)
    assert torch.equal(a[:total], b[:total])
    dy = a[:, :N].bfloat16()
    dy[total:] = 0
    assert torch.equal(grouped_gemm_tn(dy, x, _cnt(counts, torch.int32)), grouped_gemm_tn(dy, x, _cnt(counts, torch.int64)))


@pytest.mark.parametrize("N,K", [(136, 72), (128, 256)])
@pytest.mark.parametrize("name", list(CASES))
def test_weight_gradient_masks_at_the_load(name, N, K):
    """dw[g] = dy[rows of g]^T x[rows of g].  Every row outside the expert under test, and
    every row past the total, holds NaN in both operands: a kernel that multiplied such rows
    into a value it discards, or read past the expert's end, would return NaN."""
    from collective_communication_mpi_amd.ops import grouped_gemm_tn

    counts, spare = CASES[name][0], CASES[name][1]
    G, total = len(counts), sum(counts)
    cap = total + spare
    g = torch.Generator(device="cuda").manual_seed(5000 + G + N + K)
    dy = torch.randn(cap, N, device="cuda", generator=g).bfloat16()
    x = torch.randn(cap, K, device="cuda", generator=g).bfloat16()
    bounds = _bounds(counts, cap)
    ref = torch.stack([dy[a:b].float().T @ x[a:b].float() for a, b in bounds])
    tol = dict(rtol=2e-3, atol=2e-3 * max(counts) ** 0.5)
    cnt = _cnt(counts)
    # rows past the total NaN, every expert in one call
    dyn, xn = dy.clone(), x.clone()
    dyn[total:] = float("nan")
    xn[total:] = float("nan")
    out = torch.full((G, N, K), float("nan"), device="cuda")
    assert grouped_gemm_tn(dyn, xn, cnt, out=out) is out
    assert not torch.isnan(out).any()
    torch.testing.assert_close(out, ref, **tol)
    for e, (a, b) in enumerate(bounds):
        if a == b:
            assert out[e].abs().max().item() == 0, f"empty expert {e} is not exactly zero"
    # per expert: NaN in every row that is not its own
    for e, (a, b) in enumerate(bounds):
        dyn.fill_(float("nan"))
        xn.fill_(float("nan"))
        dyn[a:b] = dy[a:b]
        xn[a:b] = x[a:b]
        got = grouped_gemm_tn(dyn, xn, cnt)[e]
        assert not torch.isnan(got).any(), f"expert {e}: rows outside it reached the result"
        assert torch.equal(got, out[e]), f"expert {e} depends on the other experts' rows"
    assert torch.equal(grouped_gemm_tn(dy, x, cnt, alpha=2.0), 2 * grouped_gemm_tn(dy, x, cnt))


def test_grouped_linear_gradients():
    """dX and dW of grouped_linear against torch autograd on the per-expert loop."""
    from collective_communication_mpi_amd.ops import grouped_linear

    x0, w0, counts, cap, N, K, _ = _data("mixed")
    total, cnt = sum(counts), _cnt(counts)
    dy = torch.randn(cap, N, device="cuda", generator=torch.Generator(device="cuda").manual_seed(9)).bfloat16()
    xr = x0.float().requires_grad_()
    wr = w0.float().requires_grad_()
    yr = torch.cat([xr[a:b] @ wr[e].T for e, (a, b) in enumerate(_bounds(counts, cap))])
    yr.backward(dy[:total].float())

    # fp32 master weights (bf16-representable here): the weight gradient stays fp32
    x = x0.clone().requires_grad_()
    w32 = w0.float().requires_grad_()
    y = grouped_linear(x, w32, cnt)
    assert y.dtype == torch.bfloat16 and cnt.grad is None
    torch.testing.assert_close(y[:total].float(), yr.detach(), **_tol(torch.bfloat16, K))
    y.backward(dy)
    assert w32.grad.dtype == torch.float32 and x.grad.dtype == torch.bfloat16
    torch.testing.assert_close(x.grad[:total].float(), xr.grad[:total], **_tol(torch.bfloat16, N))
    torch.testing.assert_close(w32.grad, wr.grad, rtol=2e-3, atol=2e-3 * max(counts) ** 0.5)
    assert w32.grad[0].abs().max().item() == 0          # the empty expert

    # bf16 weights: the same kernels, the weight gradient rounded once
    xb = x0.clone().requires_grad_()
    wb = w0.clone().requires_grad_()
    grouped_linear(xb, wb, cnt).backward(dy)
    assert wb.grad.dtype == torch.bfloat16
    assert torch.equal(wb.grad, w32.grad.bfloat16()) and torch.equal(xb.grad[:total], x.grad[:total])


def test_graph_replay_reads_new_counts():
    """One captured launch, a fixed device counts tensor rewritten between replays."""
    from collective_communication_mpi_amd.ops import grouped_gemm_nt

    G, cap, N, K = 4, 600, 136, 64
    vectors = [[0, 150, 100, 50], [200, 0, 128, 129], [1, 1, 1, 300]]   # expert 0: 0 -> 200 rows
    g = torch.Generator(device="cuda").manual_seed(31)
    x = torch.randn(cap, K, device="cuda", generator=g).bfloat16()
    w = torch.randn(G, N, K, device="cuda", generator=g).bfloat16()
    cnt = _cnt([5, 5, 5, 5])
    out = torch.full((cap, N), SENTINEL, dtype=torch.float32, device="cuda")
    grouped_gemm_nt(x, w, cnt, out=out)       # warm-up outside the capture
    torch.cuda.synchronize()
    cs = torch.cuda.Stream()
    cs.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(cs):
        with torch.cuda.graph(graph, stream=cs):
            grouped_gemm_nt(x, w, cnt, out=out)
    torch.cuda.current_stream().wait_stream(cs)
    for counts in vectors:
        cnt.copy_(_cnt(counts))
        out.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        total = sum(counts)
        torch.testing.assert_close(out[:total], _ref_fwd(x, w, counts, cap), **_tol(torch.float32, K))
        assert torch.equal(out[total:], torch.full_like(out[total:], SENTINEL))
    del graph
