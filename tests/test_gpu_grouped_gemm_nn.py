"""Grouped dX kernel ``grouped_gemm_nn`` (csrc/device/grouped_gemm.hip, nn_loop of
gemm_tile128.hpp) on one GPU against the per-expert ``dy[rows].float() @ w[g].float()`` loop
in torch: both output dtypes with sentinel rows, an identity ``dy`` (a transposed or
column-permuted store), NaN behind both operands' reduction tails and outside an expert's
rows, isolation of an expert (bitwise), counts that overflow the buffer, int32 / int64
counts, the transposed-copy route of the parent, a captured graph replayed with new counts,
and the peak memory of one ``grouped_linear`` backward.

Tolerances are those of tests/test_gpu_grouped_gemm.py for the same tile and randn inputs,
R the reduction length (here N): fp32 rtol 2e-3, atol 2e-3 sqrt(R); bf16 rtol 2e-2, atol 8e-2."""
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


_LIMIT = [1 if g % 7 else 0 for g in range(256)]

#        name       counts               spare  N (reduction)  K (columns)
CASES = {
    "edge": ([130], 0, 72, 72),
    "mixed_dma": ([0, 1, 127, 129], 43, 64, 136),
    "mixed_regs": ([0, 1, 127, 129], 43, 136, 64),
    "exact2": ([128, 0, 0, 256, 3], 0, 128, 192),
    "exact3": ([128, 0, 0, 256, 3], 0, 192, 128),
    "random": (_random_counts(), 17, 520, 264),
    "limit": (_LIMIT, 256 - sum(_LIMIT), 64, 64),
}


def _bounds(counts, cap):
    e = np.minimum(np.cumsum([0] + [max(int(c), 0) for c in counts]), cap)
    return [(int(e[g]), int(e[g + 1])) for g in range(len(counts))]


def _ref(dy, w, counts, cap):
    """fp32 reference of the rows in [0, min(total, cap))."""
    return torch.cat([dy[a:b].float() @ w[g].float() for g, (a, b) in enumerate(_bounds(counts, cap))])


_DATA = {}


def _data(name):
    """(dy, w, counts list, cap, N, K, fp32 reference): made once per case, never written."""
    if name not in _DATA:
        counts, spare, N, K = CASES[name]
        cap = sum(counts) + spare
        g = torch.Generator(device="cuda").manual_seed(2000 + len(name) * 31 + N + K)
        dy = torch.randn(cap, N, device="cuda", generator=g).bfloat16()
        w = torch.randn(len(counts), N, K, device="cuda", generator=g).bfloat16()
        _DATA[name] = (dy, w, counts, cap, N, K, _ref(dy, w, counts, cap))
    return _DATA[name]


def _tol(dtype, R):
    return dict(rtol=2e-3, atol=2e-3 * R ** 0.5) if dtype == torch.float32 else dict(rtol=2e-2, atol=8e-2)


def _cnt(counts, dtype=torch.int64):
    return torch.tensor(counts, dtype=dtype, device="cuda")


def test_case_table_is_the_one_asked_for():
    assert sum(CASES["mixed_dma"][0]) + CASES["mixed_dma"][1] == 300 and sum(CASES["exact2"][0]) == 387
    assert sum(CASES["limit"][0]) + CASES["limit"][1] == 256 and len(CASES["limit"][0]) == 256
    rc = CASES["random"][0]
    assert len(rc) == 8 and min(rc) == 0 and max(rc) == 300 and CASES["random"][1:] == (17, 520, 264)


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", list(CASES))
def test_forward(name, out_dtype):
    from collective_communication_mpi_amd.ops import grouped_gemm_nn

    dy, w, counts, cap, N, K, ref = _data(name)
    total = sum(counts)
    out = torch.full((cap, K), SENTINEL, dtype=out_dtype, device="cuda")
    got = grouped_gemm_nn(dy, w, _cnt(counts), out=out)
    assert got is out
    torch.testing.assert_close(out[:total].float(), ref, **_tol(out_dtype, N))
    assert torch.equal(out[total:], torch.full_like(out[total:], SENTINEL)), "rows past the total were written"


@pytest.mark.parametrize("K", [64, 136])
def test_identity_rows_return_the_weights(K):
    """dy = identity: out is w[0] itself, exactly.  A transposed or column-permuted store, or
    fragments whose reduction elements are paired in another order, cannot pass."""
    from collective_communication_mpi_amd.ops import grouped_gemm_nn

    N = 64
    dy = torch.eye(N, device="cuda").bfloat16()
    # asymmetric and exactly representable in bf16: w[n, k] = n - 2 k (|.| < 2^8)
    w = (torch.arange(N, device="cuda")[:, None] - 2.0 * torch.arange(K, device="cuda")[None, :]).bfloat16()[None]
    assert not torch.equal(w[0, :, :N], w[0, :, :N].T)
    for dt in (torch.float32, torch.bfloat16):
        out = grouped_gemm_nn(dy, w.contiguous(), _cnt([N]), out_dtype=dt)
        assert torch.equal(out.float(), w[0].float()), f"{dt}"
    g = torch.Generator(device="cuda").manual_seed(64 + K)
    wr = torch.randn(1, N, K, device="cuda", generator=g).bfloat16()
    assert torch.equal(grouped_gemm_nn(dy, wr, _cnt([N])), wr[0])


@pytest.mark.parametrize("N", [72, 136])
def test_masking_of_b(N):
    """Rows N .. N + 7 behind every expert's weights are NaN, and the last expert's weights end
    a buffer whose next rows are NaN: the reduction tail must contribute exactly nothing."""
    from collective_communication_mpi_amd.ops import grouped_gemm_nn

    counts, K = [70, 0, 130, 5], 136
    G, cap = len(counts), sum(counts) + 3
    g = torch.Generator(device="cuda").manual_seed(300 + N)
    dy = torch.randn(cap, N, device="cuda", generator=g).bfloat16()
    w_all = torch.randn(G, N + 8, K, device="cuda", generator=g).bfloat16()
    w_all[:, N:] = float("nan")
    cnt = _cnt(counts)
    want = grouped_gemm_nn(dy, w_all[:, :N].contiguous(), cnt, out_dtype=torch.float32)
    got = grouped_gemm_nn(dy, w_all[:, :N], cnt, out_dtype=torch.float32)
    total = sum(counts)
    assert not torch.isnan(got[:total]).any(), "rows behind an expert's weights reached the result"
    assert torch.equal(got[:total], want[:total])
    torch.testing.assert_close(got[:total], _ref(dy, w_all[:, :N], counts, cap), **_tol(torch.float32, N))
    # the last expert's weights as the tail of a buffer, NaN rows right behind them
    buf = torch.full((G * N + 64, K), float("nan"), dtype=torch.bfloat16, device="cuda")
    buf[:G * N] = w_all[:, :N].reshape(G * N, K)
    got = grouped_gemm_nn(dy, buf[:G * N].view(G, N, K), cnt, out_dtype=torch.float32)
    assert not torch.isnan(got[:total]).any(), "rows behind the last expert's weights reached the result"
    assert torch.equal(got[:total], want[:total])


@pytest.mark.parametrize("name", ["edge", "mixed_regs", "mixed_dma"])
def test_masking_of_a(name):
    """dy is a view of a buffer with 8 NaN columns behind every row; rows at or past the total
    are NaN; then, per expert, every row outside it is NaN."""
    from collective_communication_mpi_amd.ops import grouped_gemm_nn

    dy, w, counts, cap, N, K, ref = _data(name)
    total, cnt = sum(counts), _cnt(counts)
    full = grouped_gemm_nn(dy, w, cnt, out_dtype=torch.float32)
    dy_all = torch.full((cap, N + 8), float("nan"), dtype=torch.bfloat16, device="cuda")
    dy_all[:total, :N] = dy[:total]
    got = grouped_gemm_nn(dy_all[:, :N], w, cnt, out_dtype=torch.float32)
    assert not torch.isnan(got[:total]).any(), "memory past column N of dy, or a row past the total, reached the result"
    assert torch.equal(got[:total], full[:total])
    for e, (a, b) in enumerate(_bounds(counts, cap)):
        if a == b:
            continue
        dy_all.fill_(float("nan"))
        dy_all[a:b, :N] = dy[a:b]
        got = grouped_gemm_nn(dy_all[:, :N], w, cnt, out_dtype=torch.float32)
        assert not torch.isnan(got[a:b]).any(), f"expert {e}: rows outside it reached the result"
        assert torch.equal(got[a:b], full[a:b]), f"expert {e} depends on the other experts' rows"


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", ["mixed_regs", "random"])
def test_isolation(name, out_dtype):
    """An expert's rows do not depend on the other experts or on where its rows start."""
    from collective_communication_mpi_amd.ops import grouped_gemm_nn

    dy, w, counts, cap, N, K, _ = _data(name)
    cnt = _cnt(counts)
    full = grouped_gemm_nn(dy, w, cnt, out_dtype=out_dtype).clone()
    for _ in range(3):
        again = grouped_gemm_nn(dy, w, cnt, out_dtype=out_dtype)
        assert torch.equal(again[:sum(counts)], full[:sum(counts)]), "repeated launches differ"
    for g, (a, b) in enumerate(_bounds(counts, cap)):
        if a == b:
            continue
        alone = grouped_gemm_nn(dy[a:b], w[g:g + 1], _cnt([b - a]), out_dtype=out_dtype)
        assert torch.equal(alone, full[a:b]), f"expert {g} differs from a G = 1 call on its slice"


def test_overflow():
    """counts = [100, 100, 100] on a 250-row view of 300 rows: the third expert is truncated
    to 50 rows and nothing at or past row 250 is read or written."""
    from collective_communication_mpi_amd.ops import grouped_gemm_nn

    N, K, G, cap = 136, 72, 3, 250
    counts = [100, 100, 100]
    g = torch.Generator(device="cuda").manual_seed(78)
    dy_all = torch.randn(300, N, device="cuda", generator=g).bfloat16()
    dy_all[cap:] = float("nan")          # a read past the view would poison the results
    w = torch.randn(G, N, K, device="cuda", generator=g).bfloat16()
    dy, cnt = dy_all[:cap], _cnt(counts)
    for dt in (torch.float32, torch.bfloat16):
        out_all = torch.full((300, K), SENTINEL, dtype=dt, device="cuda")
        grouped_gemm_nn(dy, w, cnt, out=out_all[:cap])
        torch.testing.assert_close(out_all[:cap].float(), _ref(dy, w, counts, cap), **_tol(dt, N))
        assert torch.equal(out_all[cap:], torch.full_like(out_all[cap:], SENTINEL)), "guard rows of out written"


@pytest.mark.parametrize("name", ["mixed_regs", "random"])
def test_counts_dtype_and_alpha(name):
    from collective_communication_mpi_amd.ops import grouped_gemm_nn

    dy, w, counts, cap, N, K, _ = _data(name)
    total = sum(counts)
    a = grouped_gemm_nn(dy, w, _cnt(counts, torch.int32), out_dtype=torch.float32)
    b = grouped_gemm_nn(dy, w, _cnt(counts, torch.int64), out_dtype=torch.float32)
    assert torch.equal(a[:total], b[:total])
    c = grouped_gemm_nn(dy, w, _cnt(counts), alpha=2.0, out_dtype=torch.float32)
    assert torch.equal(c[:total], 2 * a[:total])


def test_against_the_transposed_copy_route():
    """The parent's dX: the forward kernel on the [G, K, N] view of one transposed copy."""
    from collective_communication_mpi_amd.ops import grouped_gemm_nn, grouped_gemm_nt
    from collective_communication_mpi_amd.ops.kernels import _transposed_experts

    dy, w, counts, cap, N, K, _ = _data("random")
    total, cnt = sum(counts), _cnt(counts)
    new = grouped_gemm_nn(dy, w, cnt, out_dtype=torch.float32)
    old = grouped_gemm_nt(dy, _transposed_experts(w), cnt, out_dtype=torch.float32)
    torch.testing.assert_close(new[:total], old[:total], **_tol(torch.float32, N))


def test_graph_replay_reads_new_counts():
    """One captured launch, a fixed device counts tensor rewritten between replays."""
    from collective_communication_mpi_amd.ops import grouped_gemm_nn

    G, cap, N, K = 4, 600, 64, 136
    vectors = [[0, 150, 100, 50], [200, 0, 128, 129], [1, 1, 1, 300]]   # expert 0: 0 -> 200 rows
    g = torch.Generator(device="cuda").manual_seed(32)
    dy = torch.randn(cap, N, device="cuda", generator=g).bfloat16()
    w = torch.randn(G, N, K, device="cuda", generator=g).bfloat16()
    cnt = _cnt([5, 5, 5, 5])
    out = torch.full((cap, K), SENTINEL, dtype=torch.float32, device="cuda")
    grouped_gemm_nn(dy, w, cnt, out=out)       # warm-up outside the capture
    torch.cuda.synchronize()
    cs = torch.cuda.Stream()
    cs.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(cs):
        with torch.cuda.graph(graph, stream=cs):
            grouped_gemm_nn(dy, w, cnt, out=out)
    torch.cuda.current_stream().wait_stream(cs)
    for counts in vectors:
        cnt.copy_(_cnt(counts))
        out.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        total = sum(counts)
        torch.testing.assert_close(out[:total], _ref(dy, w, counts, cap), **_tol(torch.float32, N))
        assert torch.equal(out[total:], torch.full_like(out[total:], SENTINEL))
    del graph


def _backward_peak(monkeypatch, route, w_grad):
    """Peak allocation of one grouped_linear backward above the level before it, less the
    tensors every route has to return: dx, and the fp32 dw where the weights ask for one.

    The transposed copy lives only while dX is computed and is freed before dW (twice its
    size, fp32) is allocated, so with a weight gradient the backward's peak is dx + dw on
    either route and says nothing about the copy; the copy shows in the peak of a backward
    that computes dX alone (``w_grad`` False), which is where the two routes are told apart."""
    from collective_communication_mpi_amd.ops import grouped_linear

    G, N, K, cap = 4, 256, 512, 64
    if route is None:
        monkeypatch.delenv("CCMPI_GROUPED_DX", raising=False)
    else:
        monkeypatch.setenv("CCMPI_GROUPED_DX", route)
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn(cap, K, device="cuda", generator=g).bfloat16().requires_grad_()
    w = (torch.randn(G, N, K, device="cuda", generator=g) / K ** 0.5).requires_grad_(w_grad)   # fp32 master weights
    cnt = _cnt([16, 0, 40, 8])
    dy = torch.randn(cap, N, device="cuda", generator=g).bfloat16()
    grouped_linear(x, w, cnt).backward(dy)     # warm-up: kernels loaded
    x.grad = w.grad = None
    y = grouped_linear(x, w, cnt)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    y.backward(dy)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    accounted = x.numel() * 2 + (w.numel() * 4 if w_grad else 0)   # dx, dw (dy was there before)
    print(f"route {route or 'default'}, dw {w_grad}: peak {peak} B, dx + dw {accounted} B, a copy of w {w.numel() * 2} B")
    return peak - accounted, w.numel() * 2


@pytest.mark.parametrize("w_grad", [True, False], ids=["dx_dw", "dx_only"])
def test_grouped_linear_backward_makes_no_copy_of_the_weights(monkeypatch, w_grad):
    extra, copy = _backward_peak(monkeypatch, None, w_grad)
    assert extra < copy, "the backward allocated as much as a second copy of the weights"


def test_transpose_route_still_makes_the_copy(monkeypatch):
    extra, copy = _backward_peak(monkeypatch, "transpose", False)
    assert extra >= copy, "CCMPI_GROUPED_DX=transpose did not select the transposed-copy route"
