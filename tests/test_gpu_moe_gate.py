"""Fused top-k router (csrc/device/moe_gate.hip, ``ops.moe_gate``) on one GPU.

Inputs: logits ``3 * randn`` [T, E]; every second row rounded to multiples of 0.5, so equal
logits occur (asserted from the inputs alone: in at least one row the K-th and the (K + 1)-th
largest logit are equal); where E > K + 1 the last row is -inf in all but K + 1 places, and
the row before it has only max(1, K - 1) finite logits, so experts of probability 0 are
selected there, the lowest indices first.

Exact checks: ``idx`` equals the first K entries of a stable sort by (-logit, index) made on
the CPU, ``expert_tokens`` a bincount of it, two calls give the same bits (``prob_sum``
included), and a captured graph of the raw forward + backward replayed with new logits gives
the bits of the eager call.

``weights``, ``prob_sum`` and ``dlogits`` (autograd with random ``dweights`` and ``dprob_sum``)
are compared against the same composition -- softmax, gather on the fixed ``idx``,
renormalise, sum over tokens -- in fp64.  The tolerance is not a fixed number: per tensor it is
8 x the largest absolute error the fp32 torch composition itself makes against fp64 on that
input (measured here, on the device), with a floor of 2^-22 x the largest reference magnitude
for tensors that come out exact; the factor 8 pays for a different exp and summation order.
The worst error / tolerance ratio is printed; measured values are in profiles/moe/README.md."""
import pytest
import torch

from collective_communication_mpi_amd import ops
from collective_communication_mpi_amd.ops.kernels import MOE_GATE_CHUNK

pytestmark = pytest.mark.gpu

SHAPES = [(0, 8, 2), (1, 1, 1), (5, 8, 8), (67, 64, 2), (130, 96, 8), (MOE_GATE_CHUNK + 1, 256, 8)]
FLOOR = 2.0 ** -22


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _logits(T, E, K, salt=0):
    g = torch.Generator(device="cuda").manual_seed(9001 + 131 * T + 17 * E + K + 7919 * salt)
    x = 3 * torch.randn(T, E, device="cuda", generator=g)
    x[0::2] = torch.round(x[0::2] * 2) / 2
    if E > K + 1 and T >= 3:
        for row, finite in ((T - 1, K + 1), (T - 2, max(1, K - 1))):
            keep = torch.randperm(E, device="cuda", generator=g)[:finite]
            masked = torch.full((E,), float("-inf"), device="cuda")
            masked[keep] = x[row, keep]
            x[row] = masked
    return x.contiguous()


def _compose(logits, idx, dw, dps, renorm, dtype):
    """(weights, prob_sum, dlogits) of the torch composition in ``dtype`` on the fixed idx."""
    x = logits.detach().to(dtype, copy=True).requires_grad_()
    p = torch.softmax(x, dim=-1)
    w = p.gather(1, idx)
    if renorm:
        w = w / w.sum(dim=-1, keepdim=True)
    ps = p.sum(dim=0)
    ((w * dw.to(dtype)).sum() + (ps * dps.to(dtype)).sum()).backward()
    return w.detach(), ps.detach(), x.grad


_DATA = {}


def _data(shape):
    """(logits, expected idx, dweights, dprob_sum): made once per shape, never written."""
    if shape not in _DATA:
        T, E, K = shape
        x = _logits(T, E, K)
        want = torch.sort(-x.cpu(), dim=1, stable=True).indices[:, :K].cuda()
        g = torch.Generator(device="cuda").manual_seed(77 + T + E)
        dw = torch.randn(T, K, device="cuda", generator=g)
        dps = torch.randn(E, device="cuda", generator=g)
        _DATA[shape] = (x, want, dw, dps)
    return _DATA[shape]


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[1] > s[2] + 1 and s[0] >= 3], ids=str)
def test_inputs_have_a_tie_across_the_kth_place(shape):
    x, _, _, _ = _data(shape)
    K = shape[2]
    s = torch.sort(x, dim=1, descending=True).values
    tie = (s[:, K - 1] == s[:, K]) & torch.isfinite(s[:, K])
    assert tie.any(), "no row whose K-th and (K + 1)-th largest logits are equal"
    assert (torch.isinf(s[-1]).sum().item(), torch.isinf(s[-2]).sum().item()) == \
        (shape[1] - K - 1, shape[1] - max(1, K - 1))


@pytest.mark.parametrize("renorm", [True, False], ids=["renorm", "raw"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_gate_against_fp64(shape, renorm):
    T, E, K = shape
    x, want_idx, dw, dps = _data(shape)
    xg = x.clone().requires_grad_()
    w, idx, ps, tokens = ops.moe_gate(xg, K, renorm)
    assert w.shape == (T, K) and idx.shape == (T, K) and ps.shape == (E,) and tokens.shape == (E,)
    assert (w.dtype, idx.dtype, ps.dtype, tokens.dtype) == (torch.float32, torch.int32, torch.float32, torch.int64)
    assert torch.equal(idx.long(), want_idx), "idx is not the stable sort by (-logit, index)"
    assert torch.equal(tokens, torch.bincount(want_idx.reshape(-1), minlength=E))
    ((w * dw).sum() + (ps * dps).sum()).backward()
    assert xg.grad is not None and xg.grad.shape == x.shape
    if T == 0:
        assert ps.abs().max().item() == 0 and tokens.sum().item() == 0
        return
    ref = _compose(x, want_idx, dw, dps, renorm, torch.float64)
    f32 = _compose(x, want_idx, dw, dps, renorm, torch.float32)
    worst = 0.0
    for name, got, r64, r32 in zip(("weights", "prob_sum", "dlogits"), (w.detach(), ps.detach(), xg.grad), ref, f32):
        assert torch.isfinite(got).all(), name
        own = (r32.double() - r64).abs().max().item()
        tol = max(8 * own, FLOOR * r64.abs().max().item())
        err = (got.double() - r64).abs().max().item()
        ratio = err / tol if tol > 0 else (0.0 if err == 0 else float("inf"))
        print(f"moe_gate {shape} renorm={renorm} {name}: error {err:.3e}, fp32 torch error {own:.3e}, "
              f"tolerance {tol:.3e}, error / tolerance {ratio:.3f}")
        worst = max(worst, ratio)
        assert err <= tol, f"{name}: error {err:.3e} > tolerance {tol:.3e} (fp32 torch error {own:.3e})"
    print(f"moe_gate {shape} renorm={renorm}: worst error / tolerance {worst:.3f}")
    # masked experts: probability and gradient exactly 0
    dead = torch.isinf(x)
    if dead.any():
        assert xg.grad[dead].abs().max().item() == 0
        assert w.detach()[dead.gather(1, want_idx)].abs().max().item() == 0


@pytest.mark.parametrize("shape", [(130, 96, 8)], ids=str)
def test_gradient_through_the_weights_alone(shape):
    """No gradient for prob_sum: the backward runs without dprob_sum."""
    T, E, K = shape
    x, want_idx, dw, _ = _data(shape)
    xg = x.clone().requires_grad_()
    w, _, _, _ = ops.moe_gate(xg, K, True)
    (w * dw).sum().backward()
    zero = torch.zeros(E, device="cuda")
    _, _, r64 = _compose(x, want_idx, dw, zero, True, torch.float64)
    _, _, r32 = _compose(x, want_idx, dw, zero, True, torch.float32)
    tol = max(8 * (r32.double() - r64).abs().max().item(), FLOOR * r64.abs().max().item())
    assert (xg.grad.double() - r64).abs().max().item() <= tol
    raw = ops.moe_gate_backward(x, want_idx.int(), dw, None, True)
    assert torch.equal(raw, xg.grad)


@pytest.mark.parametrize("shape", SHAPES[2:], ids=str)
def test_two_calls_give_the_same_bits(shape):
    T, E, K = shape
    x, _, dw, dps = _data(shape)
    a = ops.moe_gate_forward(x, K, True)
    b = ops.moe_gate_forward(x.clone(), K, True)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    da = ops.moe_gate_backward(x, a[1], dw, dps, True)
    db = ops.moe_gate_backward(x.clone(), b[1], dw, dps, True)
    assert torch.equal(da, db)


def test_graph_replay_with_new_logits():
    T, E, K = MOE_GATE_CHUNK + 1, 256, 8
    x, _, dw, dps = _data((T, E, K))
    news = [_logits(T, E, K, salt=s) for s in (1, 2)]
    want = []
    for n in news:
        out = ops.moe_gate_forward(n, K, True)
        want.append((*out, ops.moe_gate_backward(n, out[1], dw, dps, True)))
    static = x.clone()
    cs = torch.cuda.Stream()
    cs.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(cs):
        with torch.cuda.graph(g, stream=cs):
            out = ops.moe_gate_forward(static, K, True)
            dl = ops.moe_gate_backward(static, out[1], dw, dps, True)
    torch.cuda.current_stream().wait_stream(cs)
    for n, w in zip(news, want):
        static.copy_(n)
        g.replay()
        torch.cuda.synchronize()
        for got, exp in zip((*out, dl), w):
            assert torch.equal(got, exp)
    del g
