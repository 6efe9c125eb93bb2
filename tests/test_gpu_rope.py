"""Rotary position embedding on the GPU (``ops.rope_apply`` / ``ops.rope``, csrc/device/rope.hip).

Accuracy: against ``ops.rope_reference`` (fp64) on the same bf16 inputs and the same fp32 table
every element satisfies ``|got - exact| <= 2^-8 |exact| + 2^-22 (|x1| + |x2|)``: bf16's unit roundoff
for the single rounding, plus two fp32 products and one add with a factor of two to spare.
Bitwise: position 0 is the identity; in place = out of place; q and k in one launch = two launches;
a chunk with ``pos0 = a`` = those rows of the whole call; a packed sequence = the batched call on it
alone; interleaved = half-split on the de-interleaved input; two calls agree; autograd = raw.
Adjoint, framed views, clamped boundaries, a table shorter than a document, 64-bit strides, graph
replay and refusals follow, then the model."""
import functools

import pytest
import torch

from collective_communication_mpi_amd import _native, ops

pytestmark = pytest.mark.gpu

DIMS = (16, 64, 80, 128)  # 80: 5 slices per head, not a power of two
HEADS = ((1, 1), (4, 2), (3, 5))
LENGTHS = (1, 3, 129, 257)
BATCHES = (1, 2)
STARTS = (0, 1, 1000)
P = 1300  # table rows: 1000 + 257 fit
PACKINGS = {"empty middle": [0, 3, 3, 200], "one token each": [0, 1, 2, 3], "one document": [0, 200],
            "empty first": [0, 0, 70, 200]}
SENTINEL = -7.0
BF = torch.bfloat16


@functools.lru_cache(maxsize=None)
def _table(D, rows=P):
    return ops.rope_table(rows, D, device="cuda")


def _randn(*shape, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(*shape, device="cuda", generator=g).to(BF)


@functools.lru_cache(maxsize=None)
def _inputs(lead, Hq, Hkv, D, salt=0):
    """q [*lead, Hq, D], k [*lead, Hkv, D]; shared between tests and never written."""
    seed = 7 + 1000003 * salt + 131 * sum(lead) + 17 * Hq + 3 * Hkv + D
    return _randn(*lead, Hq, D, seed=seed), _randn(*lead, Hkv, D, seed=seed + 1)


def _cu(bounds):
    return torch.tensor(bounds, dtype=torch.int32, device="cuda")


def _pair_sum(x, interleaved):
    """|x1| + |x2| of each element's pair, in the layout of x."""
    x = x.double().abs()
    D = x.shape[-1]
    if interleaved:
        s = x[..., 0::2] + x[..., 1::2]
        return torch.stack((s, s), dim=-1).reshape(x.shape)
    s = x[..., :D // 2] + x[..., D // 2:]
    return torch.cat((s, s), dim=-1)


def _bound(x, exact, interleaved):
    return 2.0 ** -8 * exact.abs() + 2.0 ** -22 * _pair_sum(x, interleaved)


def _ratio(got, x, table, positions, interleaved, inverse):
    """Worst |got - exact| / tolerance over the elements."""
    exact = ops.rope_reference(x, table, positions, interleaved, inverse)
    tol = _bound(x, exact, interleaved)
    err = (got.double() - exact).abs()
    assert (tol > 0).all()  # randn inputs: no pair is (0, 0)
    return (err / tol).max().item()


def _positions(B, S, pos0):
    return (pos0 + torch.arange(S, device="cuda")).repeat(B, 1)


def _packed_positions(bounds, T):
    """Position of every token inside its document, -1 for tokens no document owns."""
    pos = torch.full((T,), -1, dtype=torch.int64)
    for b, e in zip(bounds[:-1], bounds[1:]):
        b, e = min(max(b, 0), T), min(max(e, 0), T)
        if e > b:
            pos[b:e] = torch.arange(e - b)
    return pos.cuda()


# --- accuracy ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("heads", HEADS, ids=lambda h: f"{h[0]}x{h[1]}")
@pytest.mark.parametrize("D", DIMS)
def test_batched_accuracy_and_identity_at_position_zero(D, heads):
    Hq, Hkv = heads
    table = _table(D)
    worst = 0.0
    for S in LENGTHS:
        for B in BATCHES:
            q, k = _inputs((B, S), Hq, Hkv, D)
            for pos0 in STARTS:
                pos = _positions(B, S, pos0)
                for interleaved in (False, True):
                    for inverse in (False, True):
                        qo, ko = ops.rope_apply(q, k, table, pos0, interleaved=interleaved, inverse=inverse)
                        assert qo.shape == q.shape and ko.shape == k.shape and qo.is_contiguous() and ko.is_contiguous()
                        tag = f"S={S} B={B} pos0={pos0} interleaved={interleaved} inverse={inverse}"
                        for name, got, x in (("q", qo, q), ("k", ko, k)):
                            r = _ratio(got, x, table, pos, interleaved, inverse)
                            worst = max(worst, r)
                            assert r <= 1.0, f"{tag} {name}: error is {r:.3f} x the tolerance"
                            if pos0 == 0:  # (a) c = 1, s = 0: the row comes back bit for bit
                                assert torch.equal(got[:, 0], x[:, 0]), f"{tag} {name}: position 0 is not the identity"
    print(f"[rope D={D} heads={Hq}x{Hkv}] worst error / tolerance {worst:.3f}")


@pytest.mark.parametrize("packing", sorted(PACKINGS))
@pytest.mark.parametrize("D", DIMS)
def test_packed_accuracy_and_bitwise_per_sequence(D, packing):
    """(e) every non-empty sequence's rows are bitwise the batched B = 1, pos0 = 0 call on that
    sequence alone; rows no sequence owns keep what the output held."""
    bounds = PACKINGS[packing]
    T = 203 if bounds[-1] == 200 else 5  # a tail of rows [cu[n], T) in both
    table = _table(D)
    worst = 0.0
    for Hq, Hkv in HEADS:
        q, k = _inputs((T,), Hq, Hkv, D)
        pos = _packed_positions(bounds, T)
        owned = pos >= 0
        for interleaved in (False, True):
            for inverse in (False, True):
                qo, ko = torch.full_like(q, SENTINEL), torch.full_like(k, SENTINEL)
                ops.rope_apply(q, k, table, cu_seqlens=_cu(bounds), interleaved=interleaved, inverse=inverse, q_out=qo, k_out=ko)
                for name, got, x in (("q", qo, q), ("k", ko, k)):
                    r = _ratio(got[owned], x[owned], table, pos[owned], interleaved, inverse)
                    worst = max(worst, r)
                    assert r <= 1.0, f"{name}: error is {r:.3f} x the tolerance"
                    assert (got[~owned] == SENTINEL).all(), f"{name}: rows outside every sequence were written"
                for lanes in (1, Hq + Hkv):  # however the heads are dealt to a token's threads
                    ql, kl = torch.full_like(q, SENTINEL), torch.full_like(k, SENTINEL)
                    ops.rope_apply(q, k, table, cu_seqlens=_cu(bounds), interleaved=interleaved, inverse=inverse, q_out=ql,
                                   k_out=kl, _lanes=lanes)
                    assert torch.equal(ql, qo) and torch.equal(kl, ko), f"{lanes} head lanes"
                for b, e in zip(bounds[:-1], bounds[1:]):
                    if e > b:
                        qa, ka = ops.rope_apply(q[None, b:e], k[None, b:e], table, interleaved=interleaved, inverse=inverse)
                        assert torch.equal(qo[b:e], qa[0]) and torch.equal(ko[b:e], ka[0]), f"sequence [{b}, {e})"
                        assert torch.equal(qo[b], q[b]) and torch.equal(ko[b], k[b])  # its first token sits at position 0
    print(f"[rope packed D={D} {packing}] worst error / tolerance {worst:.3f}")


# --- bitwise contracts ---------------------------------------------------------------------------------

CASES = [(64, 4, 2, False), (80, 3, 5, True), (16, 1, 1, False), (128, 4, 2, True)]
CASE_IDS = [f"D{d}-{a}x{b}-{'interleaved' if i else 'half'}" for d, a, b, i in CASES]


@pytest.mark.parametrize("D,Hq,Hkv,interleaved", CASES, ids=CASE_IDS)
def test_bitwise_in_place_one_launch_chunks_and_repeats(D, Hq, Hkv, interleaved):
    B, S, pos0 = 2, 257, 1
    table = _table(D)
    q, k = _inputs((B, S), Hq, Hkv, D)
    for inverse in (False, True):
        kw = dict(interleaved=interleaved, inverse=inverse)
        qo, ko = ops.rope_apply(q, k, table, pos0, **kw)
        # (b) in place
        qc, kc = q.clone(), k.clone()
        r = ops.rope_apply(qc, kc, table, pos0, q_out=qc, k_out=kc, **kw)
        assert r[0] is qc and r[1] is kc
        assert torch.equal(qc, qo) and torch.equal(kc, ko), "in place differs from out of place"
        # (c) one launch against two
        q1, none = ops.rope_apply(q, None, table, pos0, **kw)
        k1, _ = ops.rope_apply(k, None, table, pos0, **kw)
        assert none is None and torch.equal(q1, qo) and torch.equal(k1, ko), "q and k together differ from each alone"
        # (g) again
        q2, k2 = ops.rope_apply(q, k, table, pos0, **kw)
        assert torch.equal(q2, qo) and torch.equal(k2, ko)
        # and however the heads are dealt to a token's threads (more than kRopeInFlight heads per thread at 1 lane)
        for lanes in {1, 2, Hq + Hkv}:
            q3, k3 = ops.rope_apply(q, k, table, pos0, _lanes=lanes, **kw)
            assert torch.equal(q3, qo) and torch.equal(k3, ko), f"{lanes} head lanes"
        # (d) rows [a, a + n) with pos0 = a are those rows of the pos0 = 0 call; the views are read as they are
        q0, k0 = ops.rope_apply(q, k, table, 0, **kw)
        for a, n in ((0, 1), (1, 128), (129, 128), (200, 57)):
            qa, ka = ops.rope_apply(q[:, a:a + n], k[:, a:a + n], table, a, **kw)
            assert torch.equal(qa, q0[:, a:a + n]) and torch.equal(ka, k0[:, a:a + n]), f"chunk [{a}, {a + n})"


@pytest.mark.parametrize("D", DIMS)
def test_bitwise_interleaved_is_half_split_on_deinterleaved_input(D):
    """(f) both pairings go through one device function."""
    Hq, Hkv, B, S = 3, 5, 2, 129
    table = _table(D)
    q, k = _inputs((B, S), Hq, Hkv, D)
    de = lambda x: torch.cat((x[..., 0::2], x[..., 1::2]), dim=-1).contiguous()
    re = lambda y: torch.stack((y[..., :D // 2], y[..., D // 2:]), dim=-1).reshape(y.shape)
    for inverse in (False, True):
        qi, ki = ops.rope_apply(q, k, table, 5, interleaved=True, inverse=inverse)
        qh, kh = ops.rope_apply(de(q), de(k), table, 5, inverse=inverse)
        assert torch.equal(qi, re(qh)) and torch.equal(ki, re(kh))


@pytest.mark.parametrize("D,Hq,Hkv,interleaved", CASES[:2], ids=CASE_IDS[:2])
def test_autograd_matches_raw(D, Hq, Hkv, interleaved):
    """(h) forward and backward, batched with a start and packed; without k too."""
    table = _table(D)
    q, k = _inputs((2, 129), Hq, Hkv, D)
    dq, dk = _inputs((2, 129), Hq, Hkv, D, salt=1)
    want = ops.rope_apply(q, k, table, 3, interleaved=interleaved)
    want_d = ops.rope_apply(dq, dk, table, 3, interleaved=interleaved, inverse=True)
    ql, kl = q.clone().requires_grad_(), k.clone().requires_grad_()
    qo, ko = ops.rope(ql, kl, table, 3, interleaved=interleaved)
    torch.autograd.backward((qo, ko), (dq, dk))
    for got, w in zip((qo.detach(), ko.detach(), ql.grad, kl.grad), (*want, *want_d)):
        assert torch.equal(got, w)
    # without k; a gradient that does not follow the view rules (the expanded scalar of a sum,
    # stride 0 on D) is made contiguous
    ql = q.clone().requires_grad_()
    qo, none = ops.rope(ql, None, table, 3, interleaved=interleaved)
    assert none is None and torch.equal(qo.detach(), want[0])
    qo.sum().backward()
    assert torch.equal(ql.grad, ops.rope_apply(torch.ones_like(q), None, table, 3, interleaved=interleaved, inverse=True)[0])
    # packed
    T, bounds = 203, PACKINGS["empty middle"]
    q, k = _inputs((T,), Hq, Hkv, D)
    dq, dk = _inputs((T,), Hq, Hkv, D, salt=1)
    cu = _cu(bounds)
    want = ops.rope_apply(q, k, table, cu_seqlens=cu, interleaved=interleaved)
    want_d = ops.rope_apply(dq, dk, table, cu_seqlens=cu, interleaved=interleaved, inverse=True)
    ql, kl = q.clone().requires_grad_(), k.clone().requires_grad_()
    qo, ko = ops.rope(ql, kl, table, cu_seqlens=cu, interleaved=interleaved)
    torch.autograd.backward((qo, ko), (dq, dk))
    for got, w in zip((qo.detach(), ko.detach(), ql.grad, kl.grad), (*want, *want_d)):
        assert torch.equal(got[:200], w[:200])


# --- adjoint ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D,Hq,Hkv,interleaved", CASES, ids=CASE_IDS)
def test_inverse_is_the_adjoint(D, Hq, Hkv, interleaved):
    """With R the rotation the table defines (any c, s: no orthogonality is used), the kernel returns
    ``y = R x + e`` and ``dx = R^T g + f`` with ``|e| <= b(x, R x)`` and ``|f| <= b(g, R^T g)``
    element by element, ``b(u, w) = 2^-8 |w| + 2^-22 (|u1| + |u2|)`` the accuracy bound.  In exact
    arithmetic ``<R x, g> = <x, R^T g>``, so

        <y, g> - <x, dx> = <e, g> - <x, f>,   |<y, g> - <x, dx>| <= sum b(x, R x) |g| + sum b(g, R^T g) |x|.

    Both sums are taken in fp64 over bf16 values (products exact, the summation error of ~1e-16
    relative is far below the bound and not added)."""
    B, S, pos0 = 2, 257, 1000
    table = _table(D)
    (x, _), (g, _) = _inputs((B, S), Hq, Hkv, D), _inputs((B, S), Hq, Hkv, D, salt=1)
    pos = _positions(B, S, pos0)
    y, _ = ops.rope_apply(x, None, table, pos0, interleaved=interleaved)
    dx, _ = ops.rope_apply(g, None, table, pos0, interleaved=interleaved, inverse=True)
    lhs, rhs = (y.double() * g.double()).sum().item(), (x.double() * dx.double()).sum().item()
    b_y = _bound(x, ops.rope_reference(x, table, pos, interleaved), interleaved)
    b_d = _bound(g, ops.rope_reference(g, table, pos, interleaved, inverse=True), interleaved)
    bound = ((b_y * g.double().abs()).sum() + (b_d * x.double().abs()).sum()).item()
    print(f"[rope adjoint D={D}] <y, g> = {lhs:.6f} <x, dx> = {rhs:.6f} difference / bound {abs(lhs - rhs) / bound:.3e}")
    assert abs(lhs - rhs) <= bound


# --- safety ------------------------------------------------------------------------------------------------

def _framed(shape, strides, offset, numel, seed=None):
    """A view inside a sentinel-filled buffer, and a mask of the buffer's elements it covers."""
    buf = torch.full((numel,), SENTINEL, dtype=BF, device="cuda")
    view = buf.as_strided(shape, strides, offset)
    mask = torch.zeros(numel, dtype=torch.bool, device="cuda")
    mask.as_strided(shape, strides, offset).fill_(True)
    if seed is not None:
        view.copy_(_randn(*shape, seed=seed))
    return buf, view, mask


@pytest.mark.parametrize("interleaved", [False, True], ids=["half", "interleaved"])
def test_framed_views_batched(interleaved):
    """q and k are column slices of one fused [B, S, (Hq + 2 Hkv) D + 8] buffer (gaps between the
    heads' runs: the v columns and the padding), outputs are views with strides of their own in
    another buffer; then in place.  Every byte outside the views keeps its value."""
    B, S, Hq, Hkv, D = 2, 129, 4, 2, 80
    row = (Hq + 2 * Hkv) * D + 8
    numel = 16 + B * S * row + 16
    table = _table(D)
    fused = torch.full((numel,), SENTINEL, dtype=BF, device="cuda")
    mask = torch.zeros(numel, dtype=torch.bool, device="cuda")
    view = lambda t, off, H: t.as_strided((B, S, H, D), (S * row, row, D, 1), 16 + off)
    q, k = view(fused, 0, Hq), view(fused, Hq * D, Hkv)
    q.copy_(_randn(B, S, Hq, D, seed=1))
    k.copy_(_randn(B, S, Hkv, D, seed=2))
    view(mask, 0, Hq).fill_(True)
    view(mask, Hq * D, Hkv).fill_(True)
    before = fused.clone()
    want_q, want_k = ops.rope_apply(q.contiguous(), k.contiguous(), table, 7, interleaved=interleaved)
    # outputs: head stride D + 16, token stride with a gap, batch stride with a gap
    so = lambda H: ((S * (H * (D + 16) + 8) + 24), H * (D + 16) + 8, D + 16, 1)
    obq, oq, mq = _framed((B, S, Hq, D), so(Hq), 8, 8 + B * so(Hq)[0] + 8)
    obk, ok, mk = _framed((B, S, Hkv, D), so(Hkv), 24, 24 + B * so(Hkv)[0] + 8)
    ops.rope_apply(q, k, table, 7, interleaved=interleaved, q_out=oq, k_out=ok)
    assert torch.equal(fused, before), "an out-of-place call changed its inputs' buffer"
    assert torch.equal(oq, want_q) and torch.equal(ok, want_k)
    assert (obq[~mq] == SENTINEL).all() and (obk[~mk] == SENTINEL).all(), "bytes outside the output views changed"
    ops.rope_apply(q, k, table, 7, interleaved=interleaved, q_out=q, k_out=k)
    assert torch.equal(q, want_q) and torch.equal(k, want_k)
    assert torch.equal(fused[~mask], before[~mask]), "in place: bytes outside the views changed"


def test_framed_views_packed_truncation_and_a_short_table():
    T, Hq, Hkv, D = 203, 3, 5, 64
    row = (Hq + 2 * Hkv) * D
    numel = 8 + T * row + 8
    fused = torch.full((numel,), SENTINEL, dtype=BF, device="cuda")
    mask = torch.zeros(numel, dtype=torch.bool, device="cuda")
    view = lambda t, off, H, rows=T: t.as_strided((rows, H, D), (row, D, 1), 8 + off)
    q, k = view(fused, 0, Hq), view(fused, Hq * D, Hkv)
    q.copy_(_randn(T, Hq, D, seed=3))
    k.copy_(_randn(T, Hkv, D, seed=4))
    # rows [cu[n], T) = [200, T) are outside the views that may change
    view(mask, 0, Hq, 200).fill_(True)
    view(mask, Hq * D, Hkv, 200).fill_(True)
    before = fused.clone()
    table = _table(D)
    bounds = PACKINGS["empty middle"]
    want_q, want_k = ops.rope_apply(q.contiguous(), k.contiguous(), table, cu_seqlens=_cu(bounds))
    ops.rope_apply(q, k, table, cu_seqlens=_cu(bounds), q_out=q, k_out=k)
    assert torch.equal(q[:200], want_q[:200]) and torch.equal(k[:200], want_k[:200])
    assert torch.equal(fused[~mask], before[~mask]), "bytes outside the sequences' rows changed"

    # cu[n] > T truncates the last sequence at T; negative boundaries clamp to 0
    q, k = _inputs((T,), Hq, Hkv, D)
    exact = ops.rope_apply(q, k, table, cu_seqlens=_cu([0, 3, 3, T]))
    for broken in ([0, 3, 3, T + 40], [-5, 3, 3, 2 ** 31 - 1]):
        got = ops.rope_apply(q, k, table, cu_seqlens=_cu(broken))
        assert torch.equal(got[0], exact[0]) and torch.equal(got[1], exact[1]), f"{broken} is not {[0, 3, 3, T]}"

    # a document longer than the table: the row index is clamped, the frame stays intact and the
    # positions the table does hold are what they always were
    short = _table(D, 8)
    assert torch.equal(short, table[:8])
    obq, oq, mq = _framed((T, Hq, D), (Hq * D + 8, D, 1), 8, 8 + T * (Hq * D + 8) + 8)
    obk, ok, mk = _framed((T, Hkv, D), (Hkv * D + 8, D, 1), 8, 8 + T * (Hkv * D + 8) + 8)
    ops.rope_apply(q, k, short, cu_seqlens=_cu([0, 3, 3, T]), q_out=oq, k_out=ok)
    assert (obq[~mq] == SENTINEL).all() and (obk[~mk] == SENTINEL).all()
    assert torch.isfinite(oq.float()).all() and torch.isfinite(ok.float()).all()
    for rows in (slice(0, 3), slice(3, 11)):
        assert torch.equal(oq[rows], exact[0][rows]) and torch.equal(ok[rows], exact[1][rows])


def test_token_stride_of_2_to_the_30_elements():
    """Three tokens 2^30 elements (2 GiB) apart: the last one's offset needs more than 32 bits.
    Only the rows in use are ever touched; the buffer is never filled."""
    Hq, Hkv, D, step = 4, 2, 64, 1 << 30
    table = _table(D)
    big = torch.empty(2 * step + (Hq + Hkv) * D, dtype=BF, device="cuda")
    q = big.as_strided((3, Hq, D), (step, D, 1))
    k = big.as_strided((3, Hkv, D), (step, D, 1), Hq * D)
    qs, ks = _inputs((3,), Hq, Hkv, D)
    q.copy_(qs)
    k.copy_(ks)
    want_b = ops.rope_apply(qs[None], ks[None], table, 998)
    want_p = ops.rope_apply(qs, ks, table, cu_seqlens=_cu([0, 1, 3]))
    got = ops.rope_apply(q[None], k[None], table, 998)  # strided in, contiguous out
    assert torch.equal(got[0], want_b[0]) and torch.equal(got[1], want_b[1])
    ops.rope_apply(q, k, table, cu_seqlens=_cu([0, 1, 3]), q_out=q, k_out=k)  # in place, packed
    assert torch.equal(q, want_p[0]) and torch.equal(k, want_p[1])
    q.copy_(torch.full_like(qs, SENTINEL))
    ops.rope_apply(qs[None], None, table, 998, q_out=q[None])  # contiguous in, strided out
    assert torch.equal(q[None], want_b[0]) and torch.equal(k, want_p[1])


def test_graph_replay_follows_the_boundaries():
    T, Hq, Hkv, D = 203, 4, 2, 128
    table = _table(D)
    q, k = _inputs((T,), Hq, Hkv, D)
    packings = ([0, 3, 3, 200], [0, 100, 150, 203])  # the same T and n
    eager = [ops.rope_apply(q, k, table, cu_seqlens=_cu(b), q_out=torch.full_like(q, SENTINEL),
                            k_out=torch.full_like(k, SENTINEL)) for b in packings]
    assert not torch.equal(eager[0][0], eager[1][0])
    cu = _cu(packings[0])
    qo, ko = torch.empty_like(q), torch.empty_like(k)
    cs = torch.cuda.Stream()
    cs.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(cs):
        with torch.cuda.graph(g, stream=cs):
            ops.rope_apply(q, k, table, cu_seqlens=cu, q_out=qo, k_out=ko)
    torch.cuda.current_stream().wait_stream(cs)
    for bounds, want in zip(packings, eager):
        cu.copy_(_cu(bounds))
        qo.fill_(SENTINEL)
        ko.fill_(SENTINEL)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(qo, want[0]) and torch.equal(ko, want[1]), f"the replay with boundaries {bounds} differs from the eager call"


def test_refused_calls_leave_the_outputs_untouched():
    B, S, Hq, Hkv, D = 2, 129, 4, 2, 64
    table = _table(D)
    q, k = _inputs((B, S), Hq, Hkv, D)
    qp, kp = _inputs((203,), Hq, Hkv, D)
    cu = _cu([0, 3, 3, 200])
    qo, ko = torch.full_like(q, SENTINEL), torch.full_like(k, SENTINEL)
    qpo, kpo = torch.full_like(qp, SENTINEL), torch.full_like(kp, SENTINEL)
    off = torch.full((k.numel() + 8,), SENTINEL, dtype=BF, device="cuda")
    ko_off = off[4:4 + k.numel()].view(k.shape)  # 8 bytes past a 16-byte boundary
    bat = lambda *a, **kw: ops.rope_apply(*a, **{"q_out": qo, "k_out": ko, **kw})
    pk = lambda *a, **kw: ops.rope_apply(*a, **{"q_out": qpo, "k_out": kpo, **kw})
    refused = [
        (TypeError, lambda: bat(q.float(), k, table)),
        (TypeError, lambda: bat(q, k, table.double())),
        (TypeError, lambda: pk(qp, kp, table, cu_seqlens=cu.long())),
        (ValueError, lambda: bat(q, k, table, P - S + 1)),
        (ValueError, lambda: bat(q, k, table, -1)),
        (ValueError, lambda: bat(q, k, table, cu_seqlens=cu)),
        (ValueError, lambda: pk(qp, kp, table)),
        (ValueError, lambda: pk(qp, kp, table, 1, cu_seqlens=cu)),
        (ValueError, lambda: pk(qp, kp, table, cu_seqlens=cu.cpu())),
        (ValueError, lambda: pk(qp, kp[:-1], table, cu_seqlens=cu)),
        (ValueError, lambda: bat(q, k, table.cpu())),
        (ValueError, lambda: bat(q, k, _table(128))),
        (ValueError, lambda: bat(q, k[:, :, :, :32], table)),
        (ValueError, lambda: bat(q, k, table, q_out=qo[:, :-1])),
        (ValueError, lambda: bat(q, k, table, k_out=ko_off)),
        (ValueError, lambda: bat(q, None, table, k_out=ko)),
    ]
    for error, call in refused:
        with pytest.raises(error, match="rope"):
            call()
    # the extension's own refusals, before any launch
    dev = _native.device()
    view = lambda t: (t.data_ptr(), t.stride(0), t.stride(1), t.stride(2))
    stream = torch.cuda.current_stream().cuda_stream

    def raw(D_=D, B_=B, S_=S, pos0=0, cu_ptr=0, n=0, rows=P, qv=None, tab=None, lanes=0):
        dev.rope_apply(qv or view(q), view(qo), Hq, view(k), view(ko), Hkv, tab or table.data_ptr(), rows, B_, S_, D_, pos0,
                       cu_ptr, n, False, False, lanes, stream)

    for kw in (dict(D_=24), dict(D_=272), dict(pos0=-1), dict(pos0=P - S + 1), dict(rows=0), dict(n=3),
               dict(cu_ptr=cu.data_ptr(), n=3), dict(cu_ptr=cu.data_ptr(), n=0, B_=1), dict(cu_ptr=cu.data_ptr(), n=65537, B_=1),
               dict(cu_ptr=cu.data_ptr(), n=3, B_=1, pos0=1), dict(cu_ptr=cu.data_ptr() + 2, n=3, B_=1),
               dict(qv=(q.data_ptr() + 2, *q.stride()[:3])), dict(qv=(q.data_ptr(), q.stride(0), q.stride(1) + 4, q.stride(2))),
               dict(tab=table.data_ptr() + 4), dict(B_=0), dict(B_=1 << 20, S_=1 << 20), dict(lanes=-1),
               dict(lanes=Hq + Hkv + 1)):
        with pytest.raises(ValueError, match="rope"):
            raw(**kw)
    torch.cuda.synchronize()
    for name, buf in (("q_out", qo), ("k_out", ko), ("packed q_out", qpo), ("packed k_out", kpo), ("misaligned k_out", off)):
        assert (buf == SENTINEL).all(), f"a refused call wrote {name}"


# --- the model ---------------------------------------------------------------------------------------------

TINY = dict(d=256, heads=4, kv_heads=2, ffn=256, vocab=512, layers=2)


def _tp():
    from collective_communication_mpi_amd import MPI, Communicator

    return Communicator(MPI.COMM_WORLD)  # one rank: the TP group of the layers


def _ids(B, S):
    return torch.randint(0, 512, (B, S), device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))


def _compare(tag, a_model, b_model, loss_a, loss_b):
    rel = abs(loss_a - loss_b) / abs(loss_b)
    worst = 1.0
    for (name, a), (_, b) in zip(a_model.named_parameters(), b_model.named_parameters()):
        assert a.grad is not None and b.grad is not None, name
        cos = torch.nn.functional.cosine_similarity(a.grad.double().flatten(), b.grad.double().flatten(), dim=0).item()
        worst = min(worst, cos)
    print(f"[rope model] {tag}: losses {loss_a:.6f} / {loss_b:.6f} relative difference {rel:.3e}; worst gradient cosine {worst:.6f}")
    assert rel <= 2.0 ** -7
    assert worst >= 0.999


def test_model_flash_matches_sdpa_and_rope_changes_the_loss():
    from collective_communication_mpi_amd.parallel.llama_dp import LlamaConfig, LlamaModel

    tp, ids = _tp(), _ids(2, 257)
    models = {kind: LlamaModel(LlamaConfig(**TINY, attention=kind, rope=True), tp, torch.device("cuda"), seed=3)
              for kind in ("sdpa", "flash")}
    for a, b in zip(models["sdpa"].parameters(), models["flash"].parameters()):
        assert torch.equal(a, b)
    assert models["flash"].rope_table.shape == (8192, 2, 32)
    assert all(blk.rope_table is models["flash"].rope_table for blk in models["flash"].blocks)
    losses = {}
    for kind, m in models.items():
        loss = m(ids)
        loss.backward()
        losses[kind] = loss.item()
    _compare("flash against sdpa", models["flash"], models["sdpa"], losses["flash"], losses["sdpa"])
    # the same weights and ids without positions give another loss, on both paths
    for kind in ("sdpa", "flash"):
        plain = LlamaModel(LlamaConfig(**TINY, attention=kind), tp, torch.device("cuda"), seed=3)
        assert plain.rope_table is None
        for a, b in zip(plain.parameters(), models[kind].parameters()):
            assert torch.equal(a, b)
        diff = abs(plain(ids).item() - losses[kind])
        print(f"[rope model] {kind}: |loss(rope) - loss(no rope)| = {diff:.3e}")
        assert diff > 0


def test_model_packed_documents_match_each_document_alone():
    from collective_communication_mpi_amd.parallel.llama_dp import LlamaConfig, LlamaModel

    docs = (67, 190)
    total = sum(docs)
    tp = _tp()
    cfg = LlamaConfig(**TINY, attention="flash", rope=True)
    packed, alone = (LlamaModel(cfg, tp, torch.device("cuda"), seed=3) for _ in range(2))
    ids = _ids(1, total)
    targets = torch.roll(ids, -1, dims=1)
    targets[0, docs[0] - 1] = -100
    targets[0, total - 1] = -100
    cu = _cu([0, docs[0], total])
    loss = packed(ids, targets=targets, cu_seqlens=cu)
    loss.backward()
    # each document alone (its positions start at 0 there), weighted by its number of predicted tokens
    parts = [alone(ids[:, b:e], targets=targets[:, b:e]) for b, e in ((0, docs[0]), (docs[0], total))]
    weights = [n - 1 for n in docs]
    mean = (weights[0] * parts[0] + weights[1] * parts[1]) / sum(weights)
    mean.backward()
    _compare("packed against each document alone", packed, alone, loss.item(), mean.item())


def test_model_positions_reach_the_logits_and_max_positions_is_enforced():
    from collective_communication_mpi_amd.parallel.llama_dp import LlamaConfig, LlamaModel

    tp, S = _tp(), 129
    model = LlamaModel(LlamaConfig(**TINY, attention="flash", rope=True), tp, torch.device("cuda"), seed=3)
    seen = []
    hook = model.head.register_forward_hook(lambda _m, _i, out: seen.append(out.detach().view(1, S, -1)[0, -1].clone()))
    ids = _ids(1, S)
    rolled = torch.cat((torch.roll(ids[:, :-1], 1, dims=1), ids[:, -1:]), dim=1)  # the same last token, its past rolled
    with torch.no_grad():
        model(ids)
        model(rolled)
    hook.remove()
    change = (seen[0].double() - seen[1].double()).abs().max().item()
    print(f"[rope model] last position's logits after rolling the tokens before it: largest change {change:.3e}")
    assert change > 0

    for kind in ("sdpa", "flash"):
        small = LlamaModel(LlamaConfig(**TINY, attention=kind, rope=True, max_positions=128), tp, torch.device("cuda"), seed=3)
        assert small.rope_table.shape[0] == 128
        with torch.no_grad():
            small(_ids(2, 128))  # exactly max_positions fits
        with pytest.raises(ValueError, match="max_positions"):
            small(ids)
