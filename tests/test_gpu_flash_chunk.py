"""The chunk form of flash attention (``ops.flash_attention_chunk_*``) on one GPU: a query chunk
whose row 0 sits at position ``q_pos0`` of a key sequence of its own length, read flat or in
segments (csrc/device/flash_attn.hip).

Numeric checks follow test_gpu_flash_attention.py, whose recipe is used unchanged: the reference is
the fp64 masked softmax composition and its autograd on the same bf16 inputs, here with the
offset mask ``key <= q_pos0 + query``; per tensor the tolerance is 8 x the error of the fp32
composition rounded once to bf16 (measured per case), floor 2^-8 x the largest reference
magnitude; ``lse`` at 2^-20 (1 + |lse|).  The worst error / tolerance ratios are printed; measured
values are in profiles/flash_attention/README.md.  Everything else is bitwise: a chunk against the
full call's rows, segmented against flat keys, a graph replay against eager calls."""
import math

import pytest
import torch

from collective_communication_mpi_amd import _native, ops
from test_gpu_flash_attention import B, FLOOR, NAMES, _framed, _need_gpu  # noqa: F401  (_need_gpu: autouse skip)

pytestmark = pytest.mark.gpu

# (Sq, Sk, q_pos0, causal) x pruned (Hq, Hkv, D)
SHAPES = [
    ((1, 1, 0, True), [(4, 2, 64), (8, 1, 128)]),          # dq and dk are exactly 0
    ((1, 130, 129, True), [(4, 2, 128), (8, 1, 64)]),      # one row that sees everything
    ((63, 191, 128, True), [(4, 2, 64), (8, 1, 128)]),
    ((128, 256, 128, True), [(4, 2, 128), (8, 1, 64)]),    # exact tiles
    ((129, 515, 257, True), [(4, 2, 64), (4, 2, 128), (8, 1, 64), (8, 1, 128)]),  # off every grid, ragged tails
    ((70, 333, 0, True), [(4, 2, 64), (8, 1, 128)]),       # keys 70.. are invisible to all
    ((70, 333, 0, False), [(4, 2, 128), (8, 1, 64)]),
    ((200, 200, 0, True), [(4, 2, 64), (8, 1, 128)]),
    ((200, 200, 0, False), [(4, 2, 128), (8, 1, 64)]),
]
CASES = [(*shape, *heads) for shape, combos in SHAPES for heads in combos]


def _id(c):
    return "q{}-k{}-p{}-{}-H{}x{}-D{}".format(c[0], c[1], c[2], "causal" if c[3] else "full", *c[4:])


def _inputs(Sq, Sk, Hq, Hkv, D, salt=0):
    g = torch.Generator(device="cuda").manual_seed(777 + 131 * Sq + 29 * Sk + 17 * Hq + 3 * Hkv + D + 7919 * salt)
    mk = lambda s, h: torch.randn(B, s, h, D, device="cuda", generator=g).bfloat16()
    return mk(Sq, Hq), mk(Sk, Hkv), mk(Sk, Hkv), mk(Sq, Hq)  # q, k, v, dout


def _compose(q, k, v, dout, causal, q_pos0, dtype):
    """(out, lse, dq, dk, dv) of the softmax composition under the offset mask, in ``dtype``."""
    _, Sq, Hq, D = q.shape
    Sk, rep = k.shape[1], Hq // k.shape[2]
    ql, kl, vl = (t.detach().to(dtype).requires_grad_() for t in (q, k, v))
    ke, ve = kl.repeat_interleave(rep, dim=2), vl.repeat_interleave(rep, dim=2)
    s = torch.einsum("bqhd,bkhd->bhqk", ql, ke) * D ** -0.5
    if causal:
        rows = torch.arange(Sq, device=q.device).view(-1, 1) + q_pos0
        s = s.masked_fill(torch.arange(Sk, device=q.device).view(1, -1) > rows, float("-inf"))
    lse = torch.logsumexp(s, dim=-1)
    out = torch.einsum("bhqk,bkhd->bqhd", torch.softmax(s, dim=-1), ve)
    out.backward(dout.to(dtype))
    return out.detach(), lse.detach(), ql.grad, kl.grad, vl.grad


_REF = {}


def _reference(case):
    """Inputs, the fp64 reference and the per-tensor tolerances of one case, computed once."""
    if case not in _REF:
        Sq, Sk, p0, causal, Hq, Hkv, D = case
        q, k, v, dout = _inputs(Sq, Sk, Hq, Hkv, D)
        ref = _compose(q, k, v, dout, causal, p0, torch.float64)
        f32 = _compose(q, k, v, dout, causal, p0, torch.float32)
        tol = {}
        for name, r, c in zip(NAMES, (ref[0], *ref[2:]), (f32[0], *f32[2:])):
            tol[name] = max(8 * (c.bfloat16().double() - r).abs().max().item(), FLOOR * r.abs().max().item())
        _REF[case] = (q, k, v, dout, ref, tol)
    return _REF[case]


def _run(q, k, v, dout, causal, q_pos0=0, kv_segment=None, **outs):
    out, lse = ops.flash_attention_chunk_forward(q, k, v, causal, q_pos0=q_pos0, kv_segment=kv_segment,
                                                 out=outs.get("out"), lse=outs.get("lse"))
    dq, dk, dv = ops.flash_attention_chunk_backward(dout, q, k, v, out, lse, causal, q_pos0=q_pos0, kv_segment=kv_segment,
                                                    **{n: outs.get(n) for n in ("dq", "dk", "dv", "delta")})
    return out, lse, dq, dk, dv


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_against_fp64(case):
    Sq, Sk, p0, causal, Hq, Hkv, D = case
    q, k, v, dout, ref, tol = _reference(case)
    out, lse, dq, dk, dv = _run(q, k, v, dout, causal, p0)
    ratios = {}
    for name, g, r in zip(NAMES, (out, dq, dk, dv), (ref[0], *ref[2:])):
        assert g.dtype == torch.bfloat16 and g.shape == r.shape and g.is_contiguous()
        err = (g.double() - r).abs().max().item()
        ratios[name] = err / tol[name] if tol[name] > 0 else (0.0 if err == 0 else math.inf)
    lse_err = ((lse.double() - ref[1]).abs() / (1 + ref[1].abs())).max().item() * 2.0 ** 20
    print(f"[flash chunk fp64] {_id(case)}: error / tolerance " + " ".join(f"{n}={x:.3f}" for n, x in ratios.items())
          + f" lse={lse_err:.3f}")
    assert lse.dtype == torch.float32 and lse.shape == (B, Hq, Sq)
    assert lse_err <= 1.0, f"lse error {lse_err:.3f} x 2^-20 (1 + |lse|)"
    for name, x in ratios.items():
        assert x <= 1.0, f"{name}: error is {x:.3f} x the tolerance {tol[name]:.3e}"
    if Sk == 1:  # the row's single key: P = 1, dP = delta
        assert (dq == 0).all() and (dk == 0).all()
    if causal and p0 + Sq < Sk:  # keys no query of the chunk sees
        assert (ref[3][:, p0 + Sq:] == 0).all() and (ref[4][:, p0 + Sq:] == 0).all()
        assert (dk[:, p0 + Sq:] == 0).all() and (dv[:, p0 + Sq:] == 0).all(), "an invisible key's dk / dv is not exactly zero"
        assert (dv[:, :p0 + Sq] != 0).any(dim=-1).all()


@pytest.mark.parametrize("case", [c for c in CASES if c[:3] == (200, 200, 0)], ids=_id)
def test_equals_self_attention_bitwise(case):
    q, k, v, dout, _, _ = _reference(case)
    causal = case[3]
    out, lse = ops.flash_attention_forward(q, k, v, causal)
    want = (out, lse, *ops.flash_attention_backward(dout, q, k, v, out, lse, causal))
    for name, g, w in zip(("out", "lse", "dq", "dk", "dv"), _run(q, k, v, dout, causal), want):
        assert torch.equal(g, w), f"{name} differs from the self-attention entry point"


@pytest.mark.parametrize("Hq,Hkv,D", [(4, 2, 64), (8, 1, 128)])
def test_chunk_equals_full_rows_bitwise(Hq, Hkv, D):
    """A row's sums run over the same key steps in the same order whichever chunk holds it, and a
    wholly masked step is an exact no-op, so out, lse and dq are the full call's rows.  (dk and
    dv regroup query rows and are not.)"""
    S = 515
    q, k, v, dout = _inputs(S, S, Hq, Hkv, D, salt=2)
    out, lse = ops.flash_attention_forward(q, k, v, True)
    dq, _, _ = ops.flash_attention_backward(dout, q, k, v, out, lse, True)
    for a, b in ((0, 131), (131, 388), (388, 515)):
        o, l = ops.flash_attention_chunk_forward(q[:, a:b], k, v, True, q_pos0=a)
        assert torch.equal(o, out[:, a:b]), f"out of chunk [{a}, {b})"
        assert torch.equal(l, lse[:, :, a:b]), f"lse of chunk [{a}, {b})"
        # the full call's rows of out and lse (contiguous copies) and the same dout rows
        g, _, _ = ops.flash_attention_chunk_backward(dout[:, a:b], q[:, a:b], k, v, out[:, a:b].contiguous(),
                                                     lse[:, :, a:b].contiguous(), True, q_pos0=a)
        assert torch.equal(g, dq[:, a:b]), f"dq of chunk [{a}, {b})"


def _segmented(t, n, L, fill, pad=24, guard=64):
    """``t`` [B, n L, H, D] as a [n, B, L, H, D] view, segments ``pad`` elements further apart than
    they are long, inside a buffer filled with ``fill``; returns (buffer, view, mask of the view)."""
    _, _, H, D = t.shape
    seg = B * L * H * D + pad
    buf = torch.full((2 * guard + n * seg,), fill, dtype=t.dtype, device=t.device)
    view = buf[guard:].as_strided((n, B, L, H, D), (seg, L * H * D, H * D, D, 1))
    mask = torch.zeros_like(buf, dtype=torch.bool)
    mask[guard:].as_strided(view.shape, view.stride()).fill_(True)
    if t is not None:
        view.copy_(t.view(B, n, L, H, D).transpose(0, 1))
    return buf, view, mask


# (n, L, Sq, q_pos0, causal, Hq, Hkv, D)
SEGMENTED = [(5, 50, 129, 100, True, 4, 2, 64), (5, 50, 70, 0, False, 8, 1, 128), (70, 1, 37, 33, True, 8, 1, 64),
             (2, 128, 128, 128, True, 4, 2, 128), (2, 128, 128, 0, True, 8, 1, 64)]


@pytest.mark.parametrize("n,L,Sq,p0,causal,Hq,Hkv,D", SEGMENTED,
                         ids=["n{}-L{}-q{}-p{}-{}-H{}x{}-D{}".format(*c[:4], "causal" if c[4] else "full", *c[5:])
                              for c in SEGMENTED])
def test_segmented_equals_flat_bitwise(n, L, Sq, p0, causal, Hq, Hkv, D):
    Sk = n * L
    q, k, v, dout = _inputs(Sq, Sk, Hq, Hkv, D, salt=4)
    want = _run(q, k, v, dout, causal, p0)
    nan = float("nan")
    _, ks, _ = _segmented(k, n, L, nan)
    _, vs, _ = _segmented(v, n, L, nan, pad=8)
    dkbuf, dks, dkmask = _segmented(torch.zeros_like(k), n, L, -7.0, pad=8)
    dvbuf, dvs, dvmask = _segmented(torch.zeros_like(v), n, L, -7.0)
    dks.fill_(-7.0)
    dvs.fill_(-7.0)
    assert not ks.is_contiguous() and ks.stride(0) % 8 == 0 and ks.stride(0) != dks.stride(0)
    got = _run(q, ks, vs, dout, causal, p0, kv_segment=L, dk=dks, dv=dvs)
    assert got[3].data_ptr() == dks.data_ptr() and got[4].data_ptr() == dvs.data_ptr()
    flat = lambda t: t.transpose(0, 1).reshape(B, Sk, Hkv, D)
    for name, g, w in zip(("out", "lse", "dq"), got[:3], want[:3]):
        assert torch.equal(g, w), f"{name} of the segmented keys differs from the flat call"
    assert torch.equal(flat(dks), want[3]) and torch.equal(flat(dvs), want[4])
    for name, buf, mask in (("dk", dkbuf, dkmask), ("dv", dvbuf, dvmask)):
        assert (buf[~mask] == -7.0).all(), f"the padding or the frame of {name} was overwritten"
        assert not torch.isnan(buf).any()


def _padded(t, fill, pad=8, guard=64):
    """``t`` [B, S, H, D] as an unsegmented view whose rows are ``pad`` elements further apart than
    they are long, inside a buffer filled with ``fill``; returns (buffer, view, mask of the view)."""
    _, S, H, D = t.shape
    row = H * D + pad
    buf = torch.full((2 * guard + B * S * row,), fill, dtype=t.dtype, device=t.device)
    view = buf[guard:].as_strided((B, S, H, D), (S * row, row, D, 1))
    mask = torch.zeros_like(buf, dtype=torch.bool)
    mask[guard:].as_strided(view.shape, view.stride()).fill_(True)
    view.copy_(t)
    return buf, view, mask


@pytest.mark.parametrize("Hq,Hkv,D", [(4, 2, 64), (8, 1, 128)])
@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
def test_strided_dk_dv_at_the_self_shape(causal, Hq, Hkv, D):
    """Sq = Sk and q_pos0 = 0 through the chunk call stay a chunk call: dk / dv go through their
    strides.  70 keys are two key blocks, the second ragged."""
    S = 70
    q, k, v, dout = _inputs(S, S, Hq, Hkv, D, salt=6)
    out, lse = ops.flash_attention_forward(q, k, v, causal)
    want = (out, lse, *ops.flash_attention_backward(dout, q, k, v, out, lse, causal))
    nan = float("nan")
    _, ks, _ = _padded(k, nan)
    _, vs, _ = _padded(v, nan, pad=16)
    dkbuf, dks, dkmask = _padded(torch.full_like(k, -7.0), -7.0, pad=16)
    dvbuf, dvs, dvmask = _padded(torch.full_like(v, -7.0), -7.0)
    assert not ks.is_contiguous() and not dks.is_contiguous() and ks.stride(1) != dks.stride(1)
    got = _run(q, ks, vs, dout, causal, 0, dk=dks, dv=dvs)
    assert got[3].data_ptr() == dks.data_ptr() and got[4].data_ptr() == dvs.data_ptr()
    for name, g, w in zip(("out", "lse", "dq", "dk", "dv"), got, want):
        assert torch.equal(g, w), f"{name} differs from self-attention on contiguous copies"
    for name, buf, mask in (("dk", dkbuf, dkmask), ("dv", dvbuf, dvmask)):
        assert (buf[~mask] == -7.0).all(), f"the padding or the frame of {name} was overwritten"
        assert not torch.isnan(buf).any()


def test_self_attention_flag_is_guarded():
    """The extension refuses, before any launch, a self_attention call whose arguments are not
    those of self-attention: the kSelf kernels read neither Sk nor q_pos0 nor the dk / dv strides."""
    S, D = 16, 64
    dev = _native.device()
    stream = torch.cuda.current_stream().cuda_stream
    q, k, v, dout = (torch.zeros(1, S, 1, D, dtype=torch.bfloat16, device="cuda") for _ in range(4))
    fr = {"out": _framed((1, S, 1, D), torch.bfloat16, -7.0), "lse": _framed((1, 1, S), torch.float32, -7.0),
          "dq": _framed((1, S, 1, D), torch.bfloat16, -7.0), "delta": _framed((1, 1, S), torch.float32, -7.0),
          "dk": _framed((1, S, 1, D + 8), torch.bfloat16, -7.0), "dv": _framed((1, S, 1, D), torch.bfloat16, -7.0)}
    o = {name: view for name, (_, view) in fr.items()}
    view = lambda t, row=D: (t.data_ptr(), 0, 0, row, 0)  # B = Hkv = 1: stride 0 on their axes
    ptr = lambda name: o[name].data_ptr()

    def fwd(Sq=S, Sk=S, seg_len=S, q_pos0=0):
        dev.flash_attn_fwd(view(q), view(k), view(v), ptr("out"), ptr("lse"), 1, Sq, Sk, seg_len, q_pos0, 1, 1, D, True,
                           D ** -0.5, True, stream)

    def bwd(Sq=S, Sk=S, seg_len=S, q_pos0=0, dk_row=D):
        dev.flash_attn_bwd(view(dout), view(q), view(k), view(v), ptr("out"), ptr("lse"), ptr("delta"), ptr("dq"),
                           view(o["dk"], dk_row), view(o["dv"]), 1, Sq, Sk, seg_len, q_pos0, 1, 1, D, True, D ** -0.5, True,
                           stream)

    for call in (fwd, bwd):
        for bad in (dict(Sq=8), dict(Sk=8, seg_len=8), dict(q_pos0=8), dict(seg_len=8)):
            with pytest.raises(ValueError, match="self-attention"):
                call(**bad)
    with pytest.raises(ValueError, match="contiguous dk / dv"):
        bwd(dk_row=D + 8)
    torch.cuda.synchronize()
    for name, (buf, _) in fr.items():
        assert (buf == -7.0).all(), f"a refused call wrote {name}"


def test_graph_replay_equals_eager():
    Sq, Sk, p0, Hq, Hkv, D, n, L = 129, 250, 100, 4, 2, 64, 5, 50
    news = [_inputs(Sq, Sk, Hq, Hkv, D, salt=s) for s in (12, 13)]
    want = [_run(*t, True, p0) for t in news]
    q, k, v, dout = (torch.zeros_like(t) for t in news[0])
    _, ks, _ = _segmented(k, n, L, 0.0)
    _, vs, _ = _segmented(v, n, L, 0.0)
    out, lse, dq, delta = torch.empty_like(want[0][0]), torch.empty_like(want[0][1]), torch.empty_like(q), \
        torch.empty_like(want[0][1])
    _, dks, _ = _segmented(torch.zeros_like(k), n, L, 0.0)
    _, dvs, _ = _segmented(torch.zeros_like(v), n, L, 0.0)
    cs = torch.cuda.Stream()
    cs.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(cs):
        with torch.cuda.graph(g, stream=cs):
            _run(q, ks, vs, dout, True, p0, kv_segment=L, out=out, lse=lse, dq=dq, dk=dks, dv=dvs, delta=delta)
    torch.cuda.current_stream().wait_stream(cs)
    flat = lambda t: t.transpose(0, 1).reshape(B, Sk, Hkv, D)
    for (nq, nk, nv, ndo), w in zip(news, want):
        q.copy_(nq)
        dout.copy_(ndo)
        ks.copy_(nk.view(B, n, L, Hkv, D).transpose(0, 1))
        vs.copy_(nv.view(B, n, L, Hkv, D).transpose(0, 1))
        g.replay()
        torch.cuda.synchronize()
        for a, b in zip((out, lse, dq, flat(dks), flat(dvs)), w):
            assert torch.equal(a, b)


def test_refused_calls_leave_the_outputs_untouched():
    Sq, Sk, Hq, Hkv, D, n, L = 70, 100, 4, 2, 64, 2, 50
    q, k, v, dout = _inputs(Sq, Sk, Hq, Hkv, D, salt=9)
    _, ks, _ = _segmented(k, n, L, 0.0)
    _, vs, _ = _segmented(v, n, L, 0.0)
    _, bad_stride, _ = _segmented(k, n, L, 0.0, pad=4)
    fr = {"out": _framed((B, Sq, Hq, D), torch.bfloat16, -7.0), "lse": _framed((B, Hq, Sq), torch.float32, -7.0),
          "dq": _framed((B, Sq, Hq, D), torch.bfloat16, -7.0), "dk": _framed((n, B, L, Hkv, D), torch.bfloat16, -7.0),
          "dv": _framed((n, B, L, Hkv, D), torch.bfloat16, -7.0), "delta": _framed((B, Hq, Sq), torch.float32, -7.0)}
    o = {name: view for name, (_, view) in fr.items()}
    fwd = dict(out=o["out"], lse=o["lse"])
    bwd = dict(dq=o["dq"], dk=o["dk"], dv=o["dv"], delta=o["delta"])
    good_out, good_lse = ops.flash_attention_chunk_forward(q, ks, vs, True, q_pos0=30, kv_segment=L)
    refused = [
        (ValueError, lambda: ops.flash_attention_chunk_forward(q, ks, vs, True, q_pos0=-1, kv_segment=L, **fwd)),
        (ValueError, lambda: ops.flash_attention_chunk_forward(q, ks, vs, True, q_pos0=(1 << 30) - Sq + 1, kv_segment=L, **fwd)),
        (ValueError, lambda: ops.flash_attention_chunk_forward(q, ks, vs[:1], True, q_pos0=30, kv_segment=L, **fwd)),
        (ValueError, lambda: ops.flash_attention_chunk_forward(q, bad_stride, vs, True, q_pos0=30, kv_segment=L, **fwd)),
        (TypeError, lambda: ops.flash_attention_chunk_forward(q, ks.float(), vs, True, q_pos0=30, kv_segment=L, **fwd)),
        (ValueError, lambda: ops.flash_attention_chunk_forward(q, k, v, True, q_pos0=30, out=o["out"][:, :-1], lse=o["lse"])),
        (ValueError, lambda: ops.flash_attention_chunk_backward(dout, q, ks, vs, good_out, good_lse, True, q_pos0=-1,
                                                                kv_segment=L, **bwd)),
        (ValueError, lambda: ops.flash_attention_chunk_backward(dout, q, ks, vs, good_out, good_lse, True, q_pos0=30,
                                                                kv_segment=L, **{**bwd, "dk": o["dk"][:1]})),
        (ValueError, lambda: ops.flash_attention_chunk_backward(dout, q, ks, vs, good_out, good_lse, True, q_pos0=30,
                                                                kv_segment=L, **{**bwd, "dv": torch.empty_like(k)})),
        (TypeError, lambda: ops.flash_attention_chunk_backward(dout, q, ks, vs, good_out, good_lse, True, q_pos0=30,
                                                               kv_segment=L, **{**bwd, "dk": o["dk"].float()})),
        (ValueError, lambda: ops.flash_attention_chunk_backward(dout[:, :-1], q, ks, vs, good_out, good_lse, True,
                                                                q_pos0=30, kv_segment=L, **bwd)),
        (ValueError, lambda: ops.flash_attention_forward(q, k, v, True, **fwd)),  # self-attention: another key length
    ]
    for error, call in refused:
        with pytest.raises(error, match="flash_attention"):
            call()
    torch.cuda.synchronize()
    for name, (buf, _) in fr.items():
        assert (buf == -7.0).all(), f"a refused call wrote {name}"
    # and the accepted call fills them
    _run(q, ks, vs, dout, True, 30, kv_segment=L, **fwd, **bwd)
    for name, (buf, view) in fr.items():
        assert (buf[:64] == -7.0).all() and (buf[-64:] == -7.0).all() and not (view == -7.0).all(), name
