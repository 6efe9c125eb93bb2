"""The packed form of flash attention (``ops.flash_attention_varlen``, the kVarlen kernels of
csrc/device/flash_attn.hip) on one GPU.

The central check is BITWISE: every sequence's rows of ``out``, ``lse``, ``dq``, ``dk`` and ``dv``
equal what ``ops.flash_attention_forward`` / ``_backward`` return for that sequence alone, its rows
taken as a B = 1 view.  The packing is (1, 63, 128, 0, 129, 257, 64), T = 642: one row, a tile less
one, exact tiles, tiles plus one for both block sizes, an empty sequence, and starts off every
tile grid; heads (4, 2, 64) and (8, 1, 128), causal and full.  The fp64 check is the per-sequence
composition under the tolerance recipe of test_gpu_flash_attention.py, unchanged.  Measured
ratios are in profiles/flash_attention/README.md ("Packed sequences")."""
import math

import pytest
import torch

from collective_communication_mpi_amd import _native, ops
from test_gpu_flash_attention import FLOOR, NAMES, _compose, _framed, _need_gpu  # noqa: F401  (_need_gpu: autouse skip)

pytestmark = pytest.mark.gpu

LENGTHS = (1, 63, 128, 0, 129, 257, 64)
T = sum(LENGTHS)
HEADS = [(4, 2, 64), (8, 1, 128)]
OUTPUTS = ("out", "lse", "dq", "dk", "dv")


def _bounds(lengths):
    cu = [0]
    for n in lengths:
        cu.append(cu[-1] + n)
    return cu


def _cu(bounds):
    return torch.tensor(bounds, dtype=torch.int32, device="cuda")


def _inputs(tokens, Hq, Hkv, D, salt=0):
    g = torch.Generator(device="cuda").manual_seed(977 + 131 * tokens + 17 * Hq + 3 * Hkv + D + 7919 * salt)
    mk = lambda h: torch.randn(tokens, h, D, device="cuda", generator=g).bfloat16()
    return mk(Hq), mk(Hkv), mk(Hkv), mk(Hq)  # q, k, v, dout


def _run(q, k, v, dout, cu, causal):
    out, lse = ops.flash_attention_varlen_forward(q, k, v, cu, causal)
    dq, dk, dv = ops.flash_attention_varlen_backward(dout, q, k, v, cu, out, lse, causal)
    return out, lse, dq, dk, dv


def _alone(q, k, v, dout, b, e, causal):
    """The self-attention call on rows [b, e) as a B = 1 view, in the packed layouts."""
    qs, ks, vs, ds = (t[b:e].unsqueeze(0) for t in (q, k, v, dout))
    out, lse = ops.flash_attention_forward(qs, ks, vs, causal)
    dq, dk, dv = ops.flash_attention_backward(ds, qs, ks, vs, out, lse, causal)
    return out[0], lse[0], dq[0], dk[0], dv[0]


def _rows(name, t, b, e):
    return t[:, b:e] if name == "lse" else t[b:e]


_BASE = {}


def _base(heads, causal):
    """Inputs and the packed call's five results of one case, computed once and never changed."""
    key = (heads, causal)
    if key not in _BASE:
        ins = _inputs(T, *heads)
        _BASE[key] = (ins, _run(*ins, _cu(_bounds(LENGTHS)), causal))
    return _BASE[key]


def _assert_sequences_bitwise(ins, got, bounds, causal, label):
    for i, (b, e) in enumerate(zip(bounds[:-1], bounds[1:])):
        if e == b:
            continue
        for name, g, w in zip(OUTPUTS, got, _alone(*ins, b, e, causal)):
            assert torch.equal(_rows(name, g, b, e), w), f"{label}: {name} of sequence {i} (rows {b}..{e}) differs"


CASES = [(h, c) for h in HEADS for c in (True, False)]
CASE_IDS = ["H{}x{}-D{}-{}".format(*h, "causal" if c else "full") for h, c in CASES]


def test_constants():
    assert T == 642 and 0 in LENGTHS
    dev = _native.device()
    assert {1, dev.FLASH_BK - 1, dev.FLASH_BK, dev.FLASH_BQ, dev.FLASH_BQ + 1, 2 * dev.FLASH_BQ + 1} <= set(LENGTHS)


@pytest.mark.parametrize("heads,causal", CASES, ids=CASE_IDS)
def test_bitwise_against_each_sequence_alone(heads, causal):
    ins, got = _base(heads, causal)
    Hq, Hkv, D = heads
    assert [tuple(t.shape) for t in got] == [(T, Hq, D), (Hq, T), (T, Hq, D), (T, Hkv, D), (T, Hkv, D)]
    assert all(t.is_contiguous() for t in got) and got[1].dtype == torch.float32
    _assert_sequences_bitwise(ins, got, _bounds(LENGTHS), causal, "packed")


@pytest.mark.parametrize("heads,causal", CASES, ids=CASE_IDS)
def test_bitwise_one_sequence(heads, causal):
    ins = _inputs(200, *heads, salt=1)
    got = _run(*ins, _cu([0, 200]), causal)
    _assert_sequences_bitwise(ins, got, [0, 200], causal, "n = 1")


@pytest.mark.parametrize("heads,causal", [(HEADS[0], True), (HEADS[1], False)], ids=[CASE_IDS[0], CASE_IDS[3]])
def test_against_fp64(heads, causal):
    ins, (out, lse, dq, dk, dv) = _base(heads, causal)
    bounds = _bounds(LENGTHS)
    parts = {torch.float64: [], torch.float32: []}
    for b, e in zip(bounds[:-1], bounds[1:]):
        if e > b:
            for dtype, acc in parts.items():
                acc.append(_compose(*(t[b:e].unsqueeze(0) for t in ins), causal, dtype))
    # (out, lse, dq, dk, dv) of the per-sequence composition, put back on the token axis
    whole = {dtype: [torch.cat([p[j][0] for p in acc], dim=1 if j == 1 else 0) for j in range(5)]
             for dtype, acc in parts.items()}
    ref, f32 = whole[torch.float64], whole[torch.float32]
    ratios = {}
    for name, g, r, c in zip(NAMES, (out, dq, dk, dv), (ref[0], *ref[2:]), (f32[0], *f32[2:])):
        tol = max(8 * (c.bfloat16().double() - r).abs().max().item(), FLOOR * r.abs().max().item())
        assert g.shape == r.shape
        ratios[name] = (g.double() - r).abs().max().item() / tol
    lse_err = ((lse.double() - ref[1]).abs() / (1 + ref[1].abs())).max().item() * 2.0 ** 20
    print(f"[flash varlen fp64] Hq={heads[0]} Hkv={heads[1]} D={heads[2]} causal={causal}: error / tolerance "
          + " ".join(f"{n}={x:.3f}" for n, x in ratios.items()) + f" lse={lse_err:.3f}")
    assert lse_err <= 1.0, f"lse error {lse_err:.3f} x 2^-20 (1 + |lse|)"
    for name, x in ratios.items():
        assert x <= 1.0, f"{name}: error is {x:.3f} x the tolerance"


@pytest.mark.parametrize("heads,causal", [(HEADS[0], True), (HEADS[1], False)], ids=[CASE_IDS[0], CASE_IDS[3]])
def test_views_frames_and_the_rows_past_the_last_boundary(heads, causal):
    """Operands are column slices of a NaN-filled fused buffer whose last five rows stay NaN
    (cu[n] = T - 5); outputs are views inside sentinel-filled buffers."""
    Hq, Hkv, D = heads
    (q, k, v, dout), _ = _base(heads, causal)
    live = T - 5
    bounds = _bounds(LENGTHS)[:-1] + [live]
    want = _run(q, k, v, dout, _cu(bounds), causal)
    pad = 8
    fused = torch.full((T, (Hq + 2 * Hkv) * D + 2 * pad), float("nan"), device="cuda", dtype=torch.bfloat16)
    cols = [pad, pad + Hq * D, pad + (Hq + Hkv) * D, pad + (Hq + 2 * Hkv) * D]
    views = []
    for t, lo, hi, h in zip((q, k, v), cols[:-1], cols[1:], (Hq, Hkv, Hkv)):
        fused[:live, lo:hi] = t[:live].reshape(live, h * D)
        views.append(fused[:, lo:hi].view(T, h, D))
    dfull = torch.full((T, Hq * D + 2 * pad), float("nan"), device="cuda", dtype=torch.bfloat16)
    dfull[:live, pad:pad + Hq * D] = dout[:live].reshape(live, Hq * D)
    dview = dfull[:, pad:pad + Hq * D].view(T, Hq, D)
    assert not any(t.is_contiguous() for t in (*views, dview))
    assert all(torch.isnan(t[live:]).all() for t in (*views, dview))
    frames = {"out": _framed((T, Hq, D), torch.bfloat16, -7.0), "lse": _framed((Hq, T), torch.float32, -7.0),
              "dq": _framed((T, Hq, D), torch.bfloat16, -7.0), "dk": _framed((T, Hkv, D), torch.bfloat16, -7.0),
              "dv": _framed((T, Hkv, D), torch.bfloat16, -7.0), "delta": _framed((Hq, T), torch.float32, -7.0)}
    cu = _cu(bounds)
    out, lse = ops.flash_attention_varlen_forward(*views, cu, causal, out=frames["out"][1], lse=frames["lse"][1])
    dq, dk, dv = ops.flash_attention_varlen_backward(dview, *views, cu, out, lse, causal, dq=frames["dq"][1],
                                                     dk=frames["dk"][1], dv=frames["dv"][1], delta=frames["delta"][1])
    for name, g, w in zip(OUTPUTS, (out, lse, dq, dk, dv), want):
        assert g.data_ptr() == frames[name][1].data_ptr()
        assert torch.equal(_rows(name, g, 0, live), _rows(name, w, 0, live)), f"{name} of the views differs"
        assert not torch.isnan(_rows(name, g, 0, live)).any()
        assert (_rows(name, g, live, T) == -7.0).all(), f"{name}: a row past cu[n] was written"
    for name, (buf, _) in frames.items():
        assert (buf[:64] == -7.0).all() and (buf[-64:] == -7.0).all(), f"a sentinel around {name} was overwritten"


@pytest.mark.parametrize("heads,causal", [(HEADS[0], False), (HEADS[1], True)], ids=[CASE_IDS[1], CASE_IDS[2]])
def test_no_key_of_another_sequence_is_visible(heads, causal):
    (q, k, v, dout), base = _base(heads, causal)
    bounds, mid = _bounds(LENGTHS), 4
    b, e = bounds[mid], bounds[mid + 1]
    assert e - b == 129
    kn, vn = k.clone(), v.clone()
    kn[b:e] = float("nan")
    vn[b:e] = float("nan")
    got = _run(q, kn, vn, dout, _cu(bounds), causal)
    for name, g, w in zip(OUTPUTS, got, base):
        for lo, hi in ((0, b), (e, T)):
            assert torch.equal(_rows(name, g, lo, hi), _rows(name, w, lo, hi)), f"{name} rows {lo}..{hi} changed"
            assert torch.isfinite(_rows(name, g, lo, hi)).all()


@pytest.mark.parametrize("heads,causal", [(HEADS[0], True), (HEADS[1], False)], ids=[CASE_IDS[0], CASE_IDS[3]])
def test_last_boundary_past_the_end_is_truncated(heads, causal):
    ins, base = _base(heads, causal)
    bounds = _bounds(LENGTHS)[:-1] + [T + 40]
    for name, g, w in zip(OUTPUTS, _run(*ins, _cu(bounds), causal), base):
        assert torch.equal(g, w), f"{name}: cu[n] = T + 40 is not the last sequence truncated at T"


@pytest.mark.parametrize("heads,causal", [(HEADS[0], True), (HEADS[1], False)], ids=[CASE_IDS[0], CASE_IDS[3]])
def test_autograd_matches_raw(heads, causal):
    (q, k, v, dout), want = _base(heads, causal)
    ql, kl, vl = (t.clone().requires_grad_() for t in (q, k, v))
    out = ops.flash_attention_varlen(ql, kl, vl, _cu(_bounds(LENGTHS)), causal=causal)
    out.backward(dout)
    for g, w in zip((out.detach(), ql.grad, kl.grad, vl.grad), (want[0], *want[2:])):
        assert torch.equal(g, w)


def test_graph_replay_follows_the_boundaries():
    heads, causal = HEADS[0], True
    (q, k, v, dout), first = _base(heads, causal)
    other = (200, 0, 1, 64, 65, 184, 128)  # another packing of the same T and n
    assert sum(other) == T and len(other) == len(LENGTHS)
    second = _run(q, k, v, dout, _cu(_bounds(other)), causal)
    assert not torch.equal(first[0], second[0])
    cu = _cu(_bounds(LENGTHS))
    out, lse = torch.empty_like(first[0]), torch.empty_like(first[1])
    dq, dk, dv, delta = (torch.empty_like(t) for t in (first[2], first[3], first[4], first[1]))
    cs = torch.cuda.Stream()
    cs.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(cs):
        with torch.cuda.graph(g, stream=cs):
            ops.flash_attention_varlen_forward(q, k, v, cu, causal, out=out, lse=lse)
            ops.flash_attention_varlen_backward(dout, q, k, v, cu, out, lse, causal, dq=dq, dk=dk, dv=dv, delta=delta)
    torch.cuda.current_stream().wait_stream(cs)
    for lengths, want in ((LENGTHS, first), (other, second)):
        cu.copy_(_cu(_bounds(lengths)))
        for t in (out, lse, dq, dk, dv):
            t.fill_(-7.0)
        g.replay()
        torch.cuda.synchronize()
        for name, a, b in zip(OUTPUTS, (out, lse, dq, dk, dv), want):
            assert torch.equal(a, b), f"{name} of the replay with lengths {lengths} differs from the eager call"


def test_refused_calls_leave_the_outputs_untouched():
    Hq, Hkv, D = HEADS[0]
    q, k, v, dout = _inputs(T, Hq, Hkv, D, salt=2)
    cu = _cu(_bounds(LENGTHS))
    shapes = {"out": ((T, Hq, D), torch.bfloat16), "lse": ((Hq, T), torch.float32), "dq": ((T, Hq, D), torch.bfloat16),
              "dk": ((T, Hkv, D), torch.bfloat16), "dv": ((T, Hkv, D), torch.bfloat16), "delta": ((Hq, T), torch.float32)}
    bufs = {name: torch.full(shape, -7.0, dtype=dtype, device="cuda") for name, (shape, dtype) in shapes.items()}
    fwd = lambda *a, **kw: ops.flash_attention_varlen_forward(*a, out=bufs["out"], lse=bufs["lse"], **kw)
    bwd = lambda *a, **kw: ops.flash_attention_varlen_backward(
        *a, **{"dq": bufs["dq"], "dk": bufs["dk"], "dv": bufs["dv"], "delta": bufs["delta"], **kw})
    good_out, good_lse = torch.zeros_like(bufs["out"]), torch.zeros_like(bufs["lse"])
    refused = [
        (TypeError, lambda: fwd(q, k, v, cu.long())),
        (TypeError, lambda: fwd(q, k, v, None)),
        (TypeError, lambda: fwd(q.float(), k, v, cu)),
        (ValueError, lambda: fwd(q, k, v, cu.cpu())),
        (ValueError, lambda: fwd(q, k, v, cu[:1])),
        (ValueError, lambda: fwd(q, k, v, torch.cat([cu, cu])[::2])),
        (ValueError, lambda: fwd(q, k[:-1], v[:-1], cu)),
        (ValueError, lambda: fwd(q.unsqueeze(0), k.unsqueeze(0), v.unsqueeze(0), cu)),
        (ValueError, lambda: fwd(q[:, :, :32], k[:, :, :32], v[:, :, :32], cu)),
        (ValueError, lambda: fwd(q, k, v, cu, scale=float("nan"))),
        (ValueError, lambda: ops.flash_attention_varlen_forward(q, k, v, cu, out=bufs["out"].unsqueeze(0), lse=bufs["lse"])),
        (ValueError, lambda: bwd(dout[:-1], q, k, v, cu, good_out, good_lse)),
        (TypeError, lambda: bwd(dout.float(), q, k, v, cu, good_out, good_lse)),
        (ValueError, lambda: bwd(dout, q, k, v, cu, good_out, good_lse.t())),
        (ValueError, lambda: bwd(dout, q, k, v, cu, good_out, good_lse, dk=bufs["dk"].unsqueeze(0))),
        (TypeError, lambda: bwd(dout, q, k, v, cu.long(), good_out, good_lse)),
    ]
    for error, call in refused:
        with pytest.raises(error, match="flash_attention"):
            call()
    # the extension's own refusals, before any launch: sequences out of range, a batch, the self flag
    dev = _native.device()
    view = lambda t: (t.data_ptr(), 0, 0, t.stride(0), t.stride(1))
    ptr = lambda name: bufs[name].data_ptr()
    tail = (Hq, Hkv, D, True, D ** -0.5)
    for B, self_flag, n in ((1, False, 0), (1, False, 65537), (2, False, 7), (1, True, 7)):
        with pytest.raises(ValueError, match="flash_attention"):
            dev.flash_attn_fwd(view(q), view(k), view(v), ptr("out"), ptr("lse"), B, T, T, T, 0, *tail, self_flag, 0,
                               cu.data_ptr(), n)
        with pytest.raises(ValueError, match="flash_attention"):
            dev.flash_attn_bwd(view(dout), view(q), view(k), view(v), good_out.data_ptr(), good_lse.data_ptr(), ptr("delta"),
                               ptr("dq"), view(bufs["dk"]), view(bufs["dv"]), B, T, T, T, 0, *tail, self_flag, 0,
                               cu.data_ptr(), n)
    with pytest.raises(ValueError, match="flash_attention"):  # sequences without boundaries
        dev.flash_attn_fwd(view(q), view(k), view(v), ptr("out"), ptr("lse"), 1, T, T, T, 0, *tail, False, 0, 0, 7)
    torch.cuda.synchronize()
    for name, buf in bufs.items():
        assert (buf == -7.0).all(), f"a refused call wrote {name}"


def test_model_packed_documents_match_each_document_alone():
    from collective_communication_mpi_amd import MPI, Communicator
    from collective_communication_mpi_amd.parallel.llama_dp import LlamaBlock, LlamaConfig, LlamaModel

    docs = (67, 190)
    total = sum(docs)
    tp = Communicator(MPI.COMM_WORLD)  # one rank: the TP group of the layers
    cfg = LlamaConfig(d=256, heads=4, kv_heads=2, ffn=256, vocab=512, layers=2, attention="flash")
    packed, alone = (LlamaModel(cfg, tp, torch.device("cuda"), seed=3) for _ in range(2))
    for a, b in zip(packed.parameters(), alone.parameters()):
        assert torch.equal(a, b)
    ids = torch.randint(0, 512, (1, total), device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    targets = torch.roll(ids, -1, dims=1)
    targets[0, docs[0] - 1] = -100
    targets[0, total - 1] = -100
    cu = _cu([0, docs[0], total])

    loss = packed(ids, targets=targets, cu_seqlens=cu)
    loss.backward()
    # each document alone, weighted by its number of predicted tokens
    parts = [alone(ids[:, b:e], targets=targets[:, b:e]) for b, e in ((0, docs[0]), (docs[0], total))]
    weights = [n - 1 for n in docs]
    mean = (weights[0] * parts[0] + weights[1] * parts[1]) / sum(weights)
    mean.backward()
    rel = abs(loss.item() - mean.item()) / abs(mean.item())
    worst = 1.0
    for (name, a), (_, b) in zip(packed.named_parameters(), alone.named_parameters()):
        assert a.grad is not None and b.grad is not None, name
        cos = torch.nn.functional.cosine_similarity(a.grad.double().flatten(), b.grad.double().flatten(), dim=0).item()
        worst = min(worst, cos)
    print(f"[flash varlen model] loss packed={loss.item():.6f} per document={mean.item():.6f} relative difference "
          f"{rel:.3e}; worst gradient cosine {worst:.6f}")
    assert rel <= 2.0 ** -7
    assert worst >= 0.999
    # without the boundaries the second document sees the first: the packing is what the model ran
    assert abs(packed(ids, targets=targets).item() - loss.item()) > 0

    sdpa = LlamaModel(LlamaConfig(d=256, heads=4, kv_heads=2, ffn=256, vocab=512, layers=1, attention="sdpa"), tp,
                      torch.device("cuda"), seed=3)
    with pytest.raises(ValueError, match="cu_seqlens"):
        sdpa(ids, targets=targets, cu_seqlens=cu)
    block = LlamaBlock(cfg, tp, 3, torch.device("cuda"), cp=object())
    with pytest.raises(ValueError, match="cu_seqlens"):
        block(torch.zeros(total, cfg.d, device="cuda", dtype=torch.bfloat16), 1, total, cu)
