"""Flash attention (csrc/device/flash_attn.hip, ``ops.flash_attention``) on one GPU.

Every numeric check is against a full-tensor fp64 reference of the masked softmax composition
and its autograd, on the same bf16 inputs (``randn``) and a random bf16 ``dout``.  The
tolerance is not a fixed number: per tensor (``out``, ``dq``, ``dk``, ``dv``) it is 8 x the
largest absolute error that the fp32 torch composition, rounded once to bf16, makes against
fp64 on that input (measured here), with a floor of 2^-8 x the largest reference magnitude;
the factor pays for bf16 P and dS and for ``delta`` taken from the bf16 ``out``.  ``lse`` is
compared in fp32: absolute error at most 2^-20 x (1 + |lse|).  The worst error / tolerance
ratio per tensor is printed; measured values are in profiles/flash_attention/README.md.

Shapes are a pruned product of S in {1, 63, 128, 257, 515, 2 max(FLASH_BQ, FLASH_BK) + 3},
(Hq, Hkv) in {(1, 1), (4, 2), (8, 1)}, D in {64, 128}, both ``causal`` values, B = 2: one row, a
tile less one, exact tiles, tiles plus one, several tiles with a ragged tail."""
import math

import pytest
import torch

from collective_communication_mpi_amd import _native, ops
from collective_communication_mpi_amd.ops.kernels import FLASH_BK, FLASH_BQ

pytestmark = pytest.mark.gpu

B = 2
S_BIG = 2 * max(FLASH_BQ, FLASH_BK) + 3
# (S, Hq, Hkv, D, causal)
CASES = [
    (1, 1, 1, 64, True), (1, 4, 2, 128, False),
    (63, 1, 1, 128, True), (63, 8, 1, 64, False),
    (128, 4, 2, 64, True), (128, 1, 1, 128, False),
    (257, 4, 2, 64, True), (257, 4, 2, 128, True), (257, 4, 2, 128, False),
    (515, 8, 1, 64, True), (515, 8, 1, 128, True), (515, 8, 1, 64, False),
    (S_BIG, 1, 1, 64, False), (S_BIG, 4, 2, 128, True),
]
FLOOR = 2.0 ** -8
NAMES = ("out", "dq", "dk", "dv")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _inputs(S, Hq, Hkv, D, salt=0):
    g = torch.Generator(device="cuda").manual_seed(4242 + 131 * S + 17 * Hq + 3 * Hkv + D + 7919 * salt)
    mk = lambda h: torch.randn(B, S, h, D, device="cuda", generator=g).bfloat16()
    return mk(Hq), mk(Hkv), mk(Hkv), mk(Hq)  # q, k, v, dout


def _compose(q, k, v, dout, causal, dtype, scale=None):
    """(out, lse, dq, dk, dv) of the masked softmax composition in ``dtype``; dk and dv are
    summed over each kv head's query heads by the autograd of the expansion."""
    Bq, S, Hq, D = q.shape
    rep = Hq // k.shape[2]
    ql, kl, vl = (t.detach().to(dtype).requires_grad_() for t in (q, k, v))
    ke, ve = kl.repeat_interleave(rep, dim=2), vl.repeat_interleave(rep, dim=2)
    s = torch.einsum("bqhd,bkhd->bhqk", ql, ke) * (D ** -0.5 if scale is None else scale)
    if causal:
        s = s.masked_fill(torch.ones(S, S, dtype=torch.bool, device=q.device).triu(1), float("-inf"))
    lse = torch.logsumexp(s, dim=-1)
    out = torch.einsum("bhqk,bkhd->bqhd", torch.softmax(s, dim=-1), ve)
    out.backward(dout.to(dtype))
    return out.detach(), lse.detach(), ql.grad, kl.grad, vl.grad


_REF = {}


def _reference(case, salt=0, edit=None):
    """Inputs, the fp64 reference and the per-tensor tolerances of one case, computed once."""
    key = (case, salt, edit)
    if key not in _REF:
        S, Hq, Hkv, D, causal = case
        q, k, v, dout = _inputs(S, Hq, Hkv, D, salt)
        if edit == "rescale":  # one key of the LAST key tile = 8 x the last query row: the row maximum jumps there
            k[:, S - 1, 0] = 8 * q[:, S - 1, 0]
        ref = _compose(q, k, v, dout, causal, torch.float64)
        f32 = _compose(q, k, v, dout, causal, torch.float32)
        tol = {}
        for name, r, c in zip(NAMES, (ref[0], *ref[2:]), (f32[0], *f32[2:])):
            tol[name] = max(8 * (c.bfloat16().double() - r).abs().max().item(), FLOOR * r.abs().max().item())
        _REF[key] = (q, k, v, dout, ref, tol)
    return _REF[key]


def _run(q, k, v, dout, causal):
    out, lse = ops.flash_attention_forward(q, k, v, causal)
    dq, dk, dv = ops.flash_attention_backward(dout, q, k, v, out, lse, causal)
    return out, lse, dq, dk, dv


def _check(case, got, ref, tol, label):
    out, lse, dq, dk, dv = got
    ratios = {}
    for name, g, r in zip(NAMES, (out, dq, dk, dv), (ref[0], *ref[2:])):
        assert g.dtype == torch.bfloat16 and g.shape == r.shape and g.is_contiguous()
        err = (g.double() - r).abs().max().item()
        ratios[name] = err / tol[name] if tol[name] > 0 else (0.0 if err == 0 else math.inf)  # S = 1: dq and dk are 0
    lse_err = ((lse.double() - ref[1]).abs() / (1 + ref[1].abs())).max().item() * 2.0 ** 20
    print(f"[flash {label}] S={case[0]} Hq={case[1]} Hkv={case[2]} D={case[3]} causal={case[4]}: error / tolerance "
          + " ".join(f"{n}={x:.3f}" for n, x in ratios.items()) + f" lse={lse_err:.3f}")
    assert lse.dtype == torch.float32 and lse.shape == ref[1].shape
    assert lse_err <= 1.0, f"lse error {lse_err:.3f} x 2^-20 (1 + |lse|)"
    for name, x in ratios.items():
        assert x <= 1.0, f"{name}: error is {x:.3f} x the tolerance {tol[name]:.3e}"


def test_constants_match_the_extension():
    dev = _native.device()
    assert (dev.FLASH_BQ, dev.FLASH_BK) == (FLASH_BQ, FLASH_BK)
    assert {c[0] for c in CASES} >= {1, 63, 128, 257, 515, S_BIG}


@pytest.mark.parametrize("case", CASES, ids=lambda c: "S{}-H{}x{}-D{}-{}".format(*c[:4], "causal" if c[4] else "full"))
def test_against_fp64(case):
    q, k, v, dout, ref, tol = _reference(case)
    _check(case, _run(q, k, v, dout, case[4]), ref, tol, "fp64")


@pytest.mark.parametrize("case", [(257, 4, 2, 64, True), (515, 8, 1, 128, False)], ids=["S257-D64-causal", "S515-D128-full"])
def test_autograd_matches_raw(case):
    q, k, v, dout, _, _ = _reference(case)
    want = _run(q, k, v, dout, case[4])
    ql, kl, vl = (t.clone().requires_grad_() for t in (q, k, v))
    out = ops.flash_attention(ql, kl, vl, causal=case[4])
    out.backward(dout)
    for g, w in zip((out.detach(), ql.grad, kl.grad, vl.grad), (want[0], *want[2:])):
        assert torch.equal(g, w)


@pytest.mark.parametrize("S,Hq,Hkv,D", [(S_BIG, 4, 2, 64), (63, 1, 1, 128)])
def test_exact_zeros_under_the_mask(S, Hq, Hkv, D):
    q, k, _, _ = _inputs(S, Hq, Hkv, D, salt=3)
    rows = torch.arange(S, device="cuda")
    for j0 in sorted({j for j in (0, FLASH_BK - 1, FLASH_BK, S - 1) if j < S}):
        v = torch.zeros(B, S, Hkv, D, device="cuda", dtype=torch.bfloat16)
        v[:, j0] = 256.0
        out, _ = ops.flash_attention_forward(q, k, v, True)
        assert (out[:, :j0] == 0).all(), f"j0={j0}: a row before the key is not exactly zero"
        assert (out[:, j0:] != 0).all(), f"j0={j0}: a row that sees the key is zero"
        out, lse = ops.flash_attention_forward(torch.zeros_like(q), k, v, True)
        want = (256.0 / (rows[j0:] + 1).double()).view(1, -1, 1, 1)
        assert (out[:, :j0] == 0).all()
        rel = ((out[:, j0:].double() - want).abs() / want).max().item()
        assert rel <= 2.0 ** -8, f"j0={j0}: uniform rows are off by {rel:.3e} relative"
        assert ((lse.double() - torch.log(rows.double() + 1).view(1, 1, -1)).abs() <= 2.0 ** -20 * (1 + lse.abs())).all()


@pytest.mark.parametrize("case", [(257, 4, 2, 64, True), (515, 8, 1, 128, True), (S_BIG, 4, 2, 128, False)],
                         ids=["S257-D64-causal", "S515-D128-causal", "Sbig-D128-full"])
def test_forced_rescale(case):
    """The running maximum jumps in the last key tile, after earlier tiles were accumulated.
    The kernel has no deferred-rescale threshold, so there is no second build to compare."""
    q, k, v, dout, ref, tol = _reference(case, salt=5, edit="rescale")
    S = case[0]
    assert (S - 1) // FLASH_BK >= 2
    assert (ref[1][:, 0, S - 1] > 30).all()  # the planted score dominates the row
    _check(case, _run(q, k, v, dout, case[4]), ref, tol, "rescale")


def _framed(shape, dtype, sentinel, guard=64):
    n = math.prod(shape)
    buf = torch.full((n + 2 * guard,), sentinel, dtype=dtype, device="cuda")
    return buf, buf[guard:guard + n].view(shape)


@pytest.mark.parametrize("S,Hq,Hkv,D,causal", [(257, 4, 2, 64, True), (S_BIG, 8, 1, 128, False)])
def test_views_and_framing(S, Hq, Hkv, D, causal):
    q, k, v, dout = _inputs(S, Hq, Hkv, D, salt=7)
    want = _run(q, k, v, dout, causal)
    pad = 8
    fused = torch.full((B * S, (Hq + 2 * Hkv) * D + 2 * pad), float("nan"), device="cuda", dtype=torch.bfloat16)
    cols = [pad, pad + Hq * D, pad + (Hq + Hkv) * D, pad + (Hq + 2 * Hkv) * D]
    views = []
    for t, lo, hi, h in zip((q, k, v), cols[:-1], cols[1:], (Hq, Hkv, Hkv)):
        fused[:, lo:hi] = t.reshape(B * S, h * D)
        views.append(fused[:, lo:hi].view(B, S, h, D))
    dfull = torch.full((B * S, Hq * D + 2 * pad), float("nan"), device="cuda", dtype=torch.bfloat16)
    dfull[:, pad:pad + Hq * D] = dout.reshape(B * S, Hq * D)
    dview = dfull[:, pad:pad + Hq * D].view(B, S, Hq, D)
    assert not any(t.is_contiguous() for t in (*views, dview))
    frames = {"out": _framed((B, S, Hq, D), torch.bfloat16, -7.0), "lse": _framed((B, Hq, S), torch.float32, -7.0),
              "dq": _framed((B, S, Hq, D), torch.bfloat16, -7.0), "dk": _framed((B, S, Hkv, D), torch.bfloat16, -7.0),
              "dv": _framed((B, S, Hkv, D), torch.bfloat16, -7.0), "delta": _framed((B, Hq, S), torch.float32, -7.0)}
    out, lse = ops.flash_attention_forward(*views, causal, out=frames["out"][1], lse=frames["lse"][1])
    assert out.data_ptr() == frames["out"][1].data_ptr() and lse.data_ptr() == frames["lse"][1].data_ptr()
    dq, dk, dv = ops.flash_attention_backward(dview, *views, out, lse, causal, dq=frames["dq"][1], dk=frames["dk"][1],
                                              dv=frames["dv"][1], delta=frames["delta"][1])
    for name, g, w in zip(("out", "lse", "dq", "dk", "dv"), (out, lse, dq, dk, dv), want):
        assert g.data_ptr() == frames[name][1].data_ptr()
        assert torch.equal(g, w), f"{name} of the views differs from the contiguous call"
    for name, (buf, view) in frames.items():
        assert (buf[:64] == -7.0).all() and (buf[-64:] == -7.0).all(), f"a sentinel around {name} was overwritten"
        assert not torch.isnan(view).any()


def test_reproducible_and_graph_capturable():
    S, Hq, Hkv, D, causal = 515, 8, 1, 64, True
    q, k, v, dout = _inputs(S, Hq, Hkv, D, salt=11)
    first, second = _run(q, k, v, dout, causal), _run(q, k, v, dout, causal)
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    news = [_inputs(S, Hq, Hkv, D, salt=s) for s in (12, 13)]
    want = [_run(*n, causal) for n in news]
    static = [t.clone() for t in (q, k, v, dout)]
    out, lse = torch.empty_like(first[0]), torch.empty_like(first[1])
    dq, dk, dv, delta = (torch.empty_like(t) for t in (first[2], first[3], first[4], first[1]))
    cs = torch.cuda.Stream()
    cs.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(cs):
        with torch.cuda.graph(g, stream=cs):
            ops.flash_attention_forward(static[0], static[1], static[2], causal, out=out, lse=lse)
            ops.flash_attention_backward(static[3], static[0], static[1], static[2], out, lse, causal, dq=dq, dk=dk,
                                         dv=dv, delta=delta)
    torch.cuda.current_stream().wait_stream(cs)
    for n, w in zip(news, want):
        for s, t in zip(static, n):
            s.copy_(t)
        g.replay()
        torch.cuda.synchronize()
        for a, b in zip((out, lse, dq, dk, dv), w):
            assert torch.equal(a, b)


@pytest.mark.parametrize("D", [64, 128])
def test_gqa_sums_the_group_without_expansion(D):
    """(8, 1): dK and dV equal the sum of the eight query heads' own fp64 gradients."""
    case = (515, 8, 1, D, True)
    q, k, v, dout, ref, tol = _reference(case)
    S = case[0]
    dk_sum = torch.zeros(B, S, 1, D, device="cuda", dtype=torch.float64)
    dv_sum = torch.zeros_like(dk_sum)
    for h in range(8):
        one = _compose(q[:, :, h:h + 1], k, v, dout[:, :, h:h + 1], True, torch.float64)
        dk_sum += one[3]
        dv_sum += one[4]
    assert (dk_sum - ref[3]).abs().max().item() <= 1e-9 * ref[3].abs().max().item()
    _, _, _, dk, dv = _run(q, k, v, dout, True)
    assert dk.shape == (B, S, 1, D) and dv.shape == (B, S, 1, D)
    assert (dk.double() - dk_sum).abs().max().item() <= tol["dk"]
    assert (dv.double() - dv_sum).abs().max().item() <= tol["dv"]


def test_model_flash_matches_sdpa():
    from collective_communication_mpi_amd import MPI, Communicator
    from collective_communication_mpi_amd.parallel.llama_dp import LlamaConfig, LlamaModel

    Bm, S = 2, 257
    tp = Communicator(MPI.COMM_WORLD)  # one rank: the TP group of the layers
    models = {}
    for kind in ("sdpa", "flash"):
        cfg = LlamaConfig(d=256, heads=4, kv_heads=2, ffn=256, vocab=512, layers=2, attention=kind)
        models[kind] = LlamaModel(cfg, tp, torch.device("cuda"), seed=3)
    for a, b in zip(models["sdpa"].parameters(), models["flash"].parameters()):
        assert torch.equal(a, b)
    ids = torch.randint(0, 512, (Bm, S), device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    losses = {}
    for kind, m in models.items():
        loss = m(ids)
        loss.backward()
        losses[kind] = loss.item()
    rel = abs(losses["flash"] - losses["sdpa"]) / abs(losses["sdpa"])
    worst = 1.0
    for (name, a), (_, b) in zip(models["sdpa"].named_parameters(), models["flash"].named_parameters()):
        assert a.grad is not None and b.grad is not None, name
        cos = torch.nn.functional.cosine_similarity(a.grad.double().flatten(), b.grad.double().flatten(), dim=0).item()
        worst = min(worst, cos)
    print(f"[flash model] loss sdpa={losses['sdpa']:.6f} flash={losses['flash']:.6f} relative difference {rel:.3e}; "
          f"worst gradient cosine {worst:.6f}")
    assert rel <= 2.0 ** -7
    assert worst >= 0.999
