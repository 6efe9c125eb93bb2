"""The fused cross-entropy kernels (csrc/device/xent.hip) on one GPU.

Shapes, W = ops.XENT_SWEEP: Vloc in {8, W - 8, W, W + 8, 3 W + 1016} x T in {1, 37}, plus the
smallest (T, Vloc) whose rows are split over several workgroups.  Logits are N(0, 2^2) rounded
to bf16; the shard starts at global column VOCAB_START.  At T = 37: row 3 has its first half
-inf, row 5's target logit is 40 (p - 1 cancels), row 7 is ignored, rows 11 and 12 have their
target in another shard, rows 0 and 1 at the shard's first and last column.  Every shape runs
with contiguous operands and FRAMED: logits a view with padded row stride inside a NaN-filled
buffer, every output a view inside a sentinel-filled buffer, the frame checked afterwards.

The checkers take the op as a bundle of callables; tests/test_cross_entropy_rules.py runs them
without a GPU on a torch emulation and on mutants of it.

Tolerances (reference: ops.cross_entropy_reference, torch fp64 on the same bf16 logits):
* lse, row_loss: the yardstick is the worst error of torch's own fp32 path
  (``torch.logsumexp(logits.float())``, ``F.cross_entropy(logits.float(), reduction="none")``)
  against the same reference, computed here; the kernel's error may be at most 4 x that, with a
  floor of 2 fp32 ulps of |lse|.
* loss_sum: the sum of the rows' bounds plus 2^-20 x sum |row_loss| (at most 16 levels of fp32
  additions, 2^-24 relative each).
* m, zt, hit of the partials: exact (a max of bf16 values, a bf16 value, a flag).
* dlogits: |err| <= 2^-7 |ref| + 2^-20 scale, scale = g / n_valid.  Also: rounding is to
  nearest -- over the non-target, non-zero elements (at least 512 of them) the mean of
  sign(ref) (got - ref) / ulp_bf16(ref) is within 0.1 of 0 (nearest: 0 +- 0.29 / sqrt(N);
  truncation: -0.5).
* ignored rows: exactly 0 in row_loss and dlogits; no valid row: loss 0, dlogits all 0.
"""
import math
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

from collective_communication_mpi_amd import ops
from collective_communication_mpi_amd.ops import cross_entropy_reference

pytestmark = pytest.mark.gpu

W = ops.XENT_SWEEP
VOCAB_START = 4096
IGNORE = -100
GRAD = 1.75
SENT = 777.0
BF16, F32, I64 = torch.bfloat16, torch.float32, torch.int64
NINF = float("-inf")


def _smallest_split_shape():
    """Smallest (T, Vloc) with xent_row_splits > 1: T = 1, the first sweep count that splits."""
    for n in range(1, 65):
        if ops.xent_row_splits(1, (n - 1) * W + 8) > 1:
            return (1, (n - 1) * W + 8)
    return None


SHAPES = [(T, V) for V in (8, W - 8, W, W + 8, 3 * W + 1016) for T in (1, 37)]
if _smallest_split_shape() is not None:  # and the same shard at T = 37, which splits as well
    SHAPES += [_smallest_split_shape(), (37, _smallest_split_shape()[1])]

REAL = SimpleNamespace(stats=ops.cross_entropy_stats, combine=ops.cross_entropy_combine,
                       backward=ops.cross_entropy_backward)


# ---------------------------------------------------------------------------
# cases, frames, references
# ---------------------------------------------------------------------------
def make_case(T, V, device, all_ignored=False):
    g = torch.Generator().manual_seed(1000 * T + V)
    z = (torch.randn(T, V, generator=g) * 2).to(BF16)
    tg = VOCAB_START + torch.randint(0, V, (T,), generator=g)
    if T >= 13:
        tg[0], tg[1] = VOCAB_START, VOCAB_START + V - 1
        z[3, :V // 2] = NINF
        tg[3] = VOCAB_START + V - 2
        z[5, int(tg[5]) - VOCAB_START] = 40.0
        tg[7] = IGNORE
        tg[11] = VOCAB_START + V + 5
        tg[12] = VOCAB_START - 1
    if all_ignored:
        tg[:] = IGNORE
    return z.to(device), tg.to(device)


def framed_flat(shape, dtype, device, fill, margin=8):
    """A contiguous ``shape`` view inside a ``fill``-ed flat buffer: (buffer, view)."""
    n = math.prod(shape)
    buf = torch.full((n + 2 * margin,), fill, dtype=dtype, device=device)
    return buf, buf[margin:margin + n].view(shape)


def framed_rows(T, V, dtype, device, fill):
    """A [T, V] view with row stride V + 16 inside a ``fill``-ed [T + 2, V + 16] buffer."""
    buf = torch.full((T + 2, V + 16), fill, dtype=dtype, device=device)
    return buf, buf[1:T + 1, 8:8 + V]


def frame_intact(buf, view, fill):
    mask = torch.ones(buf.shape, dtype=torch.bool, device=buf.device)
    torch.as_strided(mask, view.shape, view.stride(), view.storage_offset()).fill_(False)
    around = buf[mask]
    return bool(torch.isnan(around).all()) if fill != fill else bool((around == fill).all())


def run(op, z, tg, framed=False, grad=GRAD, inplace=False):
    """stats + combine + backward through ``op``; returns the outputs and the frames' problems."""
    dev = z.device
    T, V = z.shape
    splits = ops.xent_row_splits(T, V)
    problems, frames = [], []
    g = torch.tensor([grad], dtype=F32, device=dev)
    if framed:
        zb, zv = framed_rows(T, V, BF16, dev, float("nan"))
        zv.copy_(z)
        frames.append(("logits", zb, zv, float("nan")))
        out = {}
        for name, shape, dtype, fill in (("stats", (splits, T, 4), F32, SENT), ("lse", (T,), F32, SENT),
                                         ("row_loss", (T,), F32, SENT), ("loss_sum", (1,), F32, SENT),
                                         ("n_valid", (1,), I64, -7)):
            b, v = framed_flat(shape, dtype, dev, fill)
            frames.append((name, b, v, fill))
            out[name] = v
        db, dv = (zb, zv) if inplace else framed_rows(T, V, BF16, dev, SENT)
        if not inplace:
            frames.append(("dlogits", db, dv, SENT))
        stats = op.stats(zv, tg, VOCAB_START, out["stats"])
        lse, row_loss, loss_sum, n_valid = op.combine(stats, tg, IGNORE, out["lse"], out["row_loss"], out["loss_sum"],
                                                      out["n_valid"])
        dl = op.backward(zv, tg, lse, n_valid, g, VOCAB_START, IGNORE, dv)
        for name, b, v, fill in frames:
            if not frame_intact(b, v, fill):
                problems.append(f"{name}: the frame around the view was written")
    else:
        zz = z.clone() if inplace else z
        stats = op.stats(zz, tg, VOCAB_START)
        lse, row_loss, loss_sum, n_valid = op.combine(stats, tg, IGNORE)
        dl = op.backward(zz, tg, lse, n_valid, g, VOCAB_START, IGNORE, zz if inplace else None)
    res = SimpleNamespace(stats=stats, lse=lse, row_loss=row_loss, loss_sum=loss_sum, n_valid=n_valid, dlogits=dl)
    for name in ("stats", "lse", "row_loss", "loss_sum", "dlogits"):
        if torch.isnan(getattr(res, name).float()).any():
            problems.append(f"{name}: a NaN reached the result")
    return res, problems


_REFS = {}


def reference(z, tg, key=None):
    """The fp64 reference of a case and torch's fp32 yardsticks; cached under ``key``."""
    if key is not None and key in _REFS:
        return _REFS[key]
    T, V = z.shape
    stats, lse, row_loss, dl = cross_entropy_reference(z, tg, VOCAB_START, IGNORE, grad=GRAD)
    col = tg - VOCAB_START
    here = (tg != IGNORE) & (col >= 0) & (col < V)
    zf = z.float()
    y_lse = torch.logsumexp(zf, dim=1).double()
    y_loss = F.cross_entropy(zf, torch.where(here, col, torch.full_like(col, IGNORE)), reduction="none",
                             ignore_index=IGNORE).double()
    yard_lse = (y_lse - lse).abs().max().item()
    yard_loss = (y_loss - row_loss)[here].abs().max().item() if bool(here.any()) else 0.0
    n = int((tg != IGNORE).sum())
    ref = SimpleNamespace(stats=stats, lse=lse, row_loss=row_loss, dlogits=dl, yard_lse=yard_lse, yard_loss=yard_loss,
                          n_valid=n, scale=GRAD / n if n else 0.0, valid=tg != IGNORE, col=col, here=here)
    if key is not None:
        _REFS[key] = ref
    return ref


def ulp32(x):
    """One fp32 ulp at |x| (0 at 0)."""
    a = x.abs().double()
    return torch.where(a > 0, torch.exp2(torch.floor(torch.log2(a.clamp_min(1e-300))) - 23), torch.zeros_like(a))


# ---------------------------------------------------------------------------
# checkers: lists of problems, and the worst error / tolerance ratio
# ---------------------------------------------------------------------------
def check_forward(res, ref):
    problems = []
    st, rs = res.stats.double(), ref.stats
    for i, name in ((0, "m"), (2, "zt"), (3, "hit")):
        if not torch.equal(st[:, :, i], rs[:, :, i]):
            problems.append(f"stats: {name} differs from the reference (exact)")
    floor = 2 * ulp32(ref.lse)
    b_lse = torch.maximum(torch.full_like(floor, 4 * ref.yard_lse), floor)
    b_loss = torch.maximum(torch.full_like(floor, 4 * ref.yard_loss), floor)
    e_lse = (res.lse.double() - ref.lse).abs()
    e_loss = (res.row_loss.double() - ref.row_loss).abs()
    r_lse, r_loss = (e_lse / b_lse).max().item(), (e_loss / b_loss).max().item()
    if not r_lse <= 1.0:
        problems.append(f"lse: worst error {e_lse.max().item():.3e} is {r_lse:.2f} x the tolerance")
    if not r_loss <= 1.0:
        problems.append(f"row_loss: worst error {e_loss.max().item():.3e} is {r_loss:.2f} x the tolerance")
    if bool((res.row_loss[~ref.valid] != 0).any()):
        problems.append("row_loss: an ignored row is not exactly 0")
    if int(res.n_valid.item()) != ref.n_valid:
        problems.append(f"n_valid: {int(res.n_valid.item())}, expected {ref.n_valid}")
    want = ref.row_loss.sum().item()
    b_sum = b_loss[ref.valid].sum().item() + 2.0 ** -20 * ref.row_loss.abs().sum().item()
    e_sum = abs(res.loss_sum.double().item() - want)
    if not e_sum <= b_sum:
        problems.append(f"loss_sum: error {e_sum:.3e} above the tolerance {b_sum:.3e}")
    return problems, max(r_lse, r_loss)


def check_backward(res, ref):
    problems = []
    got, want = res.dlogits.double(), ref.dlogits
    if tuple(got.shape) != tuple(want.shape):
        return [f"dlogits: shape {tuple(got.shape)}"], float("inf")
    if bool((got[~ref.valid] != 0).any()):
        problems.append("dlogits: an ignored row is not exactly 0")
    if ref.n_valid == 0:
        if bool((got != 0).any()):
            problems.append("dlogits: not all 0 with no valid row")
        return problems, 0.0
    err = (got - want).abs()
    bound = 2.0 ** -7 * want.abs() + 2.0 ** -20 * abs(ref.scale)
    ratio = (err / bound).max().item()
    if not ratio <= 1.0:
        i = int((err / bound).argmax())
        problems.append(f"dlogits: error is {ratio:.2f} x the tolerance at row {i // got.shape[1]}, column "
                        f"{i % got.shape[1]}")
    # round to nearest: no bias towards 0
    pick = (want != 0) & ref.valid[:, None]
    rows = torch.nonzero(ref.here)[:, 0]
    pick[rows, ref.col[ref.here]] = False
    if int(pick.sum()) >= 512:
        w = want[pick]
        ulp = torch.exp2(torch.floor(torch.log2(w.abs())) - 7)
        bias = (torch.sign(w) * (got[pick] - w) / ulp).mean().item()
        if not abs(bias) <= 0.1:
            problems.append(f"dlogits: mean signed rounding error {bias:+.3f} bf16 ulps (round to nearest: 0)")
    return problems, ratio


def check_case(op, T, V, device, framed, all_ignored=False):
    """The whole recipe for one shape: returns (problems, ratios)."""
    z, tg = make_case(T, V, device, all_ignored)
    ref = reference(z, tg, (T, V, all_ignored, str(device)))
    res, problems = run(op, z, tg, framed)
    pf, rf = check_forward(res, ref)
    pb, rb = check_backward(res, ref)
    if all_ignored and res.loss_sum.item() != 0:
        pf.append("loss_sum: not 0 with no valid row")
    return problems + pf + pb, (rf, rb)


# ---------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------
DEV = "cuda"


def _same(a, b):
    return all(torch.equal(getattr(a, n), getattr(b, n)) for n in ("stats", "lse", "row_loss", "loss_sum", "n_valid",
                                                                   "dlogits"))


@pytest.mark.parametrize("framed", [False, True], ids=["contiguous", "framed"])
@pytest.mark.parametrize("T,V", SHAPES)
def test_against_fp64(T, V, framed):
    assert ops.XENT_SWEEP == ops.kernels._D().XENT_SWEEP and ops.XENT_CHUNK == ops.kernels._D().XENT_CHUNK
    assert ops.xent_row_splits(T, V) == ops.kernels._D().xent_row_splits(T, V)
    problems, (rf, rb) = check_case(REAL, T, V, DEV, framed)
    print(f"xent T={T} Vloc={V} {'framed' if framed else 'contiguous'} splits={ops.xent_row_splits(T, V)}: worst error "
          f"/ tolerance lse|row_loss={rf:.3f} dlogits={rb:.3f}")
    assert not problems, "\n".join(problems)
    z, tg = make_case(T, V, DEV)
    a, _ = run(REAL, z, tg, framed)
    b, _ = run(REAL, z, tg, framed)
    assert _same(a, b), "two calls differ bitwise"


@pytest.mark.parametrize("framed", [False, True], ids=["contiguous", "framed"])
def test_every_row_ignored(framed):
    problems, _ = check_case(REAL, 37, W + 8, DEV, framed, all_ignored=True)
    assert not problems, "\n".join(problems)
    z, tg = make_case(37, W + 8, DEV, all_ignored=True)
    loss = ops.cross_entropy(z.requires_grad_(), tg)
    loss.backward()
    assert loss.item() == 0.0 and not bool((z.grad != 0).any())


def test_rows_do_not_depend_on_each_other():
    T, V, a, b = 37, 3 * W + 1016, 9, 20
    assert ops.xent_row_splits(T, V) == ops.xent_row_splits(b - a, V)  # the splits are part of the bits
    z, tg = make_case(T, V, DEV)
    full, _ = run(REAL, z, tg)
    part, _ = run(REAL, z[a:b], tg[a:b].contiguous())
    assert torch.equal(part.lse, full.lse[a:b]) and torch.equal(part.row_loss, full.row_loss[a:b])
    assert torch.equal(part.stats, full.stats[:, a:b])


@pytest.mark.parametrize("framed", [False, True], ids=["contiguous", "framed"])
@pytest.mark.parametrize("T,V", [(37, W + 8), SHAPES[-2]])
def test_in_place(T, V, framed):
    z, tg = make_case(T, V, DEV)
    want, _ = run(REAL, z, tg, framed)
    got, problems = run(REAL, z, tg, framed, inplace=True)
    assert not problems, problems
    assert torch.equal(got.dlogits, want.dlogits)


def test_autograd():
    T, V = 37, W + 8
    z, tg = make_case(T, V, DEV)
    tg = torch.where(tg == IGNORE, tg, (tg - VOCAB_START).clamp(0, V - 1))
    stats = ops.cross_entropy_stats(z, tg)
    lse, _, loss_sum, n_valid = ops.cross_entropy_combine(stats, tg)
    zz = z.clone().requires_grad_()
    loss = ops.cross_entropy(zz, tg)
    assert loss.dtype == F32 and loss.dim() == 0
    assert torch.equal(loss, (loss_sum / n_valid)[0])
    up = torch.tensor(3.5, device=DEV)  # a device tensor: nothing is read on the host
    (loss * up).backward()
    want = ops.cross_entropy_backward(z, tg, lse, n_valid, up.reshape(1))
    assert torch.equal(zz.grad, want)
    ref = F.cross_entropy(z.float(), tg)
    assert abs(loss.item() - ref.item()) <= 1e-5 * abs(ref.item())


def test_graph_replay():
    T, V = 37, 3 * W + 1016
    z, tg = make_case(T, V, DEV)
    z2, tg2 = make_case(T, V + 8, DEV)
    z2, tg2 = z2[:, :V].contiguous(), torch.where(tg2 == IGNORE, tg2, tg2.clamp(max=VOCAB_START + V - 1))
    zs, ts = z.clone(), tg.clone()
    g = torch.tensor([GRAD], dtype=F32, device=DEV)
    stats = torch.empty((ops.xent_row_splits(T, V), T, 4), dtype=F32, device=DEV)
    lse, row_loss = torch.empty(T, dtype=F32, device=DEV), torch.empty(T, dtype=F32, device=DEV)
    loss_sum, n_valid = torch.empty(1, dtype=F32, device=DEV), torch.empty(1, dtype=I64, device=DEV)
    work = torch.empty(((T + ops.XENT_CHUNK - 1) // ops.XENT_CHUNK, 2), dtype=F32, device=DEV)
    dl = torch.empty_like(zs)

    def step():
        ops.cross_entropy_stats(zs, ts, VOCAB_START, stats)
        ops.cross_entropy_combine(stats, ts, IGNORE, lse, row_loss, loss_sum, n_valid, work=work)
        ops.cross_entropy_backward(zs, ts, lse, n_valid, g, VOCAB_START, IGNORE, dl)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    zs.copy_(z2)
    ts.copy_(tg2)
    graph.replay()
    torch.cuda.synchronize()
    want, _ = run(REAL, z2, tg2)
    assert torch.equal(lse, want.lse) and torch.equal(row_loss, want.row_loss) and torch.equal(dl, want.dlogits)
    assert torch.equal(loss_sum, want.loss_sum) and torch.equal(n_valid, want.n_valid)


def test_offsets_past_2_31_elements():
    T, V, stride = 131080, 16384, 16392
    assert T * stride > 1 << 31
    buf = torch.empty(T * stride, dtype=BF16, device=DEV)
    z = buf.view(T, stride)[:, :V]
    g = torch.Generator(device=DEV).manual_seed(31)
    for i in range(0, T, 8192):
        n = min(8192, T - i)
        z[i:i + n] = (torch.randn(n, V, device=DEV, generator=g) * 2).to(BF16)
    buf.view(T, stride)[:, V:] = float("nan")
    tg = VOCAB_START + torch.randint(0, V, (T,), device=DEV, generator=g)
    mid = T // 2
    tg[mid] = IGNORE
    rows = torch.tensor([0, 1, mid, T - 2, T - 1], device=DEV)
    zr, tr = z[rows].clone(), tg[rows].clone()
    gr = torch.tensor([GRAD], dtype=F32, device=DEV)
    stats = ops.cross_entropy_stats(z, tg, VOCAB_START)
    lse, row_loss, loss_sum, n_valid = ops.cross_entropy_combine(stats, tg, IGNORE)
    dl = ops.cross_entropy_backward(z, tg, lse, n_valid, gr, VOCAB_START, IGNORE, z)
    assert dl.data_ptr() == z.data_ptr() and int(n_valid.item()) == T - 1
    _, r_lse, r_loss, r_dl = cross_entropy_reference(zr, tr, VOCAB_START, IGNORE, grad=GRAD, n_valid=T - 1)
    ref = SimpleNamespace(stats=None, lse=r_lse, row_loss=r_loss, dlogits=r_dl, n_valid=T - 1, scale=GRAD / (T - 1),
                          valid=tr != IGNORE, col=tr - VOCAB_START, here=tr != IGNORE)
    y = (torch.logsumexp(zr.float(), 1).double() - r_lse).abs().max().item()
    bound = torch.maximum(torch.full_like(r_lse, 4 * y), 2 * ulp32(r_lse))
    assert bool(((lse[rows].double() - r_lse).abs() <= bound).all())
    assert bool(((row_loss[rows].double() - r_loss).abs() <= bound).all()) and row_loss[mid].item() == 0.0
    problems, _ = check_backward(SimpleNamespace(dlogits=z[rows]), ref)
    assert not problems, "\n".join(problems)
    assert not bool((z[mid] != 0).any())
    assert bool(torch.isnan(buf.view(T, stride)[:, V:].float()).all()), "the padding was written"
    total = row_loss.double().sum().item()  # loss_sum against its own rows: the summation tree's error alone
    assert abs(loss_sum.double().item() - total) <= 2.0 ** -20 * total


def test_refused_calls_write_nothing():
    T, V = 5, 64
    z, tg = make_case(T, V, DEV)
    sb, stats = framed_flat((1, T, 4), F32, DEV, SENT)
    db, dl = framed_rows(T, V, BF16, DEV, SENT)
    lse, n_valid = torch.zeros(T, device=DEV), torch.ones(1, dtype=I64, device=DEV)
    wide = torch.zeros(T, V + 8, dtype=BF16, device=DEV)
    calls = [
        (TypeError, lambda: ops.cross_entropy_stats(z.float(), tg, 0, stats)),
        (TypeError, lambda: ops.cross_entropy_stats(z, tg.int(), 0, stats)),
        (ValueError, lambda: ops.cross_entropy_stats(z[:, :60], tg, 0, stats)),
        (ValueError, lambda: ops.cross_entropy_stats(wide[:, 4:4 + V], tg, 0, stats)),
        (ValueError, lambda: ops.cross_entropy_stats(z, tg[:4], 0, stats)),
        (ValueError, lambda: ops.cross_entropy_stats(z, tg.cpu(), 0, stats)),
        (ValueError, lambda: ops.cross_entropy_stats(z, tg, -1, stats)),
        (ValueError, lambda: ops.cross_entropy_stats(z, tg, 0, stats.view(T, 4))),
        (ValueError, lambda: ops.cross_entropy_backward(z, tg, lse, n_valid, None, 0, IGNORE, dl[:, :56])),
        (ValueError, lambda: ops.cross_entropy_backward(z, tg, lse[:4], n_valid, None, 0, IGNORE, dl)),
        (TypeError, lambda: ops.cross_entropy_backward(z, tg, lse.double(), n_valid, None, 0, IGNORE, dl)),
        (ValueError, lambda: ops.cross_entropy_combine(stats, tg[:4])),
    ]
    for exc, call in calls:
        with pytest.raises(exc):
            call()
    torch.cuda.synchronize()
    assert bool((sb == SENT).all()) and bool((db == SENT).all())
