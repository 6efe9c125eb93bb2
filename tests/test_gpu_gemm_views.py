"""Every dense GEMM route, bit for bit, on framed views.

Operands are integer-valued bf16 (``_ints``), so every partial sum of every route -- any
summation order, split-K, atomics -- is an integer (a half-integer under ``alpha = 0.5``)
below 2^24: the fp32 result is exact and a bf16 output is one round-to-nearest-even of it.
Each output is compared bitwise with an fp64 reference; no tolerance anywhere
(tests/test_gemm_exact_recipe.py checks the recipe itself on the CPU).

Nothing is a tight tensor unless a form says so: operands are views of NaN-filled buffers
(a column window at an offset, a row slice), outputs are views of buffers filled with the
sentinel -512, and after every call the buffer outside the view must still be all sentinel,
the view free of NaN and equal to the reference.  Reads of an operand's frame that only
reach values that are never stored are legitimate; results and output frames are asserted.

One pytest case is (route, shape, K); inside it every form of the table that applies to
the op runs on the same operands and the same fp64 product, and every failing form is
reported.  Routes are forced with the existing setters and restored in ``finally``.
"""
import contextlib
import math
import os
from collections import namedtuple

import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = -512.0
F32, BF16 = torch.float32, torch.bfloat16
PAIR = 16384  # ring schedule bit 14: pair slots


# ---------------------------------------------------------------------------
# data recipe and frames (no GPU needed; the recipe module imports these)
# ---------------------------------------------------------------------------
def _rmax(K):
    """Largest operand magnitude for reduction length K: K * R^2 <= 2^23."""
    return min(64, math.isqrt(2 ** 23 // K))


def _int_values(shape, R, gen):
    return torch.randint(-R, R + 1, tuple(shape), generator=gen, dtype=torch.int32)


def _ints(shape, R, gen):
    """Integer-valued bf16 in [-R, R] (CPU generator, CPU tensor)."""
    return _int_values(shape, R, gen).to(BF16)


def _framed(rows, cols, dtype, fill, before=3, after=3, col_off=0, col_pad=8, device="cuda"):
    """``(buffer, view)``: a [before + rows + after, col_off + cols + col_pad] buffer filled
    with ``fill`` and its [rows, cols] window at (before, col_off)."""
    buf = torch.full((before + rows + after, col_off + cols + col_pad), fill, dtype=dtype, device=device)
    return buf, buf[before:before + rows, col_off:col_off + cols]


def _place(t, how):
    """Operand ``t`` as the form wants it: ``tight``, ``window`` (columns 8.. of a wider NaN
    buffer, 3 NaN rows before and after) or ``rows`` (a row slice: column offset 0, row
    stride > cols).  Row strides stay multiples of 8 elements: 16-B rows are the ops' contract."""
    if how == "tight":
        return t.contiguous()
    rows, cols = t.shape
    col_off = 8 if how == "window" else 0
    pad = 8 + (-(col_off + cols + 8)) % 8
    _, v = _framed(rows, cols, t.dtype, float("nan"), 3, 3, col_off, pad, device=t.device)
    v.copy_(t)
    return v


def _out_frame(rows, cols, dtype, how="aligned", col_off=None, device="cuda"):
    """Sentinel-framed output view.  ``aligned``: 16-B aligned start and rows; ``off1``: the
    view starts one element into a 16-B aligned row (misaligned C); ``oddld``: an aligned
    start with an odd row stride."""
    before, off = {"aligned": (3, 8), "off1": (3, 1), "oddld": (8, 8)}[how]
    if col_off is not None:
        off = col_off
    ld = off + cols + 8
    pad = 8 + ((ld + 1) % 2 if how == "oddld" else -ld % 8)
    return _framed(rows, cols, dtype, SENTINEL, before, 3, off, pad, device=device)


def _frame_damage(buf, view):
    """Cells of ``buf`` outside ``view`` that no longer hold the sentinel."""
    r0, c0 = divmod(view.storage_offset() - buf.storage_offset(), buf.stride(0))
    chk = buf.clone()
    chk[r0:r0 + view.shape[0], c0:c0 + view.shape[1]] = SENTINEL
    return int((chk != SENTINEL).sum())  # NaN != sentinel too


def _check(buf, view, ref64, tag):
    """Failures of one output against the exact fp64 reference, as strings."""
    errs = []
    ref64 = ref64 + 0.0  # no negative zeros in the reference
    exp = ref64.to(F32)
    if not torch.equal(exp.double(), ref64):
        errs.append(f"{tag}: the reference is not exact in fp32 (recipe broken)")
    if view.dtype == BF16:
        exp = exp.to(BF16)
    bad = _frame_damage(buf, view)
    if bad:
        errs.append(f"{tag}: {bad} cells of the output frame were overwritten")
    got = view.contiguous()
    nans = int(torch.isnan(got.float()).sum())
    if nans:
        errs.append(f"{tag}: {nans} NaN in the output")
    bits = torch.int16 if view.dtype == BF16 else torch.int32
    ne = got.view(bits) != exp.view(bits)
    if bool(ne.any()):
        i, j = [int(x) for x in ne.nonzero()[0]]
        errs.append(f"{tag}: {int(ne.sum())} of {ne.numel()} values differ bitwise; first at ({i}, {j}): "
                    f"got {float(got[i, j])!r}, expected {float(exp[i, j])!r} (exact {float(ref64[i, j])!r})")
    return errs


def _untouched(buf, tag):
    bad = int((buf != SENTINEL).sum())
    return [f"{tag}: a refused call wrote {bad} cells"] if bad else []


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@contextlib.contextmanager
def _knobs(kernel=0, w4=1, smallk=(128, 0), ring_sched=8 | PAIR, pair_ta=0, tn_pf=0, tn_variant=None, env=None):
    """Force a route with the ops' own setters; the process defaults come back in ``finally``."""
    from collective_communication_mpi_amd import _native
    from collective_communication_mpi_amd.ops.kernels import set_tn_variant

    D = _native.device()
    saved = {k: os.environ.get(k) for k in (env or {})}
    try:
        D.gemm_set_kernel(kernel)
        D.gemm_set_w4_sched(w4)
        D.gemm_set_smallk(*smallk)
        D.gemm_set_ring_sched(ring_sched)
        D.gemm_set_pair_ta(pair_ta)
        D.gemm_tn_set_prefetch(tn_pf)
        set_tn_variant(tn_variant)
        os.environ.update(env or {})
        yield D
    finally:
        D.gemm_set_kernel(0)
        D.gemm_set_w4_sched(1)
        D.gemm_set_smallk(128, 0)
        D.gemm_set_ring_sched(8 | PAIR)
        D.gemm_set_pair_ta(0)
        D.gemm_tn_set_prefetch(0)
        set_tn_variant(None)
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _seed(*xs):
    s = 12345
    for x in xs:
        s = (s * 1000003 + int(x)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


# ---------------------------------------------------------------------------
# gemm_nt: one table of routes, one table of forms
# ---------------------------------------------------------------------------
# out dtype, alpha, bias dtype, act, accumulate, splitk, output view, A view, B view,
# ncut (drop this many rows of B: N % 8 != 0 with an aligned C)
Form = namedtuple("Form", "id out alpha bias act acc splitk c a b ncut",
                  defaults=(F32, 1.0, None, None, False, 1, "aligned", "tight", "tight", 0))

NT_FORMS = [
    Form("f32"),
    Form("f32-auto", splitk=None),
    Form("f32-half-biasf32", alpha=0.5, bias=F32),
    Form("f32-biasbf16", bias=BF16),  # the last fast epilogue id (5): fp32 out, bf16 bias
    Form("f32-half-biasbf16-relu", alpha=0.5, bias=BF16, act="relu"),
    Form("bf16", out=BF16),
    Form("bf16-half", out=BF16, alpha=0.5),
    Form("bf16-biasf32", out=BF16, bias=F32),
    Form("bf16-half-biasbf16", out=BF16, alpha=0.5, bias=BF16),
    Form("bf16-biasf32-relu", out=BF16, bias=F32, act="relu"),
    Form("f32-acc-half", alpha=0.5, acc=True),
    Form("bf16-acc-biasf32", out=BF16, bias=F32, acc=True),
    Form("bf16-acc-half", out=BF16, alpha=0.5, acc=True),
    Form("f32-split2-half-biasf32", alpha=0.5, bias=F32, splitk=2),
    Form("f32-split3-biasbf16", bias=BF16, splitk=3),
    Form("f32-split3-acc-biasf32", bias=F32, acc=True, splitk=3),
    Form("f32-split2-oddld", splitk=2, c="oddld"),
    Form("f32-split2-off1-biasf32", bias=F32, splitk=2, c="off1"),
    Form("f32-off1", c="off1"),
    Form("bf16-off1-half-biasbf16", out=BF16, alpha=0.5, bias=BF16, c="off1"),
    Form("f32-oddld-biasf32", bias=F32, c="oddld"),
    Form("bf16-oddld-acc", out=BF16, acc=True, c="oddld"),
    Form("bf16-oddld", out=BF16, c="oddld"),
    Form("f32-ncut", ncut=3),
    Form("bf16-ncut-half-biasf32", out=BF16, alpha=0.5, bias=F32, ncut=3),
    Form("bf16-ncut-acc", out=BF16, acc=True, ncut=3),
    Form("bf16-windowA-rowsB", out=BF16, a="window", b="rows"),
    Form("f32-rowsA-windowB-half", alpha=0.5, a="rows", b="window"),
    Form("f32-split3-windowA-windowB", splitk=3, a="window", b="window"),
]

_S128 = [(130, 72), (1, 8), (257, 136)]   # 128x128 tiles: > 1 tile and a partial tile in M and N
_S256 = [(260, 264), (1, 8), (300, 520)]  # 256-row tiles, 128 / 192 / 256 columns
_SSK = [(256, 72), (330, 264)]            # small-K: M >= 256, 64-row tiles, 128 / 256 column slices

# id -> (knobs, runs on the LDS ring, shapes, K list).  K lists give 1, 2, an odd >= 3 and an
# even >= 4 steps of the kernel's own K step (64; 128 for the ping-pong kernels; 32 for small K,
# which stops at K = 96).  The four-wave and ring routes switch the small-K kernel off: with it on,
# K <= 96 and M >= 256 never reaches them.
NT_ROUTES = {
    "regs": (dict(kernel=1), False, _S128, (8, 72, 136, 200)),
    "glds": (dict(kernel=1), False, _S128, (64, 128, 192, 256)),
    "smallk128": (dict(smallk=(128, 2048)), False, _SSK, (8, 40, 72, 96)),
    "smallk256": (dict(smallk=(256, 2048)), False, _SSK, (8, 40, 72, 96)),
    "smallk128-walk": (dict(smallk=(128, 1)), False, _SSK, (8, 72)),  # grid cap 1: one block per N slice walks every M tile
    "pp256": (dict(kernel=2), False, _S256, (128, 256, 384, 512)),
    "pp192": (dict(kernel=4), False, _S256, (128, 256, 384, 512)),
    "pp128": (dict(kernel=3), False, _S256, (128, 256, 384, 512)),
}
for _s in (0, 1, 3, 4, 5):
    NT_ROUTES[f"w4-{_s}"] = (dict(kernel=5, w4=_s, smallk=(0, 0)), False, _S256, (64, 128, 192, 256, 320))
for _s, _n in ((8, "ring"), (9, "ringp"), (8 | PAIR, "pair"), (9 | PAIR, "pairp")):
    NT_ROUTES[_n] = (dict(kernel=5, w4=_s, smallk=(0, 0)), True, _S256, (64, 128, 192, 256, 320))

NT_CASES = [pytest.param(r, M, N, K, id=f"{r}-{M}x{N}x{K}")
            for r, (_, _, shapes, ks) in NT_ROUTES.items() for (M, N) in shapes for K in ks]


def _splitk_eff(f, M, N, K):
    from collective_communication_mpi_amd.ops.kernels import _auto_splitk

    if f.splitk is not None:
        return f.splitk
    if f.out == F32 and f.act is None:
        return _auto_splitk(((M + 127) // 128) * ((N + 127) // 128), K)
    return 1


def _run_nt_forms(D, ring, M, N, K, forms, seed):
    from collective_communication_mpi_amd.ops import gemm_nt

    gen = _seed(M, N, K, seed)
    R = _rmax(K)
    a = _ints((M, K), R, gen).cuda()
    b = _ints((N, K), R, gen).cuda()
    bias = _ints((N,), 64, gen).cuda()
    prior = _ints((M, N), 64, gen).cuda()
    P = a.double() @ b.double().T
    errs = []
    for f in forms:
        n = max(1, N - f.ncut)
        av, bv = _place(a, f.a), _place(b[:n], f.b)
        ref = f.alpha * P[:, :n]
        bias_t = None
        if f.bias is not None:
            bias_t = bias[:n].to(f.bias).contiguous()
            ref = ref + bias[:n].double()
        if f.act == "relu":
            ref = ref.clamp_min(0.0)
        if f.acc:
            ref = ref + prior[:, :n].double()
        buf, out = _out_frame(M, n, f.out, f.c)
        if f.acc:
            out.copy_(prior[:, :n])
        n0 = D.gemm_ring_launches()
        y = gemm_nt(av, bv, out=out, bias=bias_t, alpha=f.alpha, accumulate=f.acc, act=f.act, splitk=f.splitk)
        assert y is out
        launched = D.gemm_ring_launches() - n0
        want = int(ring and _splitk_eff(f, M, n, K) == 1 and K % 64 == 0)
        if launched != want:
            errs.append(f"{f.id}: {launched} LDS-ring launches, expected {want}")
        errs += _check(buf, out, ref, f.id)
    return errs


@pytest.mark.parametrize("route,M,N,K", NT_CASES)
def test_gemm_nt_route(route, M, N, K):
    knobs, ring, _, _ = NT_ROUTES[route]
    with _knobs(**knobs) as D:
        errs = _run_nt_forms(D, ring, M, N, K, NT_FORMS, seed=len(route))
    assert not errs, f"{len(errs)} failures:\n" + "\n".join(errs)


# persistent wrap-around: more 256x256 tiles than CUs, so tiles - CUs of the persistent workgroups
# (33 of 256 on an MI355X) take a second tile, whose first loads are issued from the first
# tile's epilogue
WRAP_SCHEDS = [pytest.param(1, False, id="w4p"), pytest.param(3, False, id="w4po"), pytest.param(5, False, id="w4pf"),
               pytest.param(9, True, id="ringp"), pytest.param(9 | PAIR, True, id="pairp")]


def _wrap_shape():
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    tn = 16                                  # 17 tile columns (not a multiple of the group-M of 8)
    tm = max(16, -(-cus // (tn + 1)))        # (tm + 1) * 17 > CUs
    while (tm + 1) % 8 == 0 or (tm + 1) * (tn + 1) <= cus:
        tm += 1
    return 256 * tm + 4, 256 * tn + 8, 128, cus


@pytest.fixture(scope="module")
def wrap_data():
    M, N, K, cus = _wrap_shape()
    gen = _seed(M, N, K)
    a = _ints((M, K), _rmax(K), gen).cuda()
    b = _ints((N, K), _rmax(K), gen).cuda()
    return M, N, K, cus, a, b, a.double() @ b.double().T


@pytest.mark.parametrize("sched,ring", WRAP_SCHEDS)
def test_gemm_nt_persistent_wrap(wrap_data, sched, ring):
    from collective_communication_mpi_amd.ops import gemm_nt

    M, N, K, cus, a, b, P = wrap_data
    assert -(-M // 256) * -(-N // 256) > cus
    errs = []
    with _knobs(kernel=5, w4=sched, smallk=(0, 0)) as D:
        # the ring's persistent grid takes the fast bf16 form only; the four-wave kernel any output
        for dt in ((BF16,) if ring else (BF16, F32)):
            buf, out = _out_frame(M, N, dt)
            n0 = D.gemm_ring_launches()
            gemm_nt(a, b, out=out, splitk=1)
            if D.gemm_ring_launches() - n0 != int(ring):
                errs.append(f"{dt}: LDS-ring launches {D.gemm_ring_launches() - n0}, expected {int(ring)}")
            errs += _check(buf, out, P, str(dt))
            del buf, out
    assert not errs, "\n".join(errs)


def test_gemm_nt_refusals():
    """Arguments outside the contract raise and write nothing."""
    from collective_communication_mpi_amd.ops import gemm_nt

    M, N, K = 130, 72, 64
    gen = _seed(M, N, K, 99)
    a, b = _ints((M, K), 64, gen).cuda(), _ints((N, K), 64, gen).cuda()
    errs = []

    def refused(tag, exc, av, bv, dt=F32, **kw):
        buf, out = _out_frame(M, N, dt)
        with pytest.raises(exc):
            gemm_nt(av, bv, out=out, **kw)
        errs.extend(_untouched(buf, tag))

    def shifted(t, col_off, col_pad, before=3):
        _, v = _framed(t.shape[0], t.shape[1], BF16, float("nan"), before, 3, col_off, col_pad)
        v.copy_(t)
        return v

    for v in (shifted(a, 4, 4), shifted(b, 4, 4)):     # 8 B off, row stride fine
        assert v.data_ptr() % 16 == 8 and v.stride(0) % 8 == 0
    for v in (shifted(a, 0, 4, 4), shifted(b, 0, 4, 4)):  # 16-B aligned start (4 rows in), rows are not
        assert v.data_ptr() % 16 == 0 and v.stride(0) % 8 == 4

    refused("a at col_off 4", ValueError, shifted(a, 4, 4), b)          # lda % 8 == 0, A 8 B off
    refused("b at col_off 4", ValueError, a, shifted(b, 4, 4))
    refused("lda % 8 != 0", ValueError, shifted(a, 0, 4, 4), b)
    refused("ldb % 8 != 0", ValueError, a, shifted(b, 0, 4, 4))
    refused("split-K, bf16 out", ValueError, a, b, dt=BF16, splitk=2)
    refused("split-K, relu", ValueError, a, b, act="relu", splitk=2)
    assert not errs, "\n".join(errs)


# ---------------------------------------------------------------------------
# gemm_ring: four operand layouts, every route of the K-major dispatcher
# ---------------------------------------------------------------------------
# ncut: drop this many rows of op(b): N % 8 != 0 with an aligned C (a K-contiguous b takes it;
# a tight K-major b then has rows that are no 16-B multiples and is refused)
RingForm = namedtuple("RingForm", "id out alpha acc a b ncut", defaults=(F32, 1.0, False, "tight", "tight", 0))
RING_FORMS = [
    RingForm("f32"),
    RingForm("bf16-half", out=BF16, alpha=0.5),
    RingForm("bf16", out=BF16),
    RingForm("f32-acc-half", alpha=0.5, acc=True),
    RingForm("bf16-acc", out=BF16, acc=True),
    RingForm("bf16-windowA-rowsB", out=BF16, a="window", b="rows"),
    RingForm("f32-rowsA-windowB-acc", acc=True, a="rows", b="window"),
    RingForm("bf16-windowA-windowB-half", out=BF16, alpha=0.5, a="window", b="window"),
    RingForm("bf16-ncut-half", out=BF16, alpha=0.5, ncut=3),
    RingForm("f32-ncut-acc-rowsB", acc=True, b="rows", ncut=3),
]
_LOW = {"CCMPI_KMAJOR_MIN_DIM": "8", "CCMPI_KMAJOR_MIN_MACS": "1"}
# id -> (knobs, layouts, op(a) passed as a_nt)
RING_ROUTES = {
    "slot4": (dict(ring_sched=8, env={"CCMPI_KMAJOR_ROUTE": "ring"}), [(0, 0), (0, 1), (1, 1), (1, 0)], False),
    "pair": (dict(ring_sched=8 | PAIR, pair_ta=1, env={"CCMPI_KMAJOR_ROUTE": "pair"}),
             [(0, 0), (0, 1), (1, 1), (1, 0)], False),
    "pair-ta0": (dict(ring_sched=8 | PAIR, pair_ta=0, env={"CCMPI_KMAJOR_ROUTE": "pair"}), [(1, 0)], False),
    "transpose": (dict(ring_sched=8 | PAIR, env={"CCMPI_KMAJOR_ROUTE": "transpose", **_LOW}), [(1, 1), (1, 0)], False),
    "a_nt": (dict(ring_sched=8 | PAIR, env={"CCMPI_KMAJOR_ROUTE": "ring"}), [(1, 1), (1, 0)], True),
}
_SRING = [(264, 520), (8, 8), (776, 264)]
RING_K = (64, 128, 192, 256, 320)  # 1, 2, 3, 4 and 5 steps of 64
RING_CASES = [pytest.param(r, ta, tb, M, N, K, id=f"{r}-ta{ta}tb{tb}-{M}x{N}x{K}")
              for r, (_, lay, _) in RING_ROUTES.items() for (ta, tb) in lay for (M, N) in _SRING
              for K in RING_K]


@pytest.mark.parametrize("route,ta,tb,M,N,K", RING_CASES)
def test_gemm_ring_route(route, ta, tb, M, N, K):
    """K-major operands: the NaN rows after a framed view are the rows past the reduction."""
    from collective_communication_mpi_amd.ops import gemm_ring

    knobs, _, use_a_nt = RING_ROUTES[route]
    gen = _seed(M, N, K, ta, tb, len(route))
    R = _rmax(K)
    a = _ints((K, M) if ta else (M, K), R, gen).cuda()
    b = _ints((K, N) if tb else (N, K), R, gen).cuda()
    prior = _ints((M, N), 64, gen).cuda()
    P = (a.double().T if ta else a.double()) @ (b.double() if tb else b.double().T)
    errs = []
    with _knobs(**knobs) as D:
        for f in RING_FORMS:
            n = max(1, N - f.ncut)
            if f.ncut and tb:  # op(b) = b.T: a tight [K, n] has ldb = n, no multiple of 8 elements
                buf, out = _out_frame(M, n, f.out)
                n0 = D.gemm_ring_launches()
                y = gemm_ring(_place(a, f.a), b[:, :n].contiguous(), bool(ta), True, out=out, alpha=f.alpha)
                if y is not None or D.gemm_ring_launches() != n0:
                    errs.append(f"{f.id}: K-major b with ldb % 8 != 0 was not refused")
                errs += _untouched(buf, f.id)
                continue
            av, bv = _place(a, f.a), _place(b if tb else b[:n], f.b)  # (tb: n == N here)
            kw = {}
            if use_a_nt:  # op(a) in N layout is what is read; a itself must not be
                kw["a_nt"] = _place(a.T.contiguous(), f.a)
                av = torch.full_like(av, float("nan"))
            ref = f.alpha * P[:, :n]
            buf, out = _out_frame(M, n, f.out)
            if f.acc:
                out.copy_(prior[:, :n])
                ref = ref + prior[:, :n].double()
            n0 = D.gemm_ring_launches()
            y = gemm_ring(av, bv, bool(ta), bool(tb), out=out, alpha=f.alpha, accumulate=f.acc, **kw)
            if y is not out:
                errs.append(f"{f.id}: gemm_ring returned {type(y).__name__}, not its output")
            if D.gemm_ring_launches() - n0 != 1:
                errs.append(f"{f.id}: {D.gemm_ring_launches() - n0} LDS-ring launches, expected 1")
            errs += _check(buf, out, ref, f.id)
    assert not errs, f"{len(errs)} failures:\n" + "\n".join(errs)


@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 1), (1, 0)])
def test_gemm_ring_refusals(ta, tb):
    """Misaligned C, ldc % 8 != 0 and K % 64 != 0 return None with nothing launched or written."""
    from collective_communication_mpi_amd.ops import gemm_ring

    M, N = 264, 136
    gen = _seed(M, N, ta, tb, 7)
    errs = []
    with _knobs() as D:
        for tag, K, c in (("misaligned C", 64, "off1"), ("odd ldc", 64, "oddld"), ("K % 64", 72, "aligned")):
            a = _ints((K, M) if ta else (M, K), 64, gen).cuda()
            b = _ints((K, N) if tb else (N, K), 64, gen).cuda()
            for dt in (F32, BF16):
                buf, out = _out_frame(M, N, dt, c)
                n0 = D.gemm_ring_launches()
                y = gemm_ring(a, b, bool(ta), bool(tb), out=out)
                if y is not None:
                    errs.append(f"{tag} {dt}: not refused")
                if D.gemm_ring_launches() != n0:
                    errs.append(f"{tag} {dt}: the ring was launched")
                errs += _untouched(buf, f"{tag} {dt}")
    assert not errs, "\n".join(errs)


# ---------------------------------------------------------------------------
# gemm_nt_swiglu: h exact, the gate bit for bit what swiglu_pairs makes of that h
# ---------------------------------------------------------------------------
SWIGLU_R = 2  # |h| stays where silu is not saturated
SWIGLU_K = (64, 128, 192)


@pytest.mark.parametrize("sched", [8, 8 | PAIR, 9 | PAIR], ids=["ring", "pair", "pairp"])
@pytest.mark.parametrize("M,N", [(257, 264), (300, 520)])
@pytest.mark.parametrize("K", SWIGLU_K)
def test_gemm_nt_swiglu_exact(sched, M, N, K):
    from collective_communication_mpi_amd.ops import gemm_nt_swiglu, swiglu_pairs

    gen = _seed(M, N, K, sched)
    a = _ints((M, K), SWIGLU_R, gen).cuda()
    b = _ints((N, K), SWIGLU_R, gen).cuda()
    P = a.double() @ b.double().T
    errs = []
    with _knobs(ring_sched=sched) as D:
        for how in ("tight", "window", "rows"):
            av, bv = _place(a, how), _place(b, how)
            hbuf, h = _out_frame(M, N, BF16)
            gbuf, glu = _out_frame(M, N // 2, BF16, col_off=4)  # 8-B aligned, ldglu > N / 2
            n0 = D.gemm_ring_launches()
            assert gemm_nt_swiglu(av, bv, h, glu), "the ring kernel's fast form should apply"
            if D.gemm_ring_launches() - n0 != 1:
                errs.append(f"{how}: {D.gemm_ring_launches() - n0} LDS-ring launches, expected 1")
            errs += _check(hbuf, h, P, f"{how} h")
            if _frame_damage(gbuf, glu):
                errs.append(f"{how} glu: {_frame_damage(gbuf, glu)} cells of the frame were overwritten")
            if bool(torch.isnan(glu.float()).any()):
                errs.append(f"{how} glu: NaN in the output")
            want = swiglu_pairs(h)  # the unfused gate on the very h the kernel wrote
            ne = glu.contiguous().view(torch.int16) != want.view(torch.int16)
            if bool(ne.any()):  # report both against an fp64 gate of the bf16 h
                hd = h.double()
                exact = hd[:, 0::2] * torch.sigmoid(hd[:, 0::2]) * hd[:, 1::2]
                e_fused = float((glu.double() - exact).abs().max())
                e_unfused = float((want.double() - exact).abs().max())
                i, j = [int(x) for x in ne.nonzero()[0]]
                errs.append(f"{how} glu: {int(ne.sum())} of {ne.numel()} values differ from swiglu_pairs(h); first at "
                            f"({i}, {j}): fused {float(glu[i, j])!r}, unfused {float(want[i, j])!r}, fp64 "
                            f"{float(exact[i, j])!r}; max error fused {e_fused:.6g}, unfused {e_unfused:.6g}")
    assert not errs, "\n".join(errs)


def test_gemm_nt_swiglu_refusals():
    """Outside the ring kernel's fast form the op returns False and launches nothing."""
    from collective_communication_mpi_amd.ops import gemm_nt_swiglu

    M, N, K = 257, 264, 64
    gen = _seed(M, N, K, 3)
    a, b = _ints((M, K), SWIGLU_R, gen).cuda(), _ints((N, K), SWIGLU_R, gen).cuda()
    errs = []
    with _knobs() as D:
        def glu_ld_mod4():  # 8-B aligned start (4 rows in, column 4), row stride % 4 == 2
            gbuf, glu = _framed(M, N // 2, BF16, SENTINEL, 4, 3, 4, 10)
            assert glu.data_ptr() % 8 == 0 and glu.stride(0) % 4 == 2
            return gbuf, glu

        def glu_short_ld():  # rows closer together than their N / 2 columns
            gbuf = torch.full((M * (N // 2),), SENTINEL, dtype=BF16, device="cuda")
            glu = torch.as_strided(gbuf, (M, N // 2), (N // 2 - 4, 1))
            assert glu.data_ptr() % 8 == 0 and glu.stride(0) % 4 == 0
            return gbuf, glu

        for tag, hc, mk in (("misaligned h", "off1", None), ("odd ldh", "oddld", None),
                            ("glu 2 B off", "aligned", lambda: _out_frame(M, N // 2, BF16, col_off=1)),
                            ("ldglu % 4", "aligned", glu_ld_mod4), ("ldglu < N / 2", "aligned", glu_short_ld)):
            hbuf, h = _out_frame(M, N, BF16, hc)
            gbuf, glu = mk() if mk else _out_frame(M, N // 2, BF16, col_off=4)
            n0 = D.gemm_ring_launches()
            if gemm_nt_swiglu(a, b, h, glu):
                errs.append(f"{tag}: not refused")
            if D.gemm_ring_launches() != n0:
                errs.append(f"{tag}: the ring was launched")
            errs += _untouched(hbuf, tag + " (h)") + _untouched(gbuf, tag + " (glu)")
    assert not errs, "\n".join(errs)


# ---------------------------------------------------------------------------
# gemm_tn: out[N1, N2] (+)= alpha * a[M, N1].T @ b[M, N2]; the reduction runs over rows
# ---------------------------------------------------------------------------
TnForm = namedtuple("TnForm", "id alpha acc c a b tail", defaults=(1.0, False, "aligned", "tight", "tight", False))
TN_FORMS = [
    TnForm("plain"),
    TnForm("half", alpha=0.5),
    TnForm("acc-half", alpha=0.5, acc=True),
    TnForm("off1", c="off1"),
    TnForm("off1-acc", acc=True, c="off1"),
    TnForm("oddld-half", alpha=0.5, c="oddld"),
    TnForm("oddld-acc", acc=True, c="oddld"),
    TnForm("windowA-rowsB", a="window", b="rows"),
    TnForm("rowsA-windowB-acc", acc=True, a="rows", b="window"),
    TnForm("windowA-windowB-half", alpha=0.5, a="window", b="window"),
    TnForm("tail", tail=True),
    TnForm("tail-acc-half-windows", alpha=0.5, acc=True, a="window", b="window", tail=True),
]
_STN = [(8, 8), (136, 72), (264, 136)]
TN_RED = (7, 128, 320, 1000)  # 1, 2, 5 and 16 K tiles of 64 rows; 7 and 1000 end inside a tile
TN_ROUTES = [(pf, sk, ws) for pf in (1, 2) for sk in (1, 3, None) for ws in (False, True)]
TN_CASES = [pytest.param(pf, sk, ws, N1, N2, M, id=f"pf{pf}-split{sk}-ws{int(ws)}-{N1}x{N2}-M{M}")
            for (pf, sk, ws) in TN_ROUTES for (N1, N2) in _STN for M in TN_RED]


def _run_tn_forms(N1, N2, M, splitk, workspace, forms, seed):
    from collective_communication_mpi_amd.ops import gemm_tn

    gen = _seed(N1, N2, M, seed)
    R = _rmax(M)
    a = _ints((M, N1), R, gen).cuda()
    b = _ints((M, N2), R, gen).cuda()
    prior = _ints((N1, N2), 64, gen).cuda().float()
    P = a.double().T @ b.double()
    errs = []
    for f in forms:
        av, bv = _place(a, f.a), _place(b, f.b)
        ref = f.alpha * P
        if not f.tail:
            if f.acc:
                ref = ref + prior.double()
            buf, out = _out_frame(N1, N2, F32, f.c)
            if f.acc:
                out.copy_(prior)
            y = gemm_tn(av, bv, out=out, alpha=f.alpha, accumulate=f.acc, splitk=splitk, workspace=workspace)
            assert y is out
            errs += _check(buf, out, ref, f.id)
            continue
        # column split: out (accumulated) takes columns < c, tail (overwritten) the rest
        c = (N2 // 2) // 4 * 4
        buf, out = _out_frame(N1, c, F32)
        tbuf, tail = _out_frame(N1, N2 - c, F32)
        left = ref[:, :c]
        if f.acc:
            out.copy_(prior[:, :c])
            left = left + prior[:, :c].double()
        gemm_tn(av, bv, out=out, alpha=f.alpha, accumulate=f.acc, splitk=splitk, workspace=workspace, tail=tail)
        errs += _check(buf, out, left, f.id + " (out)") + _check(tbuf, tail, ref[:, c:], f.id + " (tail)")
    return errs


@pytest.mark.parametrize("pf,splitk,workspace,N1,N2,M", TN_CASES)
def test_gemm_tn_route(pf, splitk, workspace, N1, N2, M):
    """The NaN rows after a framed operand are rows past the reduction; for M = 7 and 1000 they
    lie inside the last 64-row K tile, where a tail multiplied by zero (instead of zero-filled)
    would give NaN."""
    with _knobs(tn_pf=pf):
        errs = _run_tn_forms(N1, N2, M, splitk, workspace, TN_FORMS, seed=pf)
    assert not errs, f"{len(errs)} failures:\n" + "\n".join(errs)


TN_PP_SHAPE = (264, 264, 384)  # N1, N2 >= 256, M % 128 == 0: the 256x256 ping-pong TN kernel applies


@pytest.mark.parametrize("splitk", [1, 3])
def test_gemm_tn_pingpong_variant(splitk):
    N1, N2, M = TN_PP_SHAPE
    with _knobs(tn_variant=1):
        errs = _run_tn_forms(N1, N2, M, splitk, None, TN_FORMS, seed=11)
    assert not errs, f"{len(errs)} failures:\n" + "\n".join(errs)


def test_gemm_tn_refusals():
    from collective_communication_mpi_amd.ops import gemm_tn

    M, N2 = 128, 72
    gen = _seed(M, N2, 5)
    b = _ints((M, N2), 64, gen).cuda()
    errs = []
    # N1 % 8 != 0
    a12 = _place(_ints((M, 12), 64, gen).cuda(), "rows")  # 12 columns of 24: only N1 breaks a rule
    assert a12.data_ptr() % 16 == 0 and a12.stride(0) % 8 == 0
    buf, out = _out_frame(12, N2, F32)
    with pytest.raises(ValueError):
        gemm_tn(a12, b, out=out)
    errs += _untouched(buf, "N1 % 8")
    # the column split: a tail, or an out, that the split-K reduction cannot write as 16-B vectors
    a = _ints((M, 8), 64, gen).cuda()
    c = 36
    for tag, oc, tc in (("misaligned tail", "aligned", "off1"), ("odd tail stride", "aligned", "oddld"),
                        ("misaligned out with a tail", "off1", "aligned"), ("odd out stride with a tail", "oddld", "aligned")):
        buf, out = _out_frame(8, c, F32, oc)
        tbuf, tail = _out_frame(8, N2 - c, F32, tc)
        with pytest.raises(ValueError):
            gemm_tn(a, b, out=out, tail=tail, splitk=2)
        errs += _untouched(buf, tag + " (out)") + _untouched(tbuf, tag + " (tail)")
    assert not errs, "\n".join(errs)


# every (K, R) of this module, for the CPU recipe test
RECIPE_KR = sorted({(K, _rmax(K)) for (_, _, _, ks) in NT_ROUTES.values() for K in ks}
                   | {(K, _rmax(K)) for K in RING_K} | {(M, _rmax(M)) for M in TN_RED}
                   | {(TN_PP_SHAPE[2], _rmax(TN_PP_SHAPE[2]))} | {(K, SWIGLU_R) for K in SWIGLU_K})
