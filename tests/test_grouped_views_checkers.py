"""The checkers of tests/test_gpu_grouped_views.py, run without a GPU.

First against plain-torch emulations of the four grouped ops: a per-expert loop in fp64,
rounded once, that writes only the experts' rows.  Every form must pass, which checks the
references, the frames and the layouts of the GPU module.  Then against mutants of those
emulations, each a way a kernel can be subtly wrong; every one must be reported, with a
message that names the form.  The refusal table runs against the wrappers' validators, which
need no GPU.
"""
import pytest
import torch

import test_gpu_grouped_views as gv
from test_gpu_grouped_views import BF16, F32, LAYOUTS, _bounds

from collective_communication_mpi_amd import ops

CPU = "cpu"


def _trunc_bf16(t32):
    return (t32.view(torch.int32) & ~0xFFFF).view(F32).to(BF16)


class Emu:
    """The four ops in torch; ``mut`` names the one way in which this instance is wrong."""

    def __init__(self, mut=None):
        self.mut = mut

    # -- rows ---------------------------------------------------------------
    def bounds(self, counts, cap):
        cs = [int(c) for c in counts.tolist()]
        if self.mut == "abs":
            cs = [abs(c) for c in cs]
        b = _bounds(cs, cap)
        if self.mut == "boundary":  # every inner boundary one row early
            total = b[-1][1]
            shift = lambda r: r - 1 if 0 < r < total else r  # noqa: E731
            b = [(shift(a), shift(e)) for a, e in b]
        return b

    def cast(self, y64, dtype):
        y = (y64 + 0.0).to(F32)  # an accumulator starts at +0: a sum of zeros is never -0
        if dtype == BF16:
            return _trunc_bf16(y) if self.mut == "trunc" else y.to(BF16)
        return y

    def spoil(self, out, counts, cap):
        """The mutants that write where nothing may be written (a framed output has the room)."""
        total = _bounds([int(c) for c in counts.tolist()], cap)[-1][1]
        if self.mut == "rowtotal" and total < cap:
            out[total] = 0
        room = out.untyped_storage().nbytes() // out.element_size() - out.storage_offset()
        if self.mut == "frame" and room > out.shape[1]:
            torch.as_strided(out, (1, 1), (1, 1), out.storage_offset() + out.shape[1]).zero_()
        if self.mut == "noclamp" and any(int(c) > cap for c in counts.tolist()):
            # the rows past cap: what was read there is not the operand, what is written is the frame
            if room >= (cap + 2) * out.stride(0):
                torch.as_strided(out, (2, out.shape[1]), out.stride(), out.storage_offset() + cap * out.stride(0)).fill_(
                    float("nan"))

    def weights(self, w):
        if self.mut == "tightw" and not w.is_contiguous():
            G, N, K = w.shape
            return torch.as_strided(w, (G, N, K), (N * K, K, 1), w.storage_offset())
        return w

    # -- ops ----------------------------------------------------------------
    def nt(self, x, w, counts, out=None, bias=None, alpha=1.0, out_dtype=BF16):
        cap, K = x.shape
        G, N = w.shape[0], w.shape[1]
        if out is None:
            out = torch.empty((cap, N), dtype=out_dtype)
        w = self.weights(w)
        kk = K - 1 if self.mut == "dropk" else K
        for g, (a, b) in enumerate(self.bounds(counts, cap)):
            if b > a:
                y = alpha * (x[a:b, :kk].double() @ w[g, :, :kk].double().T)
                if bias is not None:
                    y = y + bias[g].double()
                out[a:b] = self.cast(y, out.dtype)
        self.spoil(out, counts, cap)
        return out

    @staticmethod
    def gate(h):
        h = h.float()
        return (h[:, 0::2] * torch.sigmoid(h[:, 0::2]) * h[:, 1::2]).to(BF16)

    def swiglu(self, x, w, counts, h=None, glu=None, bias=None, alpha=1.0):
        cap = x.shape[0]
        h = self.nt(x, w, counts, out=h, bias=bias, alpha=alpha)
        if glu is None:
            glu = torch.empty((cap, h.shape[1] // 2), dtype=BF16)
        for a, b in self.bounds(counts, cap):
            if b > a:
                hh = h[a:b]
                if self.mut == "gluswap":
                    hh = torch.stack((hh[:, 1::2], hh[:, 0::2]), dim=2).reshape(hh.shape)
                glu[a:b] = self.gate(hh)
        return h, glu

    def nn(self, dy, w, counts, out=None, alpha=1.0, out_dtype=BF16):
        cap, N = dy.shape
        K = w.shape[2]
        if out is None:
            out = torch.empty((cap, K), dtype=out_dtype)
        w = self.weights(w)
        nn = N - 1 if self.mut == "dropk" else N
        for g, (a, b) in enumerate(self.bounds(counts, cap)):
            if b > a:
                out[a:b] = self.cast(alpha * (dy[a:b, :nn].double() @ w[g, :nn].double()), out.dtype)
        self.spoil(out, counts, cap)
        return out

    def tn(self, dy, x, counts, out=None, alpha=1.0):
        cap, N = dy.shape
        K = x.shape[1]
        G = counts.numel()
        if out is None:
            out = torch.full((G, N, K), float("nan"), dtype=F32)  # "uninitialised", reproducibly
        for g, (a, b) in enumerate(self.bounds(counts, cap)):
            if b == a and self.mut == "emptydw":
                continue
            if b > a and self.mut == "nextrow":
                b = min(b + 1, cap)
            if b > a and self.mut == "dropk":
                b -= 1
            out[g] = self.cast(alpha * (dy[a:b].double().T @ x[a:b].double()), F32)
            if self.mut == "noclamp" and int(counts[g]) > cap:
                out[g] = float("nan")  # the reduction ran on into what lies behind the operands
        if self.mut == "frame" and out.storage_offset():
            torch.as_strided(out, (1,), (1,), out.storage_offset() - 1).zero_()
        return out

    @staticmethod
    def transposed(w):
        G, N, K = w.shape
        return w.contiguous().view(G * N, K).t().contiguous().view(K, G, N).permute(1, 0, 2)

    def linear(self, x, w, counts):
        emu = self

        class Fn(torch.autograd.Function):
            @staticmethod
            def forward(ctx, x, w, counts):
                wb = w.to(BF16)
                ctx.save_for_backward(x, wb, counts)
                ctx.w_dtype = w.dtype
                return emu.nt(x, wb, counts)

            @staticmethod
            def backward(ctx, dy):
                x, wb, counts = ctx.saved_tensors
                return emu.nn(dy, wb, counts), emu.tn(dy, x, counts).to(ctx.w_dtype), None

        return Fn.apply(x, w, counts)


def _param_values(cases):
    return [c.values for c in cases]


def _named(errs, forms):
    return bool(errs) and all(any(e.startswith(f.id) for f in forms) for e in errs)


# ---------------------------------------------------------------------------
# the emulations pass every form
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("layout,N,K", _param_values(gv.NT_CASES))
def test_emulated_nt_passes(layout, N, K):
    gv._fail(gv._run_nt_forms(Emu().nt, layout, N, K, gv.NT_FORMS, CPU))


@pytest.mark.parametrize("layout,N,K", _param_values(gv.GLU_CASES))
def test_emulated_swiglu_passes(layout, N, K):
    e = Emu()
    gv._fail(gv._run_swiglu_forms(e.swiglu, e.gate, layout, N, K, gv.GLU_FORMS, CPU))


@pytest.mark.parametrize("layout,N,K", _param_values(gv.NN_CASES))
def test_emulated_nn_passes(layout, N, K):
    e = Emu()
    gv._fail(gv._run_nn_forms(e.nn, e.nt, e.transposed, layout, N, K, gv.NN_FORMS, CPU))


@pytest.mark.parametrize("layout,N,K", _param_values(gv.TN_CASES))
def test_emulated_tn_passes(layout, N, K):
    gv._fail(gv._run_tn_forms(Emu().tn, layout, N, K, gv.TN_FORMS, CPU))


@pytest.mark.parametrize("w_dtype", [BF16, F32], ids=["wbf16", "wf32"])
@pytest.mark.parametrize("N,K", gv.LINEAR_SHAPES)
def test_emulated_linear_passes(N, K, w_dtype):
    gv._fail(gv._run_linear(Emu().linear, N, K, w_dtype, CPU))


# ---------------------------------------------------------------------------
# every mutant is reported
# ---------------------------------------------------------------------------
def _nt(mut, layout, N=72, K=72):
    return gv._run_nt_forms(Emu(mut).nt, layout, N, K, gv.NT_FORMS, CPU), gv.NT_FORMS


def _nn(mut, layout, N=72, K=72):
    e = Emu(mut)
    return gv._run_nn_forms(e.nn, e.nt, e.transposed, layout, N, K, gv.NN_FORMS, CPU), gv.NN_FORMS


def _tn(mut, layout, N=136, K=72):
    return gv._run_tn_forms(Emu(mut).tn, layout, N, K, gv.TN_FORMS, CPU), gv.TN_FORMS


def _glu(mut, layout="mixed", N=136, K=72):
    e = Emu(mut)
    return gv._run_swiglu_forms(e.swiglu, Emu.gate, layout, N, K, gv.GLU_FORMS, CPU), gv.GLU_FORMS


# mutant -> the checker runs that must each report it
MUTANTS = {
    "boundary": [lambda m: _nt(m, "mixed"), lambda m: _nn(m, "mixed"), lambda m: _tn(m, "mixed"), lambda m: _glu(m),
                 lambda m: _nt(m, "limit", 8, 128), lambda m: _tn(m, "long")],
    "abs": [lambda m: _nt(m, "mixed"), lambda m: _nn(m, "mixed"), lambda m: _tn(m, "mixed"), lambda m: _glu(m)],
    "noclamp": [lambda m: _nt(m, "huge"), lambda m: _nn(m, "huge"), lambda m: _tn(m, "huge")],
    "trunc": [lambda m: _nt(m, "one"), lambda m: _nn(m, "one"), lambda m: _nt(m, "mixed", 264, 256)],
    "dropk": [lambda m: _nt(m, "one"), lambda m: _nn(m, "overflow"), lambda m: _tn(m, "long"), lambda m: _glu(m),
              lambda m: _nt(m, "mixed", 8, 8)],
    "nextrow": [lambda m: _tn(m, "mixed"), lambda m: _tn(m, "long"), lambda m: _tn(m, "limit", 8, 8)],
    "rowtotal": [lambda m: _nt(m, "mixed"), lambda m: _nn(m, "mixed"), lambda m: _glu(m), lambda m: _nt(m, "limit")],
    "frame": [lambda m: _nt(m, "one"), lambda m: _nn(m, "overflow"), lambda m: _tn(m, "mixed"), lambda m: _glu(m)],
    "tightw": [lambda m: _nt(m, "mixed"), lambda m: _nn(m, "one"), lambda m: _glu(m)],
    "gluswap": [lambda m: _glu(m), lambda m: _glu(m, "overflow", 264, 64)],
    "emptydw": [lambda m: _tn(m, "mixed"), lambda m: _tn(m, "overflow"), lambda m: _tn(m, "limit", 8, 8)],
}


@pytest.mark.parametrize("mut", list(MUTANTS))
def test_mutant_is_reported(mut):
    for i, run in enumerate(MUTANTS[mut]):
        errs, forms = run(mut)
        assert errs, f"{mut}: run {i} reported nothing"
        assert _named(errs, forms), f"{mut}: run {i} has a message that names no form:\n" + "\n".join(errs)


def test_mutants_hit_the_forms_they_should():
    """The mutants that depend on a form's placement or dtype are reported for exactly those."""
    errs, _ = _nt("tightw", "mixed")
    assert {e.split(":")[0] for e in errs} == {f.id for f in gv.NT_FORMS if f.w == "padded"}
    errs, _ = _nt("trunc", "one")
    assert {e.split(":")[0] for e in errs} == {f.id for f in gv.NT_FORMS if f.out == BF16}
    errs, _ = _tn("frame", "mixed")
    assert {e.split(":")[0] for e in errs} == {f.id for f in gv.TN_FORMS if f.c == "window"}
    errs, _ = _nt("dropk", "one")
    assert {e.split(":")[0] for e in errs} == {f.id for f in gv.NT_FORMS}


def test_linear_checker_reports_mutants():
    for mut, tags in (("trunc", {"y", "x.grad"}), ("abs", {"y", "x.grad", "w.grad"}), ("nextrow", {"w.grad"}),
                      ("emptydw", {"w.grad"})):
        errs = gv._run_linear(Emu(mut).linear, 72, 72, BF16, CPU)
        assert {e.split(":")[0] for e in errs} == tags, (mut, errs)


# ---------------------------------------------------------------------------
# the layouts are what the table says, and _bounds walks the rows of the kernels' tile map
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_bounds_cover_the_tile_map(name):
    counts, cap = LAYOUTS[name]
    rows = {g: [] for g in range(len(counts))}
    for g, r0, n in ops.grouped_tile_map(counts, cap):
        assert 1 <= n <= 128
        rows[g] += range(r0, r0 + n)
    for g, (a, b) in enumerate(_bounds(counts, cap)):
        assert rows[g] == list(range(a, b)), (name, g)
    assert _bounds(counts, cap)[-1][1] == min(sum(max(c, 0) for c in counts), cap)


def test_layouts_hit_what_they_claim():
    b = {k: _bounds(*v) for k, v in LAYOUTS.items()}
    assert b["one"] == [(0, 130)] and LAYOUTS["one"][1] == 130                       # two tiles, no spare row
    counts, cap = LAYOUTS["mixed"]
    assert counts[0] == 0 and min(counts) < 0 and cap == 392 + 43
    assert [a for a, _ in b["mixed"]] == [0, 0, 1, 128, 128, 257, 385] and b["mixed"][-1][1] == 392
    assert {e - a for a, e in b["mixed"]} >= {0, 1, 127, 128, 129}                   # tile - 1 / exact / + 1
    assert any(a % 8 for a, e in b["mixed"] if e > a)                                # offsets off the 8-row grid
    assert b["overflow"] == [(0, 100), (100, 200), (200, 250), (250, 250)] and LAYOUTS["overflow"][1] == 250
    assert b["huge"] == [(0, 70)] and LAYOUTS["huge"][0][0] > LAYOUTS["huge"][1]
    counts, cap = LAYOUTS["limit"]
    assert len(counts) == ops.kernels.GROUPED_MAX_EXPERTS == 256 and cap == sum(counts) + 3
    assert counts[:8] == [0, 1, 1, 1, 1, 1, 1, 0]
    assert [-(-(e - a) // 64) for a, e in b["long"]] == [5, 4, 1] and b["long"][-1][1] == LAYOUTS["long"][1]
    # 0 to 5 reduction tiles of 64 rows for the two-in-flight TN loop
    tiles = {-(-(e - a) // 64) for lay in gv.TN_LAYOUTS for a, e in b[lay]}
    assert tiles >= {0, 1, 2, 3, 4, 5}
    # the K lists: 1, 2, an odd and an even count of 64-deep steps; the register loop always has a tail
    assert [k // 64 for k in gv.K_GLDS] == [1, 2, 3, 4] and all(k % 64 == 0 for k in gv.K_GLDS)
    assert [-(-k // 64) for k in gv.K_REGS] == [1, 2, 3, 4] and all(k % 64 and k % 8 == 0 for k in gv.K_REGS)


def test_weight_placements():
    w = gv._ints((3, 16, 24), 64, gv._seed(1))
    p = gv._place_w(w, "padded")
    assert torch.equal(p, w) and p.stride() == ((16 + 8) * (24 + 16), 24 + 16, 1) and p.storage_offset() == 8
    flat = torch.as_strided(p, (3 * 24 * 40,), (1,), 0).view(3, 24, 40)
    assert bool(torch.isnan(flat[:, 16:].float()).all()) and bool(torch.isnan(flat[:, :, :8].float()).all())
    t = gv._place_w(w, "tail")
    assert torch.equal(t, w) and t.is_contiguous() and (t.storage_offset() * 2) % 16 == 0
    behind = torch.as_strided(t, (64, 24), (24, 1), t.storage_offset() + w.numel())
    assert bool(torch.isnan(behind.float()).all())
    buf, o = gv._dw_frame(3, 16, 24, "window", CPU)
    assert o.shape == (3, 16, 24) and o.stride() == (18 * 36, 36, 1) and (o.storage_offset() * 4) % 16 == 0


# ---------------------------------------------------------------------------
# refusals: the wrappers' validators, which run before anything reaches the GPU
# ---------------------------------------------------------------------------
def test_refusals_by_the_validators():
    table = gv._refusals(CPU)
    want = {"nt": 7, "swiglu": 8, "nn": 7, "tn": 8}
    assert {op: sum(r.op == op for r in table) for op in want} == want
    gv._fail(gv._run_refusals({"nt": ops.grouped_validate, "swiglu": ops.grouped_swiglu_validate,
                               "nn": ops.grouped_nn_validate, "tn": ops.grouped_tn_validate}, CPU))


def test_refusal_checker_reports_an_op_that_accepts_or_writes():
    def accepts(*a, **kw):
        return None

    def writes(*a, **kw):
        for k in ("out", "h"):
            if k in kw:
                kw[k][0, ..., 0] = 1.0
        raise ValueError("too late")

    n = len(gv._refusals(CPU))
    assert len(gv._run_refusals(dict.fromkeys(("nt", "swiglu", "nn", "tn"), accepts), CPU)) == n
    errs = gv._run_refusals(dict.fromkeys(("nt", "swiglu", "nn", "tn"), writes), CPU)
    assert sum("wrote" in e for e in errs) == n
