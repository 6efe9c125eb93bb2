"""The fused AdamW kernels (csrc/device/optim.hip) and ``parallel.AdamW`` on the GPU.

Every parameter, state and workspace view lies inside a sentinel-filled frame.  The update is
compared bit for bit with ``ops.adamw_reference(dtype=float32)`` computed on the CPU (IEEE: every
operation rounded once); the norm with ``ops.grad_norm_reference`` (fp64) within 2^-16.
"""
import copy

import pytest
import torch

from collective_communication_mpi_amd import _native, ops, parallel

pytestmark = pytest.mark.gpu

BF16, F32, F64, I64, I32 = torch.bfloat16, torch.float32, torch.float64, torch.int64, torch.int32
CHUNK = ops.OPTIM_CHUNK
SENTINEL = -7.0
PAD = 16  # elements of frame in front of and behind every view
BETAS, EPS, LR, WD = (0.9, 0.999), 1e-8, 1e-3, 0.1

# (size, decays, sharded, parameter base misaligned).  Between them: sizes 1, 7, 8, 2048, 2049 and
# 4104; an offset that is no multiple of 8 (after the 7: scalar accesses from there on); S = 1;
# a spare slot ("spare": 4105 elements in 4 segments are 6 slots, 5 of them used); a parameter
# whose own base is not 16-byte aligned under an aligned offset.
LAYOUTS = {
    "mixed": [(8, True, False, False), (2048, False, True, False), (4104, True, True, False), (2049, True, False, True),
              (7, False, False, False), (1, True, True, False), (2049, True, False, False)],
    "single": [(4104, True, False, False)],
    "spare": [(2049, True, True, False), (1, False, False, False), (7, True, False, False), (2048, False, True, False)],
}


def _framed(n, dtype, fill=None, shift=0):
    """(frame, view): ``n`` elements inside a sentinel frame; the view is 16-byte aligned unless shifted."""
    frame = torch.full((n + 2 * PAD + 1,), SENTINEL, dtype=dtype, device="cuda")
    view = frame[PAD + shift:PAD + shift + n]
    if fill is not None:
        view.copy_(fill)
    return frame, view


def _intact(frame, view):
    lo = (view.data_ptr() - frame.data_ptr()) // frame.element_size()
    return bool((frame[:lo] == SENTINEL).all() and (frame[lo + view.numel():] == SENTINEL).all())


def _randn(n, seed, dtype, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, generator=g) * scale).to(dtype)


class Bucket:
    def __init__(self, layout, dtype, seed=0, nb=1):
        segs = LAYOUTS[layout]
        self.dtype, self.sizes = dtype, [s[0] for s in segs]
        self.off = [0]
        for s in self.sizes:
            self.off.append(self.off[-1] + s)
        self.n, self.S = self.off[-1], len(segs)
        self.flags = [(ops.OPTIM_DECAY if d else 0) | (ops.OPTIM_SHARDED if sh else 0) for _, d, sh, _ in segs]
        self.frames = {}
        self.params = []
        for i, (size, _, _, mis) in enumerate(segs):
            f, v = _framed(size, dtype, _randn(size, seed + 10 + i, dtype), shift=1 if mis else 0)
            assert (v.data_ptr() % 16 != 0) == mis
            self.frames[f"param {i}"] = (f, v)
            self.params.append(v)
        self.p0 = torch.cat([p.float().cpu() for p in self.params])
        for name, dt, fill in (("g", dtype, None), ("m", F32, 0.0), ("v", F32, 0.0), ("p32", F32, self.p0)):
            if name == "p32" and dtype == F32:
                self.p32 = None
                continue
            f, v = _framed(self.n, dt)
            if fill is not None:
                v.copy_(fill if isinstance(fill, torch.Tensor) else torch.full((self.n,), fill))
            self.frames[name] = (f, v)
            setattr(self, name, v)
        f, self.partials = _framed(ops.optim_slots(self.n, self.S), F32)
        self.frames["partials"] = (f, self.partials)
        f, v = _framed(2 * nb, F64)
        self.sums = v.view(2, nb)
        self.frames["sums"] = (f, v)
        f, self.clip = _framed(2, F32)
        self.frames["clip"] = (f, self.clip)
        self.seg_off = torch.tensor(self.off, dtype=I64, device="cuda")
        self.seg_ptr = torch.tensor([p.data_ptr() for p in self.params], dtype=I64, device="cuda")
        self.seg_flags = torch.tensor(self.flags, dtype=I32, device="cuda")
        self.sched = torch.zeros(4, dtype=F32, device="cuda")
        self.decays = torch.cat([torch.full((s,), bool(f & 1)) for s, f in zip(self.sizes, self.flags)])

    def set_grad(self, seed, scale=1.0):
        self.g.copy_(_randn(self.n, seed, self.dtype, scale))
        return self.g.cpu()

    def update(self, t, clip=None, max_grid=0):
        self.sched.copy_(ops.optim_sched(LR, BETAS, WD, t))
        ops.optim_adamw_update(self.g, self.seg_off, self.seg_ptr, self.seg_flags, self.p32, self.m, self.v, self.sched,
                               clip, BETAS, EPS, max_grid=max_grid)

    def norm(self, bucket=0, max_grid=0):
        ops.optim_sqsum(self.g, self.seg_off, self.seg_flags, self.partials, self.sums, bucket, max_grid=max_grid)

    def param_values(self):
        return torch.cat([p.cpu() for p in self.params])

    def masters(self):
        return self.param_values() if self.p32 is None else self.p32.cpu()

    def assert_frames(self):
        torch.cuda.synchronize()
        for name, (f, v) in self.frames.items():
            assert _intact(f, v), f"the frame around {name} was written"


def _bits(t):
    return t.view(torch.int32 if t.dtype == F32 else torch.int16)


def _same(name, got, want):
    assert got.dtype == want.dtype and torch.equal(_bits(got), _bits(want)), \
        f"{name}: {int((_bits(got) != _bits(want)).sum())} of {got.numel()} elements differ from the fp32 mirror"


@pytest.mark.parametrize("dtype", (BF16, F32), ids=("bf16", "fp32"))
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("clipped", (False, True), ids=("no clip", "clip"))
def test_update_is_the_fp32_mirror_bitwise(layout, dtype, clipped):
    b = Bucket(layout, dtype)
    p, m, v = b.p0.clone(), torch.zeros(b.n), torch.zeros(b.n)
    coef = None
    for t in (1, 2, 3):
        g = b.set_grad(40 + t, scale=3.0)
        if clipped:
            b.norm()
            ops.optim_clip(b.sums, 0.5 + t, b.clip)  # the norm is far above: a coef below 1
            coef = b.clip.cpu()[1]
            assert 0.0 < coef.item() < 1.0
        b.update(t, b.clip if clipped else None)
        p, m, v = ops.adamw_reference(g, p, m, v, ops.optim_sched(LR, BETAS, WD, t), coef, BETAS, EPS, b.decays)
        assert bool(((m == 0) | (m.abs() >= 2.0 ** -100)).all() and ((v == 0) | (v.abs() >= 2.0 ** -100)).all())
        torch.cuda.synchronize()
        _same(f"step {t} m", b.m.cpu(), m)
        _same(f"step {t} v", b.v.cpu(), v)
        _same(f"step {t} master", b.masters(), p)
        _same(f"step {t} parameters", b.param_values(), p.to(dtype))
        assert torch.equal(_bits(b.g.cpu()), _bits(g)), "the gradients were written"
    assert not torch.equal(p, b.p0)
    b.assert_frames()


@pytest.mark.parametrize("dtype", (BF16, F32), ids=("bf16", "fp32"))
def test_walking_several_slots_per_workgroup_changes_no_bit(dtype):
    a, b = Bucket("mixed", dtype), Bucket("mixed", dtype)
    for x, grid in ((a, 0), (b, 2)):
        x.set_grad(5)
        x.norm(max_grid=grid)
        ops.optim_clip(x.sums, 1.0, x.clip)
        x.update(1, x.clip, max_grid=grid)
    torch.cuda.synchronize()
    for name in ("partials", "sums", "clip", "m", "v"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert torch.equal(a.masters(), b.masters()) and torch.equal(a.param_values(), b.param_values())
    b.assert_frames()


@pytest.mark.parametrize("dtype", (BF16, F32), ids=("bf16", "fp32"))
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_norm(layout, dtype):
    nb = 3
    b = Bucket(layout, dtype, nb=nb)
    tol = 2.0 ** -16
    exact = []
    for k, scale in enumerate((1.0, 1e-3, 30.0)):  # three "buckets": the same table, other gradients
        g = b.set_grad(70 + k, scale)
        b.norm(bucket=k)
        parts = [g[lo:hi] for lo, hi in zip(b.off, b.off[1:])]
        _, sh, rep = ops.grad_norm_reference(parts, [bool(f & ops.OPTIM_SHARDED) for f in b.flags])
        exact.append((sh, rep))
        got = b.sums.cpu()[:, k]
        for what, x, e in (("sharded", got[0].item(), sh), ("replicated", got[1].item(), rep)):
            ratio = abs(x ** 0.5 - e ** 0.5) / (tol * e ** 0.5) if e else float(x != 0.0)
            print(f"[optim norm] {layout} {dtype} bucket {k} {what}: {ratio:.4f} of the bound")
            assert ratio <= 1.0
    spare = [i for i, e in enumerate(ops.optim_tile_map(b.off)) if e is None]
    if layout == "spare":
        assert spare
    assert (b.partials[spare] == 0).all(), "a spare slot's partial is not zero"
    max_norm = 2.5
    ops.optim_clip(b.sums, max_norm, b.clip)
    first = (b.partials.clone(), b.sums.clone(), b.clip.clone())
    norm, coef = b.clip.cpu()
    total = sum(sh for sh, _ in exact) + sum(rep for _, rep in exact)
    ratio = abs(norm.item() - total ** 0.5) / (tol * total ** 0.5)
    print(f"[optim norm] {layout} {dtype} norm: {ratio:.4f} of the bound")
    assert ratio <= 1.0
    want = torch.clamp(torch.tensor(max_norm, dtype=F32) / (norm + torch.tensor(1e-6, dtype=F32)), max=1.0)
    assert torch.equal(_bits(coef.reshape(1)), _bits(want.reshape(1))), (coef.item(), want.item())
    # again: the same bits
    b.norm(bucket=2)
    ops.optim_clip(b.sums, max_norm, b.clip)
    torch.cuda.synchronize()
    for x, y in zip(first, (b.partials, b.sums, b.clip)):
        assert torch.equal(x, y)
    b.assert_frames()


def test_norm_of_zeros():
    b = Bucket("mixed", BF16)
    b.g.zero_()
    b.norm()
    ops.optim_clip(b.sums, 1.0, b.clip)
    assert b.sums.cpu().tolist() == [[0.0], [0.0]] and b.clip.cpu().tolist() == [0.0, 1.0]
    b.assert_frames()


def test_refused_calls_write_nothing():
    b = Bucket("mixed", BF16)
    b.set_grad(3)
    before = {name: v.clone() for name, (_, v) in b.frames.items()}
    upd = lambda **kw: ops.optim_adamw_update(**{**dict(g=b.g, seg_off=b.seg_off, seg_ptr=b.seg_ptr, seg_flags=b.seg_flags,
                                                     p32=b.p32, m=b.m, v=b.v, sched=b.sched, clip=b.clip), **kw})
    sq = lambda **kw: ops.optim_sqsum(**{**dict(g=b.g, seg_off=b.seg_off, seg_flags=b.seg_flags, partials=b.partials,
                                               sums=b.sums), **kw})
    off = torch.full((b.n + 8,), SENTINEL, dtype=F32, device="cuda")
    refused = [
        (TypeError, lambda: upd(g=b.g.half())),
        (TypeError, lambda: upd(m=b.m.double())),
        (TypeError, lambda: upd(seg_off=b.seg_off.int())),
        (TypeError, lambda: upd(sched=b.sched.double())),
        (TypeError, lambda: sq(sums=b.sums.float())),
        (TypeError, lambda: ops.optim_clip(b.sums, 1.0, b.clip.double())),
        (ValueError, lambda: upd(p32=None)),
        (ValueError, lambda: upd(m=b.m[:-1])),
        (ValueError, lambda: upd(v=off[1:1 + b.n])),
        (ValueError, lambda: upd(seg_off=b.seg_off.cpu())),
        (ValueError, lambda: upd(seg_ptr=b.seg_ptr[:-1])),
        (ValueError, lambda: upd(clip=b.clip[:1])),
        (ValueError, lambda: upd(betas=(0.9, 1.0))),
        (ValueError, lambda: upd(eps=-1.0)),
        (ValueError, lambda: upd(max_grid=5000)),
        (ValueError, lambda: sq(partials=b.partials[:-1])),
        (ValueError, lambda: sq(bucket=1)),
        (ValueError, lambda: sq(seg_flags=None)),
        (ValueError, lambda: ops.optim_clip(b.sums, 0.0, b.clip)),
        (ValueError, lambda: ops.optim_clip(b.sums.cpu(), 1.0, b.clip)),
    ]
    for error, call in refused:
        with pytest.raises(error, match="optim"):
            call()
    # the extension's own refusals, all on the host, before any launch
    dev = _native.device()
    st = torch.cuda.current_stream().cuda_stream

    def raw_update(**kw):
        a = dict(g=b.g.data_ptr(), f32=False, seg_off=b.seg_off.data_ptr(), seg_ptr=b.seg_ptr.data_ptr(),
                 seg_flags=b.seg_flags.data_ptr(), S=b.S, n=b.n, p32=b.p32.data_ptr(), m=b.m.data_ptr(), v=b.v.data_ptr(),
                 clip=b.clip.data_ptr(), sched=b.sched.data_ptr(), b1=0.9, b2=0.999, eps=1e-8, max_grid=0, stream=st)
        a.update(kw)
        dev.optim_adamw(**a)

    def raw_sqsum(**kw):
        a = dict(g=b.g.data_ptr(), f32=False, seg_off=b.seg_off.data_ptr(), seg_flags=b.seg_flags.data_ptr(), S=b.S, n=b.n,
                 partials=b.partials.data_ptr(), out_sharded=b.sums.data_ptr(), out_replicated=b.sums.data_ptr() + 8,
                 max_grid=0, stream=st)
        a.update(kw)
        dev.optim_sqsum(**a)

    for kw in (dict(n=0), dict(S=0), dict(S=b.n + 1), dict(n=(1 << 40) + 1), dict(g=0), dict(g=b.g.data_ptr() + 2),
               dict(seg_off=0), dict(seg_ptr=0), dict(seg_flags=0), dict(p32=0), dict(p32=b.p32.data_ptr() + 4),
               dict(f32=True), dict(m=0), dict(v=b.v.data_ptr() + 8), dict(sched=0), dict(clip=b.clip.data_ptr() + 2),
               dict(b1=1.0), dict(b2=-0.5), dict(eps=-1.0), dict(eps=float("inf")), dict(max_grid=-1), dict(max_grid=4097)):
        with pytest.raises(ValueError, match="optim"):
            raw_update(**kw)
    for kw in (dict(n=0), dict(S=0), dict(g=0), dict(seg_flags=0), dict(partials=0), dict(partials=b.partials.data_ptr() + 2),
               dict(out_sharded=0), dict(out_replicated=b.sums.data_ptr() + 4), dict(max_grid=4097)):
        with pytest.raises(ValueError, match="optim"):
            raw_sqsum(**kw)
    for kw in (dict(nb=0), dict(max_norm=0.0), dict(max_norm=float("nan")), dict(clip=0), dict(sharded=0)):
        a = dict(sharded=b.sums.data_ptr(), replicated=b.sums.data_ptr() + 8, nb=1, max_norm=1.0, clip=b.clip.data_ptr(),
                 stream=st)
        a.update(kw)
        with pytest.raises(ValueError, match="optim"):
            dev.optim_clip(**a)
    torch.cuda.synchronize()
    for name, (_, v) in b.frames.items():
        assert torch.equal(v, before[name]), f"a refused call wrote {name}"
    assert (off == SENTINEL).all()
    b.assert_frames()


# --- parallel.AdamW ------------------------------------------------------------------------------------------


def _comm():
    from collective_communication_mpi_amd import MPI, Communicator

    return Communicator(MPI.COMM_WORLD)  # one rank


class Params(torch.nn.Module):
    """bf16 parameters of the layouts' sizes and one fp32 "router": several buckets, two dtypes."""

    def __init__(self):
        super().__init__()
        shapes = [(2049,), (8, 513), (7,), (1,), (4, 512), (8,)]
        self.ws = torch.nn.ParameterList(
            [torch.nn.Parameter(_randn(torch.Size(s).numel(), 200 + i, BF16).view(s).cuda()) for i, s in enumerate(shapes)])
        self.router = torch.nn.Parameter(_randn(4 * 33, 300, F32).view(4, 33).cuda())


def _set_grads(ddp, step):
    for i, q in enumerate(ddp.module.parameters()):
        q.grad.copy_(_randn(q.numel(), 1000 * step + i, q.dtype, 2.0).view_as(q))


def _optimizer(bucket_bytes=6000, **kw):
    ddp = parallel.DistributedDataParallel(Params(), _comm(), bucket_bytes=bucket_bytes)
    return ddp, parallel.AdamW(ddp, LR, BETAS, EPS, WD, **{"max_grad_norm": 1.0, **kw})


def test_adamw_class_against_the_mirror_and_its_table():
    ddp, opt = _optimizer()
    assert len(opt.states) >= 3 and {s.buf.dtype for s in opt.states} == {BF16, F32}
    names = dict(ddp.module.named_parameters())
    start = {n: q.detach().clone() for n, q in names.items()}
    ref = {n: (q.detach().float().cpu(), torch.zeros(q.shape), torch.zeros(q.shape)) for n, q in names.items()}
    for step in (1, 2, 3):
        _set_grads(ddp, step)
        if step == 2:  # a parameter moves: the table follows
            q = names["ws.2"]
            q.data = q.data.clone()
        opt.step()
        norm, coef = opt.clip.cpu()
        exact, _, _ = ops.grad_norm_reference([q.grad for q in names.values()])
        assert abs(norm.item() - exact) <= 2.0 ** -16 * exact and coef.item() < 1.0
        assert torch.equal(opt.grad_norm.cpu(), norm.reshape(1))
        for n, q in names.items():
            ref[n] = ops.adamw_reference(q.grad.cpu(), *ref[n], ops.optim_sched(LR, BETAS, WD, step), coef, BETAS, EPS,
                                         q.ndim >= 2)
    sd = opt.state_dict()
    assert sd["step"] == 3 and set(sd["state"]) == set(names)
    for n, q in names.items():
        p, m, v = ref[n]
        e = sd["state"][n]
        _same(f"{n} master", e["master"].cpu(), p)
        _same(f"{n} exp_avg", e["exp_avg"].cpu(), m)
        _same(f"{n} exp_avg_sq", e["exp_avg_sq"].cpu(), v)
        _same(f"{n} parameter", q.detach().cpu(), p.to(q.dtype))
        # (three steps of 1e-3 can leave a bf16 value of magnitude 1 where it was: the master moved)
        assert not torch.equal(e["master"], start[n].float())
    # no clipping: no norm, the plain update
    ddp2, opt2 = _optimizer(max_grad_norm=None)
    _set_grads(ddp2, 1)
    opt2.step()
    assert opt2.grad_norm is None
    for n, q in ddp2.module.named_parameters():
        p, _, _ = ops.adamw_reference(q.grad.cpu(), start[n].float().cpu(), torch.zeros(q.shape), torch.zeros(q.shape),
                                      ops.optim_sched(LR, BETAS, WD, 1), None, BETAS, EPS, q.ndim >= 2)
        _same(f"{n} unclipped", q.detach().cpu(), p.to(q.dtype))


def test_adamw_class_refuses():
    with pytest.raises(TypeError, match="DistributedDataParallel"):
        parallel.AdamW(Params(), LR)
    mod = Params()
    mod.router = torch.nn.Parameter(mod.router.detach().half())
    with pytest.raises(TypeError, match="bf16 or fp32"):
        parallel.AdamW(parallel.DistributedDataParallel(mod, _comm()), LR)
    mod = Params()
    mod.router = torch.nn.Parameter(mod.router.detach().t())
    with pytest.raises(ValueError, match="contiguous"):
        parallel.AdamW(parallel.DistributedDataParallel(mod, _comm()), LR)
    with pytest.raises(ValueError, match="optim"):
        parallel.AdamW(parallel.DistributedDataParallel(Params(), _comm()), LR, betas=(0.9, 1.0))
    with pytest.raises(ValueError, match="max_norm"):
        parallel.AdamW(parallel.DistributedDataParallel(Params(), _comm()), LR, max_grad_norm=0.0)


def test_graph_replay_is_the_eager_steps():
    warm_ddp, warm = _optimizer()  # every kernel has run once before the capture
    _set_grads(warm_ddp, 1)
    warm.step()
    eager_ddp, eager = _optimizer()
    ddp, opt = _optimizer()
    _set_grads(ddp, 1)
    cs = torch.cuda.Stream()
    cs.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(cs):
        with torch.cuda.graph(graph, stream=cs):
            opt.launch()
    torch.cuda.current_stream().wait_stream(cs)
    torch.cuda.synchronize()
    start = [q.detach().clone() for q in ddp.module.parameters()]
    for q, e in zip(start, eager_ddp.module.parameters()):
        assert torch.equal(q, e), "the capture itself ran the kernels"
    lrs = (1e-3, 5e-4, 2e-3)  # a schedule: the graph reads it from the device
    for step, lr in enumerate(lrs, 1):
        _set_grads(eager_ddp, step)
        eager.step(lr)
        _set_grads(ddp, step)
        opt.advance(lr)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(opt.clip, eager.clip)
        for (n, a), e in zip(ddp.module.named_parameters(), eager_ddp.module.parameters()):
            assert torch.equal(a, e), f"step {step}: the replay's {n} differs from the eager step"
    a, e = opt.state_dict(), eager.state_dict()
    for n in a["state"]:
        for k in ("master", "exp_avg", "exp_avg_sq"):
            assert torch.equal(a["state"][n][k], e["state"][n][k]), (n, k)
    assert any(not torch.equal(q, s) for q, s in zip(ddp.module.parameters(), start))


def test_llama_model_trains():
    from test_gpu_rms_norm import _ids, _model, _tp

    tp, ids = _tp(), _ids(2, 64)
    ddp = parallel.DistributedDataParallel(_model(tp), tp)
    opt = parallel.AdamW(ddp, 1e-3, max_grad_norm=1.0, weight_decay=0.01, tp=tp)
    start = {n: q.detach().clone() for n, q in ddp.module.named_parameters()}
    losses = []
    for _ in range(20):
        ddp.zero_grad()
        loss = ddp(ids)
        loss.backward()
        ddp.finish()
        opt.step()
        losses.append(loss.item())
    print(f"[optim model] loss {losses[0]:.4f} -> {losses[-1]:.4f}; last norm {opt.grad_norm.item():.4f}")
    assert losses[-1] < losses[0]
    sd = opt.state_dict()
    for n, q in ddp.module.named_parameters():
        assert not torch.equal(q.detach(), start[n]), f"{n} did not change"
        assert torch.equal(q.detach(), sd["state"][n]["master"].to(q.dtype)), f"{n} is not its master, rounded once"
    # the state moves to a fresh optimizer; one more step from the same gradients gives the same bits
    ddp.zero_grad()
    ddp(ids).backward()
    ddp.finish()
    grads = {n: q.grad.detach().clone() for n, q in ddp.module.named_parameters()}
    ddp2 = parallel.DistributedDataParallel(_model(tp), tp)
    opt2 = parallel.AdamW(ddp2, 1e-3, max_grad_norm=1.0, weight_decay=0.01, tp=tp)
    opt2.load_state_dict(copy.deepcopy(sd))
    for n, q in ddp2.module.named_parameters():
        assert torch.equal(q.detach(), dict(ddp.module.named_parameters())[n].detach()), n
        ddp2._view_of[id(q)].copy_(grads[n])
        q.grad = ddp2._view_of[id(q)]
    opt.step()
    opt2.step()
    assert opt2.t == opt.t == 21 and torch.equal(opt.clip, opt2.clip)
    a, b = opt.state_dict()["state"], opt2.state_dict()["state"]
    for n, q in ddp2.module.named_parameters():
        assert torch.equal(q.detach(), dict(ddp.module.named_parameters())[n].detach()), n
        for k in ("master", "exp_avg", "exp_avg_sq"):
            assert torch.equal(a[n][k], b[n][k]), (n, k)
    # keyed by name: the state does not depend on the buckets
    ddp3 = parallel.DistributedDataParallel(_model(tp), tp, bucket_bytes=1 << 20)
    opt3 = parallel.AdamW(ddp3, 1e-3, max_grad_norm=1.0, weight_decay=0.01, tp=tp)
    assert len(opt3.states) != len(opt.states)
    opt3.load_state_dict(copy.deepcopy(sd))
    c = opt3.state_dict()
    assert c["step"] == 20
    for n in sd["state"]:
        for k in ("master", "exp_avg", "exp_avg_sq"):
            assert torch.equal(c["state"][n][k], sd["state"][n][k]), (n, k)
