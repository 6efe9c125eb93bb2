"""Backward of the routed MoE collectives (DeviceGroup.moe_combine_backward and the
autograd dispatch of parallel.moe_dispatch) on p ranks sharing the GPU.

Every rank regenerates every rank's dout, topk_idx, weights, y and upstream gradient of a
case from per-(rank, case) seeded generators and builds the whole oracle locally: the row
every (token, slot) takes, in (local expert, source rank, token, slot) order.

Cases (the smallest shapes at which the kernel can go wrong; T = 37 + 5 * rank):
  a  El = 1, K = 1, fp32 D = 8 (two vectors per row), the last rank has T = 0
  b  El = 3, K = 2, bf16 D = 520 (65 vectors: one lane past a full wave pass): every first
     slot on expert 0, expert 1 chosen by nobody, ~10 % dropped slots, a token with every
     slot dropped
  c  El = 1, K = 8, fp16 D = 1032 (129 vectors: a ragged second pass), experts repeat
     within a token, ~10 % dropped slots, a token with every slot dropped
In every case a few row_of entries of the handle are overwritten with -1 on the device
while idx >= 0: the slot a dispatch refused for capacity.
Checks: dy bitwise against (w * dout.float()).to(dtype) per routed row (dout itself with
weights=None), refused rows and the rows at or past the rank's total keep their sentinel;
dweights within D * 2^-23 * sum |dout * y| of the fp64 dot, exactly 0 for a slot that is not
live, bitwise equal between two calls; x.grad of the autograd dispatch bitwise equal to the
unweighted moe_combine of the gradient and within the combine's tolerance of fp64; y.grad of
the autograd combine without weights; the binding refuses dweights without y; on 2
ranks the dispatch and the combine backward captured in a graph and replayed with new
dout, weights and routing.  Prints "moe backward OK" on success."""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", ".."))
from collective_communication_mpi_amd import MPI, Communicator  # noqa: E402
from collective_communication_mpi_amd import parallel  # noqa: E402
from collective_communication_mpi_amd.device import dtype_code  # noqa: E402

comm = Communicator(MPI.COMM_WORLD)
rank, p = comm.Get_rank(), comm.Get_size()
dev = comm.dev
D = dev.device
fails = []
SENTINEL = -512.0
SPARE = 8
TOL = {torch.float32: 1e-5, torch.bfloat16: 1e-2, torch.float16: 2e-3}  # moe_worker.check_close's

CASES = {
    "a": dict(El=1, K=1, dtype=torch.float32, Dm=8, T=lambda r: 0 if r == p - 1 else 37 + 5 * r),
    "b": dict(El=3, K=2, dtype=torch.bfloat16, Dm=520, T=lambda r: 37 + 5 * r),
    "c": dict(El=1, K=8, dtype=torch.float16, Dm=1032, T=lambda r: 37 + 5 * r),
}


def fail(msg):
    fails.append(msg)


def done():
    torch.cuda.synchronize()
    dev.check()


def gen_case(r, name, salt=0):
    """Rank r's (dout, topk_idx int64, weights, refused mask): identical on every rank that asks."""
    c = CASES[name]
    T, K, E = c["T"](r), c["K"], c["El"] * p
    g = torch.Generator(device=D).manual_seed(2_000_003 * (ord(name) + 131 * salt) + 7919 * r + 31)
    dout = (torch.randn(T, c["Dm"], generator=g, device=D, dtype=torch.float64) * 2).to(c["dtype"])
    w = torch.rand(T, K, generator=g, device=D, dtype=torch.float32) + 0.25
    if name == "b":
        idx = torch.randint(0, E - 1, (T, K), generator=g, device=D)
        idx = idx + (idx >= 1).long()                                 # expert 1: chosen by nobody
        idx[:, 0] = 0                                                 # every first slot on expert 0
    else:
        idx = torch.randint(0, E, (T, K), generator=g, device=D)
    idx[torch.rand(T, K, generator=g, device=D) < 0.1] = -1           # dropped slots
    if name != "a" and T > 1:
        idx[1, :] = -1                                                # a token with every slot dropped
    refused = (torch.rand(T, K, generator=g, device=D) < 0.06) & (idx >= 0)
    return dout, idx.long(), w, refused


def gen_rows(r, name, cap, salt, what):
    """Rank r's [cap, Dm] buffer `what` (0: y, 1: the gradient of recv_x)."""
    c = CASES[name]
    g = torch.Generator(device=D).manual_seed(3_000_017 * (ord(name) + 131 * salt) + 104_729 * r + 7 + what)
    return (torch.randn(cap, c["Dm"], generator=g, device=D, dtype=torch.float64) * 2).to(c["dtype"])


class Oracle:
    """Every (token, slot)'s owner and row, from all ranks' routing; this rank's expected results."""

    def __init__(self, name, salt=0):
        c = CASES[name]
        self.name, self.El, self.K, self.dtype, self.Dm = name, c["El"], c["K"], c["dtype"], c["Dm"]
        self.E = self.El * p
        data = [gen_case(r, name, salt) for r in range(p)]
        self.douts, self.idxs, self.ws, self.refused = ([d[j] for d in data] for j in range(4))
        Ts = [x.shape[0] for x in self.douts]
        self.T = Ts[rank]
        off = torch.tensor([sum(Ts[:i]) for i in range(p)], device=D)
        e_l, i_l, t_l, k_l = [], [], [], []
        for i, idx in enumerate(self.idxs):
            t, k = torch.meshgrid(torch.arange(Ts[i], device=D), torch.arange(self.K, device=D), indexing="ij")
            v = idx >= 0
            e_l.append(idx[v]); i_l.append(torch.full_like(idx[v], i)); t_l.append(t[v]); k_l.append(k[v])
        e, i, t, k = (torch.cat(z) for z in (e_l, i_l, t_l, k_l))
        order = torch.argsort(((e * p + i) * (max(Ts) + 1) + t) * self.K + k)  # (expert, source, token, slot)
        e, i, t, k = e[order], i[order], t[order], k[order]
        owner = e // self.El
        per_owner = torch.bincount(owner, minlength=p)
        row = torch.arange(e.numel(), device=D) - (torch.cumsum(per_owner, 0) - per_owner)[owner]
        self.n = per_owner.tolist()
        self.cap = max(self.n) + SPARE                       # the same on every rank
        self.owner, self.row, self.src, self.tok, self.slot = owner, row, i, t, k
        self.gtok = off[i] + t                               # token index in the concatenation over ranks
        self.dead = torch.cat(self.refused)[self.gtok, k]    # entries whose row_of is overwritten with -1
        self.ys = [gen_rows(r, name, self.cap, salt, 0) for r in range(p)]
        self.gs = [gen_rows(r, name, self.cap, salt, 1) for r in range(p)]

    def dy(self, weighted):
        """This rank's whole dy buffer: routed rows, the sentinel elsewhere."""
        m = self.owner == rank
        d = torch.cat(self.douts)[self.gtok[m]]
        if weighted:
            d = (torch.cat(self.ws)[self.gtok[m], self.slot[m]][:, None] * d.float()).to(self.dtype)
        d = d.clone()
        d[self.dead[m]] = SENTINEL
        want = torch.full((self.cap, self.Dm), SENTINEL, dtype=self.dtype, device=D)
        want[:self.n[rank]] = d
        return want

    def mine(self, live_only):
        m = self.src == rank
        if live_only:
            m = m & ~self.dead
        return m

    def dweights(self):
        """(fp64 dots, bounds D * 2^-23 * sum |dout * y|) as [T, K]; both 0 where the slot is not live."""
        m = self.mine(True)
        yrows = torch.cat(self.ys)[self.owner[m] * self.cap + self.row[m]]
        prod = self.douts[rank][self.tok[m]].double() * yrows.double()
        dot = torch.zeros(self.T, self.K, dtype=torch.float64, device=D)
        bound = torch.zeros_like(dot)
        dot[self.tok[m], self.slot[m]] = prod.sum(dim=1)
        bound[self.tok[m], self.slot[m]] = self.Dm * 2.0 ** -23 * prod.abs().sum(dim=1)
        return dot, bound

    def dx64(self):
        """fp64 sum over the routed slots of the owners' gradient rows."""
        m = self.mine(False)
        out = torch.zeros(self.T, self.Dm, dtype=torch.float64, device=D)
        out.index_add_(0, self.tok[m], torch.cat(self.gs)[self.owner[m] * self.cap + self.row[m]].double())
        return out


def check_backward(tag, o, dy, dw, weighted):
    if not torch.equal(dy, o.dy(weighted)):
        want = o.dy(weighted)
        bad = (dy != want).any(dim=1).nonzero().reshape(-1).tolist()
        fail(f"{tag}: dy differs in rows {bad[:8]} of {o.n[rank]} routed (+{SPARE} spare)")
    if dw is not None:
        dot, bound = o.dweights()
        err = (dw.double() - dot).abs()
        live = bound > 0
        ratio = (err[live] / bound[live]).max().item() if live.any() else 0.0
        print(f"[rank {rank}] {tag}: dweights worst error / bound {ratio:.4f}", flush=True)
        if not bool((err <= bound).all()):
            fail(f"{tag}: dweights off by {err.max().item()} (worst error / bound {ratio:.3f})")
        dead = torch.ones_like(live)
        m = o.mine(True)
        dead[o.tok[m], o.slot[m]] = False
        if dead.any() and dw[dead].abs().max().item() != 0:
            fail(f"{tag}: dweights of a slot that is not live is not 0")


def knock_out(h, o):
    """The capacity-refused slot: row_of = -1 on the device while idx >= 0."""
    h.row_of.masked_fill_(o.refused[rank], -1)


def run_case(name):
    o = Oracle(name)
    dout, idx, w = o.douts[rank], o.idxs[rank], o.ws[rank]
    # dispatch backward through autograd, on the untouched handle
    x = dout.clone().requires_grad_(True)
    recv, h = parallel.moe_dispatch(comm if name == "a" else dev, x, idx, o.E, o.cap)
    if not dev.is_symmetric(recv) or tuple(recv.shape) != (o.cap, o.Dm):
        fail(f"dispatch[{name}]: recv_x is not a [cap, D] heap tensor")
    recv.backward(o.gs[rank])
    done()
    g_heap = dev.empty((o.cap, o.Dm), o.dtype)
    g_heap.copy_(o.gs[rank])
    direct = dev.moe_combine(g_heap, h, None)
    done()
    if x.grad is None or not torch.equal(x.grad, direct):
        fail(f"dispatch backward[{name}]: x.grad is not moe_combine(g, h, None)")
    else:
        tol = TOL[o.dtype] * o.K
        if not torch.allclose(x.grad.double(), o.dx64(), rtol=tol, atol=4 * tol):
            fail(f"dispatch backward[{name}]: max diff {(x.grad.double() - o.dx64()).abs().max().item()}")
    # combine backward on the handle with refused slots
    knock_out(h, o)
    y = dev.empty((o.cap, o.Dm), o.dtype)
    y.copy_(o.ys[rank])
    dy = dev.empty((o.cap, o.Dm), o.dtype)
    dy.fill_(SENTINEL)
    got, dw = dev.moe_combine_backward(dout, h, w, y=y, dy=dy)
    done()
    if got is not dy:
        fail(f"combine backward[{name}]: dy= not returned")
    check_backward(f"combine backward[{name}, weighted]", o, dy, dw, True)
    dy2 = dev.empty((o.cap + 3, o.Dm), o.dtype)        # more rows than cap, through the Communicator
    dy2.fill_(SENTINEL)
    _, dw2 = comm.moe_combine_backward(dout, h, w, y=y, dy=dy2)
    done()
    if not torch.equal(dw, dw2) or not torch.equal(dy2[:o.cap], dy):
        fail(f"combine backward[{name}]: two calls differ")
    if not torch.equal(dy2[o.cap:], torch.full_like(dy2[o.cap:], SENTINEL)):
        fail(f"combine backward[{name}]: rows past cap overwritten")
    # weights=None: a bitwise copy; and no y: nothing pulled
    dy.fill_(SENTINEL)
    _, dw = dev.moe_combine_backward(dout, h, None, y=y, dy=dy)
    done()
    check_backward(f"combine backward[{name}, weights=None]", o, dy, dw, False)
    got, none = dev.moe_combine_backward(dout, h, w)
    done()
    if none is not None:
        fail(f"combine backward[{name}]: dweights returned without y")
    written = ~o.dead[o.owner == rank]                 # a refused row of a fresh buffer is unspecified
    if not dev.is_symmetric(got) or got.shape[0] < o.cap or \
            not torch.equal(got[:o.n[rank]][written], o.dy(True)[:o.n[rank]][written]):
        fail(f"combine backward[{name}]: the allocated dy differs")
    # the autograd combine without weights: y.grad is the unweighted dy, no dweights asked for
    ya = y.clone().requires_grad_(True)                # not in the heap: staged by the forward
    parallel.moe_combine(dev, ya, h, None).backward(dout)
    done()
    if ya.grad is None or not torch.equal(ya.grad[:o.n[rank]][written], o.dy(False)[:o.n[rank]][written]):
        fail(f"autograd combine[{name}, weights=None]: y.grad is not dout per routed row")
    # the binding's own rule, on every rank before any launch: dweights without y
    try:
        dev.dc.moe_combine_bwd(dout.data_ptr(), 0, 0, dy.data_ptr(), dy.shape[0], dw2.data_ptr() or 16,
                               h.topk_idx.data_ptr(), h.row_of.data_ptr(), 0, h.T, h.K, h.num_experts,
                               o.Dm * dout.element_size(), dtype_code(o.dtype),
                               torch.cuda.current_stream().cuda_stream, 1)
        fail(f"combine backward[{name}]: dweights without y was accepted")
    except ValueError as e:
        if "together" not in str(e):
            fail(f"combine backward[{name}]: unexpected error {e}")


def graph():
    """dispatch + refusal + combine backward captured once, replayed with new inputs and routing."""
    o0, o1 = Oracle("b", salt=1), Oracle("b", salt=2)
    cap = max(o0.cap, o1.cap)
    o0.cap = o1.cap = cap
    for o in (o0, o1):                                   # the buffers' rows follow the shared cap
        o.ys = [gen_rows(r, "b", cap, 9, 0) for r in range(p)]
    dout, idx, w, refused = o0.douts[rank].clone(), o0.idxs[rank].clone(), o0.ws[rank].clone(), o0.refused[rank].clone()
    recv, y, dy = (dev.empty((cap, o0.Dm), o0.dtype) for _ in range(3))
    y.copy_(o0.ys[rank])
    cs = torch.cuda.Stream()
    cs.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(cs):
        with torch.cuda.graph(g, stream=cs):
            h = dev.moe_dispatch(dout, idx, o0.E, recv)
            h.row_of.masked_fill_(refused, -1)
            _, dw = dev.moe_combine_backward(dout, h, w, y=y, dy=dy)
    torch.cuda.current_stream().wait_stream(cs)
    o = o1
    dout.copy_(o.douts[rank]); idx.copy_(o.idxs[rank]); w.copy_(o.ws[rank]); refused.copy_(o.refused[rank])
    dy.fill_(SENTINEL)
    torch.cuda.synchronize()
    dev.host.Barrier()
    g.replay()
    done()
    check_backward("graph replay", o, dy, dw, True)
    del g


t0 = time.time()
for name in "abc":
    run_case(name)
if p == 2 and dev.ranks_per_device <= 2:
    graph()
torch.cuda.synchronize()
dev.check()
bad = comm.comm.allreduce(len(fails), op=MPI.SUM)
if fails:
    print(f"[rank {rank}] " + "\n".join(fails[:20]), flush=True)
if rank == 0:
    print(f"moe backward OK ({time.time() - t0:.1f}s)" if bad == 0 else f"moe backward FAILED ({bad})", flush=True)
sys.exit(1 if bad else 0)
