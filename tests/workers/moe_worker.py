"""Routed MoE dispatch / combine (DeviceGroup.moe_dispatch, moe_combine) on p ranks
sharing the GPU.

Every rank regenerates every rank's x, topk_idx and weights of a case from
per-(rank, case) seeded generators and builds the whole oracle locally: the rows
every rank must receive, in (local expert, source rank, token, slot) order, and
the row every (token, slot) takes.

Cases (the smallest shapes at which the kernels can go wrong):
  a  El = 1, K = 1, fp32 D = 4 (16-B rows), T = 5 + rank but 0 on rank 0
  b  El = 3, K = 2, bf16 D = 24 (48-B rows), T = 33: an expert nobody chooses, dropped
     slots, a token with the same expert twice, a token with every slot dropped
  c  El = 2, K = 8, bf16 D = 520 (1040-B rows: longer than one wave's span), T = 64
  d  El = 1, K = 2, fp16 D = 32, T = 700, experts 0 and 1 only (1400 entries: more than
     one routing chunk, extreme skew)
  e  El = 8 at p = 8 else 4, K = 4, fp32 D = 64, T = 96: a realistic mix
Checks: dispatch is a pure copy (rows, spare rows untouched, expert_counts, row_of);
El = 1 bitwise against the existing alltoallv with device counts; round trips;
combine bitwise (weights=None) and against fp64 (weighted); 20 skewed back-to-back
pairs; HIP graph replays (<= 2 ranks per GPU); a buffer one row short.
Prints "moe OK" on success."""
import os
import random
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", ".."))
from collective_communication_mpi_amd import MPI, Communicator  # noqa: E402
from collective_communication_mpi_amd.device import moe_layout  # noqa: E402

comm = Communicator(MPI.COMM_WORLD)
rank, p = comm.Get_rank(), comm.Get_size()
dev = comm.dev
D = dev.device
fails = []
SENTINEL = -512.0
SPARE = 8
TOL = {torch.float32: 1e-5, torch.bfloat16: 1e-2, torch.float16: 2e-3}  # device_worker.check's

CASES = {
    "a": dict(El=1, K=1, dtype=torch.float32, Dm=4, T=lambda r: 0 if r == 0 else 5 + r),
    "b": dict(El=3, K=2, dtype=torch.bfloat16, Dm=24, T=lambda r: 33),
    "c": dict(El=2, K=8, dtype=torch.bfloat16, Dm=520, T=lambda r: 64),
    "d": dict(El=1, K=2, dtype=torch.float16, Dm=32, T=lambda r: 700),
    "e": dict(El=8 if p == 8 else 4, K=4, dtype=torch.float32, Dm=64, T=lambda r: 96),
}


def fail(msg):
    fails.append(msg)


def gen_case(r, name, salt=0):
    """Rank r's (x, topk_idx int64, weights) of a case: identical on every rank that asks."""
    c = CASES[name]
    T, K, E = c["T"](r), c["K"], c["El"] * p
    g = torch.Generator(device=D).manual_seed(1_000_003 * (ord(name) + 131 * salt) + 7919 * r + 29)
    x = (torch.randn(T, c["Dm"], generator=g, device=D, dtype=torch.float64) * 3).to(c["dtype"])
    w = torch.rand(T, K, generator=g, device=D, dtype=torch.float32) + 0.25
    if name == "d":  # experts 0 and 1 only, the two slots of a token distinct
        first = torch.randint(0, 2, (T, 1), generator=g, device=D)
        idx = torch.cat([first, 1 - first], dim=1)
    elif name == "e":  # K distinct experts per token
        idx = torch.rand(T, E, generator=g, device=D).topk(K, dim=1).indices
    elif name in ("a", "c"):  # c: K = 8 slots over as few as 4 experts, so experts repeat within a token
        idx = torch.randint(0, E, (T, K), generator=g, device=D)
    else:
        idx = torch.randint(0, E - 1, (T, K), generator=g, device=D)
        idx = idx + (idx >= 1).long()                                 # expert 1: chosen by nobody
        idx[torch.rand(T, K, generator=g, device=D) < 0.15] = -1      # some dropped slots
        idx[0, :] = 2 + r % 2                                         # the same expert in both slots
        idx[1, :] = -1                                                # a token with every slot dropped
    return x, idx.long(), w


class Oracle:
    """Every rank's expected receive rows and every (token, slot)'s row, from all ranks' inputs."""

    def __init__(self, name, salt=0, K=None):
        c = CASES[name]
        self.name, self.El, self.dtype, self.Dm = name, c["El"], c["dtype"], c["Dm"]
        self.E = self.El * p
        data = [gen_case(r, name, salt) for r in range(p)]
        if K is not None:  # the first K slots only
            data = [(x, idx[:, :K].contiguous(), w[:, :K].contiguous()) for x, idx, w in data]
        self.K = data[0][1].shape[1]
        self.xs, self.idxs, self.ws = [d[0] for d in data], [d[1] for d in data], [d[2] for d in data]
        Ts = [x.shape[0] for x in self.xs]
        off = [0]
        for t in Ts:
            off.append(off[-1] + t)
        e_l, i_l, t_l, k_l = [], [], [], []
        for i, idx in enumerate(self.idxs):
            t, k = torch.meshgrid(torch.arange(Ts[i], device=D), torch.arange(self.K, device=D), indexing="ij")
            v = idx >= 0
            e_l.append(idx[v]); i_l.append(torch.full_like(idx[v], i)); t_l.append(t[v]); k_l.append(k[v])
        e, i, t, k = (torch.cat(z) for z in (e_l, i_l, t_l, k_l))
        key = ((e * p + i) * (max(Ts) + 1) + t) * self.K + k   # (expert, source, token, slot), unique
        order = torch.argsort(key)
        e, i, t, k = e[order], i[order], t[order], k[order]
        owner = e // self.El
        per_owner = torch.bincount(owner, minlength=p)
        starts = torch.cumsum(per_owner, 0) - per_owner
        row = torch.arange(e.numel(), device=D) - starts[owner]
        xcat = torch.cat(self.xs)
        rows = xcat[torch.tensor(off[:-1], device=D)[i] + t]
        self.n = per_owner.tolist()
        self.recv = [rows[owner == j] for j in range(p)]
        self.elocal = [(e % self.El)[owner == j] for j in range(p)]
        self.last_source_rank0 = int(i[owner == 0][-1]) if self.n[0] else -1
        self.row_of = []
        for r in range(p):
            ro = torch.full((Ts[r], self.K), -1, dtype=torch.int64, device=D)
            m = i == r
            ro[t[m], k[m]] = row[m]
            self.row_of.append(ro)
        self.counts = torch.stack([torch.bincount(idx[idx >= 0], minlength=self.E) for idx in self.idxs]).cpu().numpy()
        self.expert_counts = torch.bincount(self.elocal[rank], minlength=self.El)

    def combine(self, ys, w=None, wide=False):
        """out of this rank from every rank's y: slot order k = 0..K-1, fp32 (or fp64)."""
        idx, ro = self.idxs[rank], self.row_of[rank]
        at = torch.float64 if wide else torch.float32
        acc = torch.zeros(idx.shape[0], self.Dm, dtype=at, device=D)
        for k in range(self.K):
            term = torch.zeros_like(acc)
            for j in range(p):
                m = (idx[:, k] >= 0) & (idx[:, k].clamp(min=0) // self.El == j)
                term[m] = ys[j][ro[m, k]].to(at)
            if w is not None:
                term = term * w[:, k:k + 1].to(at)
            acc = acc + term
        return acc


def expert_scaled(o):
    """y of every rank: (local expert + 1) * row, rounded to the dtype."""
    return [(o.recv[j].float() * (o.elocal[j] + 1).float()[:, None]).to(o.dtype) for j in range(p)]


def row_scaled(rows):
    """A y that depends on the row index only (no data-dependent shapes on the device)."""
    s = (torch.arange(rows.shape[0], device=D) % 7 + 1).float()[:, None]
    return (rows.float() * s).to(rows.dtype)


def new_recv(o, spare=SPARE):
    r = dev.empty((o.n[rank] + spare, o.Dm), o.dtype)
    r.fill_(SENTINEL)
    return r


def done():
    torch.cuda.synchronize()
    dev.check()


def check_dispatch(tag, o, recv, h):
    n = o.n[rank]
    if not torch.equal(recv[:n], o.recv[rank]):
        fail(f"{tag}: recv_x rows differ")
    if not torch.equal(recv[n:], torch.full_like(recv[n:], SENTINEL)):
        fail(f"{tag}: spare rows overwritten")
    if not torch.equal(h.expert_counts, o.expert_counts):
        fail(f"{tag}: expert_counts {h.expert_counts.tolist()} != {o.expert_counts.tolist()}")
    if not torch.equal(h.row_of.long(), o.row_of[rank]):
        fail(f"{tag}: row_of differs")
    base, ec, totals = moe_layout(o.counts, rank)
    if ec.tolist() != o.expert_counts.tolist() or totals.tolist() != o.n:
        fail(f"{tag}: moe_layout disagrees with the oracle")


def check_close(tag, got, want64, o):
    tol = TOL[o.dtype] * o.K
    if not torch.allclose(got.double(), want64, rtol=tol, atol=4 * tol):
        fail(f"{tag}: max diff {(got.double() - want64).abs().max().item()}")
    dropped = (o.idxs[rank] < 0).all(dim=1)
    if dropped.any() and got[dropped].abs().max().item() != 0:
        fail(f"{tag}: a token with every slot dropped is not zero")


def run_case(name, int32_idx):
    o = Oracle(name)
    x, idx, w = o.xs[rank], o.idxs[rank], o.ws[rank]
    recv = new_recv(o)
    h = dev.moe_dispatch(x, idx.int() if int32_idx else idx, o.E, recv)
    done()
    check_dispatch(f"dispatch[{name}]", o, recv, h)
    if o.El == 1:
        # the contract order is alltoallv's here: a stable sort by destination + pack,
        # through the existing kernel with the counts on the device, must give the same bytes
        flat = idx.reshape(-1)
        keep = torch.nonzero(flat >= 0).reshape(-1)
        order = keep[torch.sort(flat[keep], stable=True).indices]
        packed = x[order // o.K]
        xs = dev.empty(max(1, packed.numel()), o.dtype)
        xs[:packed.numel()].copy_(packed.reshape(-1))
        cnt = torch.bincount(flat[keep], minlength=p) * o.Dm
        y2 = dev.empty(recv.numel(), o.dtype)
        y2.fill_(SENTINEL)
        dev.alltoallv(xs, cnt, y2, None)
        done()
        if not torch.equal(y2.view_as(recv), recv):
            fail(f"dispatch[{name}]: differs from alltoallv with device counts")
    # round trip: y = recv_x, no weights
    y = dev.empty(tuple(recv.shape), o.dtype)
    if name in ("a", "d"):
        y.copy_(recv)
        out = dev.moe_combine(y, h)
        done()
        if not torch.equal(out, (o.K * x.float()).to(o.dtype)):
            fail(f"round trip[{name}]: out != {o.K} * x")
    # weights=None, y = (local expert + 1) * row: bitwise against the fp32 slot-order sum
    ys = expert_scaled(o)
    y.fill_(SENTINEL)
    y[:o.n[rank]].copy_(ys[rank])
    out = dev.moe_combine(y, h)
    done()
    if not torch.equal(out, o.combine(ys).to(o.dtype)):
        fail(f"combine[{name}, weights=None]: not the fp32 slot-order sum")
    # weighted, into a caller's out
    out2 = torch.full((x.shape[0], o.Dm), 7.0, dtype=o.dtype, device=D)
    got = dev.moe_combine(y, h, w, out=out2)
    done()
    if got is not out2:
        fail(f"combine[{name}]: out= not returned")
    check_close(f"combine[{name}, weighted]", out2, o.combine(ys, w, wide=True), o)


def round_trip_two_experts():
    """K = 2 distinct experts, fp32: out is bitwise 2 * x."""
    o = Oracle("e", K=2)
    recv = new_recv(o)
    h = comm.moe_dispatch(o.xs[rank], o.idxs[rank], o.E, recv)  # through the Communicator
    done()
    check_dispatch("dispatch[e, K=2]", o, recv, h)
    out = comm.moe_combine(recv, h)
    done()
    if not torch.equal(out, 2 * o.xs[rank]):
        fail("round trip[e, K=2]: out != 2 * x")
    # buffers outside the symmetric heap are refused on every rank before any launch
    for what, call in (("recv_x", lambda: dev.moe_dispatch(o.xs[rank], o.idxs[rank], o.E, torch.empty_like(recv))),
                       ("y", lambda: dev.moe_combine(torch.empty_like(recv), h))):
        try:
            call()
            fail(f"{what} outside the symmetric heap was accepted")
        except ValueError:
            pass


def skew(iters=20):
    """Back-to-back dispatch -> combine pairs, ranks arriving in random order, the same
    buffers every time (epoch and scratch reuse); results checked at the end."""
    rng = random.Random(77 + rank)
    os_ = [Oracle("e", salt=s) for s in (1, 2)]
    cap = max(max(o.n) for o in os_) + SPARE
    recv, y = dev.empty((cap, 64), torch.float32), dev.empty((cap, 64), torch.float32)
    pending = []
    for it in range(iters):
        o = os_[it % 2]
        d = rng.random()
        if d < 0.3:
            time.sleep(rng.random() * 0.004)
        elif d < 0.6:
            torch.cuda._sleep(rng.randint(1000, 200000))
        recv.fill_(SENTINEL)
        h = dev.moe_dispatch(o.xs[rank], o.idxs[rank], o.E, recv)
        y.copy_(row_scaled(recv))
        w = o.ws[rank] if it % 2 == 0 or it % 3 == 0 else None
        out = dev.moe_combine(y, h, w)
        pending.append((it, o, w, recv.clone(), h, out))
    done()
    for it, o, w, got, h, out in pending:
        check_dispatch(f"skew[{it}]", o, got[:o.n[rank] + SPARE], h)
        ys = [row_scaled(o.recv[j]) for j in range(p)]
        if w is None:
            if not torch.equal(out, o.combine(ys)):
                fail(f"skew[{it}]: combine not bitwise")
        else:
            check_close(f"skew[{it}]", out, o.combine(ys, w, wide=True), o)


def graph():
    """dispatch + combine captured once, replayed with new indices, rows and weights."""
    os_ = [Oracle("e", salt=s) for s in (3, 4, 5)]
    cap = max(max(o.n) for o in os_) + SPARE
    o0 = os_[0]
    x, idx, w = o0.xs[rank].clone(), o0.idxs[rank].clone(), o0.ws[rank].clone()
    recv, y = dev.empty((cap, 64), torch.float32), dev.empty((cap, 64), torch.float32)
    out = torch.empty_like(x)
    recv.fill_(SENTINEL)
    cs = torch.cuda.Stream()
    cs.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(cs):
        with torch.cuda.graph(g, stream=cs):
            h = dev.moe_dispatch(x, idx, o0.E, recv)
            y.copy_(row_scaled(recv))
            dev.moe_combine(y, h, w, out=out)
    torch.cuda.current_stream().wait_stream(cs)
    for rep, o in enumerate(os_):
        x.copy_(o.xs[rank]); idx.copy_(o.idxs[rank]); w.copy_(o.ws[rank])
        recv.fill_(SENTINEL)
        out.zero_()
        torch.cuda.synchronize()
        dev.host.Barrier()
        g.replay()
        done()
        check_dispatch(f"graph[{rep}]", o, recv[:o.n[rank] + SPARE], h)
        check_close(f"graph[{rep}]", out, o.combine([row_scaled(o.recv[j]) for j in range(p)], w, wide=True), o)
    del g


def capacity():
    """Rank 0's buffer one row short: the row is refused, its sender reports 0xA00, nothing
    is written past the buffer, and the next call works."""
    o = Oracle("e", salt=6)
    full = new_recv(o)
    short = full[:o.n[0] - 1] if rank == 0 else full
    h = dev.moe_dispatch(o.xs[rank], o.idxs[rank], o.E, short)
    torch.cuda.synchronize()
    sender = o.last_source_rank0
    try:
        dev.check()
        if rank == sender:
            fail("capacity: the overflowing row was not reported")
    except RuntimeError as e:
        if rank != sender or "0xa0" not in str(e):
            fail(f"capacity: unexpected error on rank {rank}: {e}")
    if rank == 0:
        if not torch.equal(full[o.n[0] - 1:], torch.full_like(full[o.n[0] - 1:], SENTINEL)):
            fail("capacity: written past the short buffer")
        if not torch.equal(full[:o.n[0] - 1], o.recv[0][:-1]):
            fail("capacity: the rows that fit differ")
    if rank == sender:
        want = o.row_of[rank].clone()
        want[(want == o.n[0] - 1) & (o.idxs[rank].clamp(min=0) // o.El == 0) & (o.idxs[rank] >= 0)] = -1
        if not torch.equal(h.row_of.long(), want):
            fail("capacity: row_of of the refused row is not -1")
    dev.host.Barrier()
    full.fill_(SENTINEL)
    h = dev.moe_dispatch(o.xs[rank], o.idxs[rank], o.E, full)
    done()
    check_dispatch("capacity: following call", o, full, h)


t0 = time.time()
for n_, name in enumerate("abcde"):
    run_case(name, int32_idx=n_ % 2 == 1)
round_trip_two_experts()
skew()
if dev.ranks_per_device <= 2:
    graph()
capacity()
torch.cuda.synchronize()
dev.check()
bad = comm.comm.allreduce(len(fails), op=MPI.SUM)
if fails:
    print(f"[rank {rank}] " + "\n".join(fails[:20]), flush=True)
if rank == 0:
    print(f"moe OK ({time.time() - t0:.1f}s)" if bad == 0 else f"moe FAILED ({bad})", flush=True)
sys.exit(1 if bad else 0)
