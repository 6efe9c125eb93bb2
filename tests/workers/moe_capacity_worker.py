"""Routed MoE dispatch with a per-expert capacity (``expert_capacity``) on p ranks sharing
the GPU: token dropping, the compacted row layout, and the combine / combine backward /
grouped GEMM over the result.

Every rank regenerates every rank's x, topk_idx, weights and dout of a case from
per-(rank, case) seeded CPU generators and builds the whole oracle locally by walking the
entries in (expert, source rank, token, slot) order: entry number q of an expert is kept iff
q < Ce; the kept entries, in that order, are the rows of the expert's rank.

Cases (receive buffers have (E / p) * Ce rows plus 8 sentinel rows):
  a  El = 1, K = 1, fp32 D = 4, T = 5 + rank but 0 on rank 0, every token to expert 0, Ce = 4:
     rank 1 keeps 4 of 6, every later rank nothing (before >= Ce)
  b  El = 3, K = 2, bf16 D = 24, T = 33, skewed random routing with router-dropped slots,
     expert 1 chosen by nobody, row 0 with one expert in both slots, a token with every slot
     dropped, Ce = 16.  Asserted from the oracle alone: an expert over capacity, a non-empty one
     under it, a token whose slot 0 is kept and slot 1 dropped
  c  El = 2, K = 8, bf16 D = 520, T = 64, Ce = 1: almost everything dropped, many tokens
     without a kept slot (zero rows in the combine)
  d  El = 1, K = 2, fp16 D = 32, T = 700, experts 0 and 1 only, Ce = 1000: positions past one
     routing chunk; rank 0 kept whole, rank 1 cut at 300, later ranks nothing
  e  case b's inputs with Ce = the largest column total: bit for bit the call without
     expert_capacity (recv_x, row_of, expert_counts), num_dropped = 0
Checks per case: kept rows bitwise and in order, rows past the total and the sentinels
untouched, expert_counts / row_of / num_dropped exact, the host mirrors (moe_layout,
moe_kept) agree, check() clean; moe_combine(weights=None) bitwise against the fp32
slot-ordered sum, weighted against fp64 with moe_worker.py's TOL; moe_combine_backward: kept
dy rows bitwise, dweights of dropped slots exactly 0 (kept ones within moe_backward_worker.py's
bound D * 2^-23 * sum |dout * y|); on case b ops.grouped_gemm_nt over the result with
h.expert_counts against the per-expert loop (test_gpu_grouped_gemm.py's fp32 tolerance);
on <= 2 ranks per GPU a captured dispatch + combine with expert_capacity, replayed with new
routing that changes which entries drop.
Prints "moe capacity OK" on success."""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", ".."))

SENTINEL = -512.0
SPARE = 8
TOL = {torch.float32: 1e-5, torch.bfloat16: 1e-2, torch.float16: 2e-3}  # moe_worker.py's

CASES = {
    "a": dict(El=1, K=1, dtype=torch.float32, Dm=4, T=lambda r: 0 if r == 0 else 5 + r, Ce=4),
    "b": dict(El=3, K=2, dtype=torch.bfloat16, Dm=24, T=lambda r: 33, Ce=16),
    "c": dict(El=2, K=8, dtype=torch.bfloat16, Dm=520, T=lambda r: 64, Ce=1),
    "d": dict(El=1, K=2, dtype=torch.float16, Dm=32, T=lambda r: 700, Ce=1000),
}


def gen_case(r, name, p, salt=0):
    """Rank r's (x, topk_idx int64, weights, dout) of a case, on the CPU: identical wherever asked."""
    c = CASES[name]
    T, K, E = c["T"](r), c["K"], c["El"] * p
    g = torch.Generator().manual_seed(2_000_003 * (ord(name) + 131 * salt) + 7919 * r + 31)
    x = (torch.randn(T, c["Dm"], generator=g, dtype=torch.float64) * 3).to(c["dtype"])
    w = torch.rand(T, K, generator=g, dtype=torch.float32) + 0.25
    dout = torch.randn(T, c["Dm"], generator=g, dtype=torch.float64).to(c["dtype"])
    if name == "a":
        idx = torch.zeros(T, K, dtype=torch.int64)
    elif name == "d":  # experts 0 and 1 only, the two slots of a token distinct
        first = torch.randint(0, 2, (T, 1), generator=g)
        idx = torch.cat([first, 1 - first], dim=1)
    elif name == "c":
        idx = torch.randint(0, E, (T, K), generator=g)
    else:  # skewed: expert e drawn with weight 1 / (1 + e), expert 1 never
        pr = 1.0 / (1.0 + torch.arange(E, dtype=torch.float64))
        pr[1] = 0
        idx = torch.multinomial(pr.expand(T, E), K, replacement=True, generator=g)
        idx[torch.rand(T, K, generator=g) < 0.15] = -1        # slots the router dropped
        idx[0, :] = 2 + r % 2                                  # the same expert in both slots
        idx[1, :] = -1                                         # a token with every slot dropped
    return x, idx.long(), w, dout


class Oracle:
    """Every rank's expected rows and every (token, slot)'s row under capacity Ce (None: no
    limit), from all ranks' inputs; CPU tensors."""

    def __init__(self, name, p, Ce="case", salt=0):
        c = CASES[name]
        self.name, self.p, self.El, self.dtype, self.Dm, self.K = name, p, c["El"], c["dtype"], c["Dm"], c["K"]
        self.E = self.El * p
        self.Ce = c["Ce"] if Ce == "case" else Ce
        data = [gen_case(r, name, p, salt) for r in range(p)]
        self.xs, self.idxs, self.ws, self.douts = ([d[j] for d in data] for j in range(4))
        Ts = [x.shape[0] for x in self.xs]
        off = [0]
        for t in Ts:
            off.append(off[-1] + t)
        e_l, i_l, t_l, k_l = [], [], [], []
        for i, idx in enumerate(self.idxs):
            t, k = torch.meshgrid(torch.arange(Ts[i]), torch.arange(self.K), indexing="ij")
            v = idx >= 0
            e_l.append(idx[v]); i_l.append(torch.full_like(idx[v], i)); t_l.append(t[v]); k_l.append(k[v])
        e, i, t, k = (torch.cat(z) for z in (e_l, i_l, t_l, k_l))
        key = ((e * p + i) * (max(Ts) + 1) + t) * self.K + k   # (expert, source, token, slot), unique
        order = torch.argsort(key)
        e, i, t, k = e[order], i[order], t[order], k[order]
        self.col = torch.bincount(e, minlength=self.E)          # entries per expert before any drop
        q = torch.arange(e.numel()) - (torch.cumsum(self.col, 0) - self.col)[e]   # number within the expert
        kept = q < self.Ce if self.Ce is not None else torch.ones_like(q, dtype=torch.bool)
        self.counts = torch.stack([torch.bincount(idx[idx >= 0], minlength=self.E) for idx in self.idxs]).numpy()
        self.dropped = [int(((i == r) & ~kept).sum()) for r in range(p)]
        self.kept_mask = []                                      # per rank [T, K]: routed and kept
        for r in range(p):
            km = torch.zeros(Ts[r], self.K, dtype=torch.bool)
            m = (i == r) & kept
            km[t[m], k[m]] = True
            self.kept_mask.append(km)
        e, i, t, k = e[kept], i[kept], t[kept], k[kept]
        owner = e // self.El
        per_owner = torch.bincount(owner, minlength=p)
        starts = torch.cumsum(per_owner, 0) - per_owner
        row = torch.arange(e.numel()) - starts[owner]
        src = torch.tensor(off[:-1], dtype=torch.int64)[i] + t
        self.n = per_owner.tolist()
        self.recv = [torch.cat(self.xs)[src][owner == j] for j in range(p)]
        self.elocal = [(e % self.El)[owner == j] for j in range(p)]
        self.src = [(i[owner == j], t[owner == j], k[owner == j]) for j in range(p)]   # of every row of rank j
        self.row_of = []
        for r in range(p):
            ro = torch.full((Ts[r], self.K), -1, dtype=torch.int64)
            m = i == r
            ro[t[m], k[m]] = row[m]
            self.row_of.append(ro)
        self.expert_counts = [torch.bincount(self.elocal[j], minlength=self.El) for j in range(p)]

    def combine(self, rank, ys, w=None, wide=False):
        """out of ``rank`` from every rank's y: slot order k = 0..K-1, fp32 (or fp64)."""
        idx, ro = self.idxs[rank], self.row_of[rank]
        at = torch.float64 if wide else torch.float32
        acc = torch.zeros(idx.shape[0], self.Dm, dtype=at)
        for k in range(self.K):
            term = torch.zeros_like(acc)
            for j in range(self.p):
                m = (ro[:, k] >= 0) & (idx[:, k].clamp(min=0) // self.El == j)
                term[m] = ys[j][ro[m, k]].to(at)
            if w is not None:
                term = term * w[:, k:k + 1].to(at)
            acc = acc + term
        return acc

    def dy(self, rank, weighted):
        """The rows peers push into ``rank``'s dy: w[t, k] * dout[t], one fp32 multiply, one rounding."""
        i, t, k = self.src[rank]
        rows = []
        for s in range(self.p):
            m = i == s
            d = self.douts[s][t[m]]
            rows.append((m, (self.ws[s][t[m], k[m]][:, None] * d.float()).to(self.dtype) if weighted else d))
        out = torch.zeros(self.n[rank], self.Dm, dtype=self.dtype)
        for m, v in rows:
            out[m] = v
        return out


def expert_scaled(o):
    """y of every rank: (local expert + 1) * row, rounded to the dtype."""
    return [(o.recv[j].float() * (o.elocal[j] + 1).float()[:, None]).to(o.dtype) for j in range(o.p)]


def case_b_conditions(o):
    """What case b must exercise, from the oracle alone; a list of what is missing."""
    missing = []
    if not (o.col > o.Ce).any():
        missing.append("no expert over capacity")
    if not ((o.col > 0) & (o.col < o.Ce)).any():
        missing.append("no non-empty expert under capacity")
    if o.col[1] != 0:
        missing.append("expert 1 was chosen")
    if not any((km[:, 0] & ~km[:, 1] & (idx[:, 1] >= 0)).any() for km, idx in zip(o.kept_mask, o.idxs)):
        missing.append("no token with slot 0 kept and slot 1 dropped over capacity")
    return missing


def main():
    torch.set_num_threads(1)  # the oracle is small CPU work in p processes at once
    from collective_communication_mpi_amd import MPI, Communicator, ops
    from collective_communication_mpi_amd.device import moe_kept, moe_layout

    comm = Communicator(MPI.COMM_WORLD)
    rank, p = comm.Get_rank(), comm.Get_size()
    dev = comm.dev
    D = dev.device
    fails = []
    t0 = time.time()

    def fail(msg):
        fails.append(msg)

    def done():
        torch.cuda.synchronize()
        dev.check()

    def new_buf(o, Ce):
        r = dev.empty((o.El * Ce + SPARE, o.Dm), o.dtype)
        r.fill_(SENTINEL)
        return r

    def check_dispatch(tag, o, recv, h):
        n = o.n[rank]
        got = recv.cpu()
        if not torch.equal(got[:n], o.recv[rank]):
            fail(f"{tag}: kept rows differ")
        if not torch.equal(got[n:], torch.full_like(got[n:], SENTINEL)):
            fail(f"{tag}: rows past the total or the sentinels were written")
        if h.expert_counts.cpu().tolist() != o.expert_counts[rank].tolist():
            fail(f"{tag}: expert_counts {h.expert_counts.tolist()} != {o.expert_counts[rank].tolist()}")
        if not torch.equal(h.row_of.cpu().long(), o.row_of[rank]):
            fail(f"{tag}: row_of differs")
        if h.num_dropped.cpu().tolist() != [o.dropped[rank]]:
            fail(f"{tag}: num_dropped {h.num_dropped.tolist()} != {o.dropped[rank]}")
        if o.Ce is not None:
            base, ec, totals = moe_layout(o.counts, rank, expert_capacity=o.Ce)
            kept = moe_kept(o.counts, o.Ce)
            if ec.tolist() != o.expert_counts[rank].tolist() or totals.tolist() != o.n:
                fail(f"{tag}: moe_layout disagrees with the oracle")
            if (o.counts - kept).sum(axis=1).tolist() != o.dropped:
                fail(f"{tag}: moe_kept disagrees with the oracle")
            for e in range(o.E):                       # the first kept row of this rank's segments
                m = (o.idxs[rank] == e) & o.kept_mask[rank]
                if m.any() and int(o.row_of[rank][m].min()) != int(base[rank, e]):
                    fail(f"{tag}: moe_layout base of expert {e} disagrees with the oracle")

    def run_case(name, int32_idx):
        o = Oracle(name, p)
        if name == "b":
            for what in case_b_conditions(o):
                fail(f"case b does not exercise what it should: {what}")
        x, idx, w, dout = (z[rank].to(D) for z in (o.xs, o.idxs, o.ws, o.douts))
        recv = new_buf(o, o.Ce)
        h = dev.moe_dispatch(x, idx.int() if int32_idx else idx, o.E, recv, expert_capacity=o.Ce)
        done()
        if h.expert_capacity != o.Ce:
            fail(f"dispatch[{name}]: the handle's expert_capacity is {h.expert_capacity}")
        check_dispatch(f"dispatch[{name}]", o, recv, h)
        n = o.n[rank]
        # weights=None, y = (local expert + 1) * row: bitwise against the fp32 slot-order sum
        ys = expert_scaled(o)
        y = dev.empty(tuple(recv.shape), o.dtype)
        y.fill_(SENTINEL)
        y[:n].copy_(ys[rank])
        out = dev.moe_combine(y, h)
        done()
        if not torch.equal(out.cpu(), o.combine(rank, ys).to(o.dtype)):
            fail(f"combine[{name}, weights=None]: not the fp32 slot-order sum")
        no_row = ~o.kept_mask[rank].any(dim=1)
        if no_row.any() and out.cpu()[no_row].abs().max().item() != 0:
            fail(f"combine[{name}]: a token without a kept slot is not zero")
        outw = dev.moe_combine(y, h, w)
        done()
        tol = TOL[o.dtype] * o.K
        want = o.combine(rank, ys, o.ws[rank], wide=True)
        if not torch.allclose(outw.cpu().double(), want, rtol=tol, atol=4 * tol):
            fail(f"combine[{name}, weighted]: max diff {(outw.cpu().double() - want).abs().max().item()}")
        # backward of the combine: kept dy rows bitwise, dweights of dropped slots exactly 0
        for weighted in (True, False):
            dy = dev.empty(tuple(recv.shape), o.dtype)
            dy.fill_(SENTINEL)
            dy, dw = dev.moe_combine_backward(dout, h, w if weighted else None, y=y if weighted else None, dy=dy)
            done()
            got = dy.cpu()
            if not torch.equal(got[:n], o.dy(rank, weighted)):
                fail(f"combine backward[{name}, weighted={weighted}]: kept dy rows differ")
            if not torch.equal(got[n:], torch.full_like(got[n:], SENTINEL)):
                fail(f"combine backward[{name}, weighted={weighted}]: dy rows past the total were written")
            if weighted:
                dw = dw.cpu()
                km = o.kept_mask[rank]
                if (~km).any() and dw[~km].abs().max().item() != 0:
                    fail(f"combine backward[{name}]: dweights of a dropped slot is not 0")
                dot = torch.zeros(km.shape, dtype=torch.float64)
                bound = torch.zeros(km.shape, dtype=torch.float64)
                for k in range(o.K):
                    for j in range(p):
                        m = km[:, k] & (o.idxs[rank][:, k].clamp(min=0) // o.El == j)
                        prod = o.douts[rank][m].double() * ys[j][o.row_of[rank][m, k]].double()
                        dot[m, k] = prod.sum(dim=1)
                        bound[m, k] = prod.abs().sum(dim=1)
                if not ((dw.double() - dot).abs() <= o.Dm * 2.0 ** -23 * bound).all():
                    fail(f"combine backward[{name}]: dweights of a kept slot is outside its bound")
        if name == "b":
            # the grouped GEMM over the kept rows, counts read on the device
            g = torch.Generator().manual_seed(4711)
            wts = torch.randn(o.El, 16, o.Dm, generator=g).bfloat16()
            res = ops.grouped_gemm_nt(recv, wts.to(D), h.expert_counts, out_dtype=torch.float32)
            done()
            want = torch.cat([o.recv[rank][o.elocal[rank] == el].float() @ wts[el].float().T for el in range(o.El)])
            if not torch.allclose(res.cpu()[:n], want, rtol=2e-3, atol=2e-3 * o.Dm ** 0.5):
                fail("grouped_gemm_nt over the kept rows differs from the per-expert loop")
        return o, x, idx, recv, h

    def same_as_no_capacity(o_b, x, idx):
        """Case e: a capacity no expert reaches is bit for bit the call without one."""
        Ce = int(o_b.col.max())
        o = Oracle("b", p, Ce=Ce)
        if sum(o.dropped):
            fail("case e: the oracle drops something")
        with_c, without = new_buf(o, Ce), new_buf(o, Ce)
        h1 = dev.moe_dispatch(x, idx, o.E, with_c, expert_capacity=Ce)
        h0 = dev.moe_dispatch(x, idx, o.E, without)
        done()
        check_dispatch("dispatch[e]", o, with_c, h1)
        if not (torch.equal(with_c, without) and torch.equal(h1.row_of, h0.row_of)
                and torch.equal(h1.expert_counts, h0.expert_counts)):
            fail("case e: differs from the call without expert_capacity")
        if h1.num_dropped.item() != 0 or h0.num_dropped.item() != 0 or h0.expert_capacity is not None:
            fail("case e: num_dropped is not 0")

    def graph():
        """dispatch + combine with expert_capacity captured once, replayed with new routing."""
        os_ = [Oracle("b", p, salt=s) for s in (0, 1, 2)]
        if len({tuple(o.dropped) for o in os_}) < 2:
            fail("graph: the replays drop the same numbers of entries")
        o0 = os_[0]
        x, idx, w = (z[rank].to(D).clone() for z in (o0.xs, o0.idxs, o0.ws))
        recv, y = new_buf(o0, o0.Ce), new_buf(o0, o0.Ce)
        out = torch.empty_like(x)
        cs = torch.cuda.Stream()
        cs.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(cs):
            with torch.cuda.graph(g, stream=cs):
                h = dev.moe_dispatch(x, idx, o0.E, recv, expert_capacity=o0.Ce)
                y.copy_(recv)
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
            check_dispatch(f"graph[{rep}]", o, recv, h)
            tol = TOL[o.dtype] * o.K
            want = o.combine(rank, o.recv, o.ws[rank], wide=True)
            if not torch.allclose(out.cpu().double(), want, rtol=tol, atol=4 * tol):
                fail(f"graph[{rep}]: combine max diff {(out.cpu().double() - want).abs().max().item()}")
        del g

    kept_b = None
    for n_, name in enumerate("abcd"):
        res = run_case(name, int32_idx=n_ % 2 == 1)
        if name == "b":
            kept_b = res
    same_as_no_capacity(kept_b[0], kept_b[1], kept_b[2])
    if dev.ranks_per_device <= 2:
        graph()
    torch.cuda.synchronize()
    dev.check()
    bad = comm.comm.allreduce(len(fails), op=MPI.SUM)
    if fails:
        print(f"[rank {rank}] " + "\n".join(fails[:20]), flush=True)
    if rank == 0:
        print(f"moe capacity OK ({time.time() - t0:.1f}s)" if bad == 0 else f"moe capacity FAILED ({bad})", flush=True)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
