"""Backward of the routed MoE collectives: the fused device-plane path against the path
composed from the primitives that existed before it.

    scripts/mpirun -n 2 python benchmarks/moe_backward.py      # ranks sharing one GPU
    scripts/mpirun -n 8 python benchmarks/moe_backward.py

Shape: that of benchmarks/moe_dispatch.py -- T tokens per rank, D = 7168 bf16, K = 8 experts
per token out of E = 32 p.  The forward (dispatch, y = the received rows, weights) runs once
as set-up; what the forward would save for its backward (the composed path's sort order,
counts and regroup permutation) is kept, so neither path pays for routing again.

fused     ``moe_combine_backward`` with ``dweights`` (one kernel: push w * dout into the
          owners' dy, pull the y rows for the dots) + the dispatch backward, the unweighted
          ``moe_combine`` of a [cap, D] gradient.
composed  combine backward: torch gather-scale-pack of T K rows -> ``alltoallv`` with device
          counts -> regroup to (expert, source) order; for dweights a second gathered copy of
          y (un-group, reverse ``alltoallv``) and a row-wise dot.  Dispatch backward:
          un-group the gradient, reverse ``alltoallv``, ``index_add_`` in fp32.
forward   the fused ``moe_dispatch`` + ``moe_combine`` pair, timed in the same rounds for the
          achieved bytes/s.

The results are first checked against each other (dy bitwise, dweights against the fp64
dot of the composed path's rows within D 2^-23 sum |dout y|, dx within bf16 tolerance), then
timed in interleaved rounds: wall clock around a device synchronise, the slowest rank counts.
Bytes moved per rank (rows read + rows written, 2 D bytes each): forward (2 K + 2) T,
backward (3 K + 2) T.  With several ranks on one GPU this measures HBM traffic + protocol,
not xGMI.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

from collective_communication_mpi_amd import MPI, Communicator  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--tokens", type=int, default=2048)
ap.add_argument("--dim", type=int, default=7168)
ap.add_argument("--topk", type=int, default=8)
ap.add_argument("--experts-per-rank", type=int, default=32)
ap.add_argument("--rounds", type=int, default=10)
ap.add_argument("--inner", type=int, default=3, help="calls per sample")
ap.add_argument("--warmup", type=int, default=2)
args = ap.parse_args()

comm = Communicator(MPI.COMM_WORLD)
rank, p = comm.Get_rank(), comm.Get_size()
dev, hc = comm.dev, comm.comm
Dv = dev.device
T, Dm, K, El = args.tokens, args.dim, args.topk, args.experts_per_rank
E = El * p
dtype = torch.bfloat16

g = torch.Generator(device=Dv).manual_seed(4242 + rank)
x = (torch.randn(T, Dm, generator=g, device=Dv) * 2).to(dtype)
idx = torch.rand(T, E, generator=g, device=Dv).topk(K, dim=1).indices.int()
w = torch.softmax(torch.randn(T, K, generator=g, device=Dv), dim=1)
dout = torch.randn(T, Dm, generator=g, device=Dv).to(dtype)

# capacity: what this rank receives (set-up only: one host exchange of the histograms)
mine = torch.bincount(idx.reshape(-1).long(), minlength=E).cpu().tolist()
allc = hc.allgather(mine)
n_recv = sum(allc[i][e] for i in range(p) for e in range(rank * El, (rank + 1) * El))
cap = max(hc.allgather(n_recv)) + 64

y = dev.empty((cap, Dm), dtype)                # the forward's y: the received rows
dy_f = dev.empty((cap, Dm), dtype)             # fused: gradient of y (doubles as the gradient of recv_x)
recv_c = dev.empty((cap, Dm), dtype)           # composed: rows in (source, expert) order
back_c = dev.empty((T * K, Dm), dtype)         # composed: rows returned to the source
hist_out = dev.empty((p, El), torch.int64)

# ---- the forward, once: the handle, and what the composed path would have saved ---------
h = dev.moe_dispatch(x, idx, E, y)
flat = idx.reshape(-1).long()
order = torch.argsort(flat, stable=True)
tok = order // K
hist = torch.bincount(flat, minlength=E).view(p, El)
cnt = hist.sum(dim=1) * Dm
rcnt = torch.empty(p, dtype=torch.int64, device=Dv)
dev.alltoallv(x[tok].view(-1), cnt, recv_c.view(-1), rcnt)
dev.alltoall(hist.view(-1), hist_out.view(-1))
seg = torch.searchsorted(torch.cumsum(hist_out.view(-1), 0), torch.arange(cap, device=Dv), right=True)
perm = torch.argsort(torch.where(seg < p * El, (seg % El) * p + seg // El, p * El), stable=True)
w_sorted = w.reshape(-1)[order][:, None]
torch.cuda.synchronize()
dev.check()
fwd_ok = torch.equal(recv_c[perm][:n_recv], y[:n_recv])     # both paths see the same rows in the same order
recv_f = dev.empty((cap, Dm), dtype)


def fused():
    dy, dw = dev.moe_combine_backward(dout, h, w, y=y, dy=dy_f)
    return dy, dw, dev.moe_combine(dy, h, None)


def composed():
    d = dout[tok]                                                     # gather: T K rows
    packed = (d.float() * w_sorted).to(dtype)                         # scale + pack
    dev.alltoallv(packed.view(-1), cnt, recv_c.view(-1), None)
    dy = recv_c[perm]                                                 # regroup: what the grouped GEMMs read
    recv_c[perm] = y                                                  # a second gathered copy of y, back at the source
    dev.alltoallv(recv_c.view(-1), rcnt, back_c.view(-1), None)
    dw = torch.empty(T * K, dtype=torch.float32, device=Dv)
    dw[order] = (back_c.float() * d.float()).sum(dim=1)
    recv_c[perm] = dy                                                 # dispatch backward: un-group, return, sum
    dev.alltoallv(recv_c.view(-1), rcnt, back_c.view(-1), None)
    dx = torch.zeros(T, Dm, dtype=torch.float32, device=Dv)
    dx.index_add_(0, tok, back_c.float())
    return dy, dw.view(T, K), dx.to(dtype)


def forward():
    hf = dev.moe_dispatch(x, idx, E, recv_f)
    return dev.moe_combine(recv_f, hf, w)


# ---- the two paths against each other ----------------------------------------------
ok, msg = fwd_ok, "" if fwd_ok else "the forward's rows differ between the paths"
try:
    if ok:
        dy1, dw1, dx1 = fused()
        torch.cuda.synchronize()
        dev.check()
        dy1 = dy1[:n_recv].clone()
        dy2, dw2, dx2 = composed()
        torch.cuda.synchronize()
        dev.check()
        # back_c holds the returned dy rows now; the y rows at the source for the fp64 dots:
        recv_c[perm] = y
        dev.alltoallv(recv_c.view(-1), rcnt, back_c.view(-1), None)
        prod = back_c.double() * dout[tok].double()
        dot64 = torch.empty(T * K, dtype=torch.float64, device=Dv)
        bound = torch.empty_like(dot64)
        dot64[order] = prod.sum(dim=1)
        bound[order] = Dm * 2.0 ** -23 * prod.abs().sum(dim=1)
        torch.cuda.synchronize()
        dev.check()
        if not torch.equal(dy1, dy2[:n_recv]):
            ok, msg = False, "dy differs from the composed path's"
        elif not bool(((dw1.reshape(-1).double() - dot64).abs() <= bound).all()):
            ok, msg = False, f"fused dweights off by {(dw1.reshape(-1).double() - dot64).abs().max().item()}"
        elif not bool(((dw2.reshape(-1).double() - dot64).abs() <= bound).all()):
            ok, msg = False, "composed dweights off"
        elif not torch.allclose(dx1.float(), dx2.float(), rtol=1e-2 * K, atol=4e-2 * K):
            ok, msg = False, f"dx differs: {(dx1.float() - dx2.float()).abs().max().item()}"
        del dy1, dy2, dw1, dw2, dx1, dx2, prod, dot64, bound
except Exception as e:  # noqa: BLE001
    ok, msg = False, str(e)
if not ok:
    print(f"# rank {rank}: {msg}", file=sys.stderr, flush=True)
if not hc.allreduce(int(ok), op=MPI.MIN):
    if rank == 0:
        print(json.dumps({"bench": "moe_backward", "ranks": p, "exact": False}), flush=True)
    sys.exit(1)

# ---- timing: interleaved rounds ----------------------------------------------------
paths = {"fused": fused, "composed": composed, "forward": forward}
for _ in range(args.warmup):
    for fn in paths.values():
        fn()
samples = {k: [] for k in paths}
for _ in range(args.rounds):
    for name, fn in paths.items():
        torch.cuda.synchronize()
        hc.Barrier()
        t0 = time.perf_counter()
        for _ in range(args.inner):
            fn()
        torch.cuda.synchronize()
        samples[name].append(hc.allreduce((time.perf_counter() - t0) / args.inner, op=MPI.MAX))
dev.check()
if rank == 0:
    res = {k: {"median_ms": round(statistics.median(v) * 1e3, 4), "min_ms": round(min(v) * 1e3, 4),
               "max_ms": round(max(v) * 1e3, 4)} for k, v in samples.items()}
    moved = {"fused": (3 * K + 2) * T * Dm * 2, "forward": (2 * K + 2) * T * Dm * 2}
    gbs = {k: round(moved[k] / (res[k]["median_ms"] * 1e-3) / 1e9, 1) for k in moved}
    print(json.dumps({"bench": "moe_backward", "ranks": p, "shared_gpu": dev.shared_device, "exact": True,
                      "tokens_per_rank": T, "dim": Dm, "topk": K, "experts": E, "dtype": "bf16",
                      "rounds": args.rounds, "calls_per_sample": args.inner,
                      "payload_bytes_per_rank": T * K * Dm * 2, "results": res,
                      "fused_over_composed": round(res["fused"]["median_ms"] / res["composed"]["median_ms"], 4),
                      "fused_outside_composed_spread": res["fused"]["median_ms"] < res["composed"]["min_ms"],
                      "bytes_moved_per_rank": moved, "gb_per_s_per_rank": gbs,
                      "gb_per_s_all_ranks": {k: round(v * p, 1) for k, v in gbs.items()}}), flush=True)
