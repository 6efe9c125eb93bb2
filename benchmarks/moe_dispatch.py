"""Routed MoE dispatch + weighted combine: the fused device-plane path against the
path composed from the primitives that existed before it.

    scripts/mpirun -n 2 python benchmarks/moe_dispatch.py      # ranks sharing one GPU
    scripts/mpirun -n 8 python benchmarks/moe_dispatch.py

Shape: T tokens per rank, D = 7168 bf16, K = 8 experts per token out of E = 32 p.

fused     ``moe_dispatch`` (route on the device, push each token once per slot into the
          owner's expert-grouped buffer) + ``moe_combine`` (pull, fp32 in slot order).
composed  torch stable argsort of the router's indices + gather-pack of T K rows ->
          ``alltoallv`` with device counts (plus an ``alltoall`` of the per-expert
          histograms, which the receiver needs to know what arrived) -> receiver
          regroup from (source, expert) to (expert, source) order -> the inverse
          permutation and a reverse ``alltoallv`` -> weighted ``index_add_``.  No host
          synchronisation either: every shape is fixed, counts stay on the device.

Both are first checked (the fused rows bitwise against the composed rows, the combined
output within bf16 tolerance), then timed in interleaved rounds: one sample is one
dispatch + combine pair, wall clock around a device synchronise, the slowest rank
counts.  With several ranks on one GPU this measures HBM traffic + protocol, not xGMI.
Prints one JSON line."""
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
ap.add_argument("--inner", type=int, default=3, help="pairs per sample")
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

# capacity: what this rank receives (set-up only: one host exchange of the histograms)
mine = torch.bincount(idx.reshape(-1).long(), minlength=E).cpu().tolist()
allc = hc.allgather(mine)
n_recv = sum(allc[i][e] for i in range(p) for e in range(rank * El, (rank + 1) * El))
cap = max(hc.allgather(n_recv)) + 64

recv_f = dev.empty((cap, Dm), dtype)           # fused: expert-grouped rows (doubles as y)
recv_c = dev.empty((cap, Dm), dtype)           # composed: rows in (source, expert) order
back_c = dev.empty((T * K, Dm), dtype)         # composed: rows returned to the source
hist_out = dev.empty((p, El), torch.int64)
arange_cap = torch.arange(cap, device=Dv)


def fused():
    h = dev.moe_dispatch(x, idx, E, recv_f)
    return h, dev.moe_combine(recv_f, h, w)


def composed():
    flat = idx.reshape(-1).long()
    order = torch.argsort(flat, stable=True)
    tok = order // K
    packed = x[tok]                                                   # pack: T K rows
    hist = torch.bincount(flat, minlength=E).view(p, El)
    cnt = hist.sum(dim=1) * Dm
    rcnt = torch.empty(p, dtype=torch.int64, device=Dv)
    dev.alltoallv(packed.view(-1), cnt, recv_c.view(-1), rcnt)
    dev.alltoall(hist.view(-1), hist_out.view(-1))                    # hist_out[i, l]: rows of source i for local expert l
    seg = torch.searchsorted(torch.cumsum(hist_out.view(-1), 0), arange_cap, right=True)   # i * El + l; p * El past the end
    key = torch.where(seg < p * El, (seg % El) * p + seg // El, p * El)                    # rows past the end sort last
    perm = torch.argsort(key, stable=True)                                                 # (expert, source) order
    grouped = recv_c[perm]                                            # regroup: what a grouped GEMM reads
    y = grouped                                                       # (the experts would run here)
    recv_c[perm] = y                                                  # back to arrival order
    dev.alltoallv(recv_c.view(-1), rcnt, back_c.view(-1), None)
    out = torch.zeros(T, Dm, dtype=torch.float32, device=Dv)
    out.index_add_(0, tok, back_c.float() * w.reshape(-1)[order][:, None])
    return grouped, out.to(dtype)


# ---- exactness -------------------------------------------------------------------
ok = True
msg = ""
try:
    h, out_f = fused()
    torch.cuda.synchronize()
    dev.check()
    rows_f = recv_f[:n_recv].clone()
    grouped, out_c = composed()
    torch.cuda.synchronize()
    dev.check()
    if int(h.expert_counts.sum()) != n_recv:
        ok, msg = False, "expert_counts"
    elif not torch.equal(rows_f, grouped[:n_recv]):
        ok, msg = False, "dispatched rows differ from the composed path's"
    elif not torch.allclose(out_f.float(), out_c.float(), rtol=1e-2 * K, atol=4e-2 * K):
        ok, msg = False, f"combine differs: {(out_f.float() - out_c.float()).abs().max().item()}"
    else:  # the fused output against fp64 of its own rows: sum_k w x[t] = x[t] sum_k w
        want = x.double() * w.double().sum(dim=1, keepdim=True)
        if not torch.allclose(out_f.double(), want, rtol=1e-2 * K, atol=4e-2 * K):
            ok, msg = False, "fused combine differs from fp64"
    del rows_f, grouped, out_c, out_f
except Exception as e:  # noqa: BLE001
    ok, msg = False, str(e)
if not ok:
    print(f"# rank {rank}: {msg}", file=sys.stderr, flush=True)
if not hc.allreduce(int(ok), op=MPI.MIN):
    if rank == 0:
        print(json.dumps({"bench": "moe_dispatch", "ranks": p, "exact": False}), flush=True)
    sys.exit(1)

# ---- timing: interleaved rounds ----------------------------------------------------
paths = {"fused": fused, "composed": composed}
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
    print(json.dumps({"bench": "moe_dispatch", "ranks": p, "shared_gpu": dev.shared_device, "exact": True,
                      "tokens_per_rank": T, "dim": Dm, "topk": K, "experts": E, "dtype": "bf16",
                      "rounds": args.rounds, "pairs_per_sample": args.inner,
                      "payload_bytes_per_rank": T * K * Dm * 2, "results": res,
                      "fused_over_composed": round(res["fused"]["median_ms"] / res["composed"]["median_ms"], 4)}),
          flush=True)
