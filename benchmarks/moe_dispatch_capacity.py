"""What the per-expert capacity costs the routed MoE dispatch when it drops nothing.

    scripts/mpirun -n 2 python benchmarks/moe_dispatch_capacity.py     # ranks sharing one GPU
    scripts/mpirun -n 8 python benchmarks/moe_dispatch_capacity.py

The routing of benchmarks/moe_dispatch.py (T tokens per rank, D = 7168 bf16, K = 8 out of
E = 32 p experts), ``moe_dispatch`` alone:

plain    no ``expert_capacity``: the path every existing caller takes.
capped   ``expert_capacity`` = the largest column total, so that nothing is dropped and the
         same rows move; the two results are first compared bit for bit.
Both use the same receive buffer of ``(E / p) * expert_capacity`` rows.

``--plain-only`` times the plain path alone and never names the new argument, and ``--tree``
imports the package from another checkout: together they time a commit from before the
capacity existed (built in a second tree) with this same file, launches of the two trees
alternating in one session (profiles/moe/README.md).

Interleaved rounds: one sample = ``--inner`` back-to-back dispatches, wall clock around a
device synchronise, the slowest rank counts; median and min-max.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--tokens", type=int, default=2048)
ap.add_argument("--dim", type=int, default=7168)
ap.add_argument("--topk", type=int, default=8)
ap.add_argument("--experts-per-rank", type=int, default=32)
ap.add_argument("--rounds", type=int, default=10)
ap.add_argument("--inner", type=int, default=5, help="dispatches per sample")
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--plain-only", action="store_true", help="time the call without expert_capacity only")
ap.add_argument("--tree", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."),
                help="import the package from this checkout")
ap.add_argument("--tag", default="", help="copied into the JSON line")
args = ap.parse_args()

sys.path.insert(0, os.path.abspath(args.tree))
import torch  # noqa: E402

from collective_communication_mpi_amd import MPI, Communicator  # noqa: E402

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

# set-up only: one host exchange of the histograms gives the largest column total
mine = torch.bincount(idx.reshape(-1).long(), minlength=E).cpu().tolist()
allc = hc.allgather(mine)
Ce = max(sum(allc[i][e] for i in range(p)) for e in range(E))
recv = dev.empty((El * Ce, Dm), dtype)


def plain():
    return dev.moe_dispatch(x, idx, E, recv)


def capped():
    return dev.moe_dispatch(x, idx, E, recv, expert_capacity=Ce)


paths = {"plain": plain} if args.plain_only else {"plain": plain, "capped": capped}

same = True
if not args.plain_only:
    h0 = plain()
    torch.cuda.synchronize()
    rows0 = recv.clone()
    recv.zero_()
    h1 = capped()
    torch.cuda.synchronize()
    dev.check()
    n = int(h0.expert_counts.sum())
    same = bool(torch.equal(rows0[:n], recv[:n]) and torch.equal(h0.row_of, h1.row_of)
                and torch.equal(h0.expert_counts, h1.expert_counts) and h1.num_dropped.item() == 0)
    del rows0
if not hc.allreduce(int(same), op=MPI.MIN):
    if rank == 0:
        print(json.dumps({"bench": "moe_dispatch_capacity", "ranks": p, "same": False}), flush=True)
    sys.exit(1)

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
    line = {"bench": "moe_dispatch_capacity", "tag": args.tag, "ranks": p, "shared_gpu": dev.shared_device,
            "same": True, "tokens_per_rank": T, "dim": Dm, "topk": K, "experts": E, "expert_capacity": Ce,
            "rounds": args.rounds, "dispatches_per_sample": args.inner, "results": res}
    if "capped" in res:
        line["capped_over_plain"] = round(res["capped"]["median_ms"] / res["plain"]["median_ms"], 4)
    print(json.dumps(line), flush=True)
