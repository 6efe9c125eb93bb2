"""Context-parallel attention (``parallel.context_parallel_attention``) on p ranks against the
single-rank ``ops.flash_attention`` on the whole sequence.

    scripts/mpirun -n 1 python benchmarks/context_parallel_attention.py
    scripts/mpirun -n 2 python benchmarks/context_parallel_attention.py
    scripts/mpirun -n 4 python benchmarks/context_parallel_attention.py

Shape: B = 2, total S = 8192 (S / p per rank), Hq / Hkv = 32 / 8, D = 128, causal; gaussian bf16.

single   ``ops.flash_attention`` on [B, S, H, D], timed on rank 0 while the other ranks wait.
cp       every rank at once on its shard: the k | v staging copy, the all-gather, the chunk kernel;
         "fwd+bwd" adds the second gather, the chunk backward and the reduce-scatter.
gather / reduce_scatter: the two collectives alone on the layer's own buffers.

One sample = ``--inner`` back-to-back calls between a host barrier and a device synchronise, timed
on every rank; per rank the median over the rounds, and the slowest rank.  Ranks that share one
GPU share its CUs and HBM: their kernels run beside or behind each other, so the table shows
overhead and imbalance, not scaling over links.  Rank 0 prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

from collective_communication_mpi_amd import MPI, Communicator, ops  # noqa: E402
from collective_communication_mpi_amd.parallel import context_parallel_attention  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=2)
ap.add_argument("--seq", type=int, default=8192, help="total sequence length")
ap.add_argument("--heads", type=int, default=32)
ap.add_argument("--kv-heads", type=int, default=8)
ap.add_argument("--dim", type=int, default=128)
ap.add_argument("--rounds", type=int, default=10)
ap.add_argument("--inner", type=int, default=3, help="calls per sample")
ap.add_argument("--warmup", type=int, default=2)
args = ap.parse_args()

comm = Communicator(MPI.COMM_WORLD)
rank, p = comm.Get_rank(), comm.Get_size()
dev = comm.dev
DEV = dev.device
B, S, Hq, Hkv, D = args.batch, args.seq, args.heads, args.kv_heads, args.dim
assert S % p == 0
S_loc = S // p

g = torch.Generator(device=DEV).manual_seed(1234)
q = torch.randn(B, S, Hq, D, generator=g, device=DEV).bfloat16()
k = torch.randn(B, S, Hkv, D, generator=g, device=DEV).bfloat16()
v = torch.randn(B, S, Hkv, D, generator=g, device=DEV).bfloat16()
dout = torch.randn(B, S, Hq, D, generator=g, device=DEV).bfloat16()
lo, hi = rank * S_loc, (rank + 1) * S_loc
qs, ks, vs = (t[:, lo:hi].contiguous().requires_grad_() for t in (q, k, v))
dos = dout[:, lo:hi].contiguous()
q.requires_grad_(), k.requires_grad_(), v.requires_grad_()


def single_fwd():
    with torch.no_grad():
        ops.flash_attention(q, k, v, causal=True)


def single_fwd_bwd():
    q.grad = k.grad = v.grad = None
    ops.flash_attention(q, k, v, causal=True).backward(dout)


def cp_fwd():
    with torch.no_grad():
        context_parallel_attention(comm, qs, ks, vs, causal=True)


def cp_fwd_bwd():
    qs.grad = ks.grad = vs.grad = None
    context_parallel_attention(comm, qs, ks, vs, causal=True).backward(dos)


shape = (B, S_loc, Hkv, D)
stage = dev.scratch_view("cp_stage", (2, *shape), torch.bfloat16)
gathered = dev.scratch_view("cp_gathered", (p, 2, *shape), torch.bfloat16)
partial = dev.scratch_view("cp_partial", (p, 2, *shape), torch.bfloat16)
dkv = torch.empty((2, *shape), dtype=torch.bfloat16, device=DEV)
partial.normal_()


def gather():
    dev.allgather(stage, gathered, algo="auto", symmetric=True)


def reduce_scatter():
    dev.reduce_scatter(partial, dkv, "SUM", symmetric=True)


def sample(fn):
    torch.cuda.synchronize()
    comm.comm.Barrier()
    t0 = time.perf_counter()
    for _ in range(args.inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / args.inner


collective = {"cp fwd": cp_fwd, "cp fwd+bwd": cp_fwd_bwd}
if p > 1:
    collective.update({"gather": gather, "reduce_scatter": reduce_scatter})
alone = {"single fwd": single_fwd, "single fwd+bwd": single_fwd_bwd}
times = {name: [] for name in (*collective, *alone)}
for r in range(args.warmup + args.rounds):
    for name, fn in collective.items():
        t = sample(fn)
        if r >= args.warmup:
            times[name].append(t)
    for name, fn in alone.items():  # rank 0 alone; the others wait at the next barrier
        if rank == 0:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.inner):
                fn()
            torch.cuda.synchronize()
            if r >= args.warmup:
                times[name].append((time.perf_counter() - t0) / args.inner)
        comm.comm.Barrier()
dev.check()

rec = {"bench": "context_parallel_attention", "ranks": p, "shared_gpu": bool(dev.shared_device), "B": B, "S": S,
       "S_loc": S_loc, "Hq": Hq, "Hkv": Hkv, "D": D, "causal": True, "rounds": args.rounds, "inner": args.inner}
for name in collective:
    med = comm.comm.allgather(statistics.median(times[name]))
    rec[name] = {"per_rank_median_ms": [round(x * 1e3, 3) for x in med], "slowest_ms": round(max(med) * 1e3, 3)}
if rank == 0:
    for name in alone:
        rec[name] = {"median_ms": round(statistics.median(times[name]) * 1e3, 3),
                     "min_ms": round(min(times[name]) * 1e3, 3)}
    print(json.dumps(rec), flush=True)
