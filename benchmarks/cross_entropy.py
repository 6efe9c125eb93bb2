"""The fused cross-entropy (``ops.cross_entropy``, csrc/device/xent.hip) against
``F.cross_entropy(logits.float(), tgt)``, what the Llama head used before it.

    python benchmarks/cross_entropy.py                 # the loss alone, one rank
    python benchmarks/cross_entropy.py --model         # a 2-layer full-vocabulary LlamaModel step, A/B
    python -m collective_communication_mpi_amd.launch -n 2 python benchmarks/cross_entropy.py --ranks

Loss alone: T = 4096 rows, V = 128256 (the benchmark's head) and V = 16032 (the TP = 8 shard's local
work); logits N(0, 2^2) in bf16, random targets.  "fwd" is the loss under no_grad; "fwd+bwd" goes
from the bf16 logits (a leaf) to their bf16 gradient.  The two paths alternate in one process; one
sample = ``--inner`` back-to-back calls between two device events; median and minimum over the
rounds.  ``peak_MB`` is the ``torch.cuda.max_memory_allocated`` delta of one call over what was
allocated before it (the logits themselves are not counted).  For each fused kernel alone: its
time and the bytes it MUST move (computed from the shapes: stats reads T V bf16; backward reads
and writes T V bf16; combine reads 16 P T bytes), as GB/s.

--model: ``LlamaModel`` (Llama-3-8B widths, 2 layers, vocabulary 128256, attention="flash"), 4096
tokens as 2 x 2048, one rank; the SAME weights with ``loss="torch"`` and ``loss="fused"``
alternating: step time (zero_grad + forward + backward) and peak memory of a step.

--ranks (under the launcher, ranks sharing one GPU): Vloc = 64128 per rank; the local forward
(stats + combine on the shard alone) against the collective forward (stats, all-gather, combine):
the difference is what the all-gather and its synchronisation cost when the ranks share a GPU.  It is
NOT an xGMI number.

Prints one JSON line per record."""
import argparse
import dataclasses
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from collective_communication_mpi_amd import ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--tokens", type=int, default=4096)
ap.add_argument("--vocabs", type=int, nargs="+", default=[128256, 16032])
ap.add_argument("--rounds", type=int, default=10)
ap.add_argument("--inner", type=int, default=5, help="calls per sample")
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--model", action="store_true")
ap.add_argument("--ranks", action="store_true")
args = ap.parse_args()
dev = torch.device("cuda")


def sample(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / inner


def peak_mb(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 1e6, 1)


def alternate(paths, rounds, warmup, inner):
    """paths: name -> callable; every round times every path once.  name -> (median, min) ms."""
    ts = {n: [] for n in paths}
    for r in range(warmup + rounds):
        for n, fn in paths.items():
            t = sample(fn, inner)
            if r >= warmup:
                ts[n].append(t)
    return {n: (statistics.median(v), min(v)) for n, v in ts.items()}


def stat(pair):
    return {"median_ms": round(pair[0], 4), "min_ms": round(pair[1], 4)}


def loss_alone(T, V):
    g = torch.Generator(device=dev).manual_seed(7 + V)
    logits = (torch.randn(T, V, device=dev, generator=g) * 2).bfloat16().requires_grad_()
    tgt = torch.randint(0, V, (T,), device=dev, generator=g)

    def torch_fwd():
        with torch.no_grad():
            return F.cross_entropy(logits.float(), tgt)

    def fused_fwd():
        with torch.no_grad():
            return ops.cross_entropy(logits, tgt)

    def torch_fb():
        logits.grad = None
        F.cross_entropy(logits.float(), tgt).backward()

    def fused_fb():
        logits.grad = None
        ops.cross_entropy(logits, tgt).backward()

    diff = abs(torch_fwd().item() - fused_fwd().item())
    rec = {"bench": "cross_entropy", "T": T, "V": V, "rounds": args.rounds, "inner": args.inner,
           "loss_abs_difference": diff, "row_splits": ops.xent_row_splits(T, V)}
    for kind, pair in (("fwd", {"torch": torch_fwd, "fused": fused_fwd}),
                       ("fwd+bwd", {"torch": torch_fb, "fused": fused_fb})):
        res = alternate(pair, args.rounds, args.warmup, args.inner)
        for name, fn in pair.items():
            rec[f"{name} {kind}"] = {**stat(res[name]), "peak_MB": peak_mb(fn)}
        rec[f"speedup {kind} (median)"] = round(res["torch"][0] / res["fused"][0], 2)
    # each fused kernel alone, with caller buffers
    z = logits.detach()
    stats = ops.cross_entropy_stats(z, tgt)
    lse, row_loss, loss_sum, n_valid = ops.cross_entropy_combine(stats, tgt)
    one = torch.ones(1, device=dev)
    dl = torch.empty_like(z)
    work = torch.empty(((T + ops.XENT_CHUNK - 1) // ops.XENT_CHUNK, 2), device=dev)

    def combine():
        return ops.cross_entropy_combine(stats, tgt, -100, lse, row_loss, loss_sum, n_valid, work=work)

    def backward():
        return ops.cross_entropy_backward(z, tgt, lse, n_valid, one, 0, -100, dl)

    kernels = {"k_xent_stats": (lambda: ops.cross_entropy_stats(z, tgt, 0, stats), 2 * T * V),
               "k_xent_combine + k_xent_sum": (combine, 16 * stats.shape[0] * T + 8 * T + 8 * T),
               "k_xent_backward": (backward, 4 * T * V)}
    res = alternate({n: f for n, (f, _) in kernels.items()}, args.rounds, args.warmup, 20)
    for n, (_, nbytes) in kernels.items():
        rec[n] = {**stat(res[n]), "bytes": nbytes, "GBps_median": round(nbytes / res[n][0] / 1e6, 1)}
    print(json.dumps(rec), flush=True)


def model_ab():
    from collective_communication_mpi_amd import MPI, Communicator
    from collective_communication_mpi_amd.parallel.llama_dp import LLAMA3_8B, LlamaModel, _self_comm

    comm = Communicator(MPI.COMM_WORLD)
    cfg = dataclasses.replace(LLAMA3_8B, layers=2, attention="flash")
    model = LlamaModel(cfg, _self_comm(comm), dev)
    gen = torch.Generator(device=dev).manual_seed(3)
    ids = torch.randint(0, cfg.vocab, (2, args.tokens // 2), device=dev, generator=gen)

    def step(kind):
        def run():
            model.cfg = dataclasses.replace(cfg, loss=kind)
            model.zero_grad()
            loss = model(ids)
            loss.backward()
            return loss
        return run

    losses = {k: step(k)().item() for k in ("torch", "fused")}
    res = alternate({k: step(k) for k in ("torch", "fused")}, args.rounds, args.warmup, 2)
    rec = {"bench": "cross_entropy model A/B", "model": "LlamaModel 2 layers, d 4096, vocab 128256, flash attention",
           "tokens": args.tokens, "rounds": args.rounds, "loss": losses}
    for k in ("torch", "fused"):
        rec[f"{k} step"] = {**stat(res[k]), "peak_MB": peak_mb(step(k))}
    rec["step saved ms (median)"] = round(res["torch"][0] - res["fused"][0], 3)
    rec["step saved share (median)"] = round(1 - res["fused"][0] / res["torch"][0], 4)
    print(json.dumps(rec), flush=True)


def ranks():
    from collective_communication_mpi_amd import MPI, Communicator
    from collective_communication_mpi_amd.parallel import vocab_parallel_cross_entropy_forward

    comm = Communicator(MPI.COMM_WORLD)
    p, rank = comm.Get_size(), comm.Get_rank()
    T, V = args.tokens, 64128
    g = torch.Generator(device=dev).manual_seed(11 + rank)
    z = (torch.randn(T, V, device=dev, generator=g) * 2).bfloat16()
    tgt = torch.randint(0, p * V, (T,), device=dev, generator=torch.Generator(device=dev).manual_seed(5))
    stats = torch.empty((ops.xent_row_splits(T, V), T, 4), device=dev)
    lse, row_loss = torch.empty(T, device=dev), torch.empty(T, device=dev)
    loss_sum, n_valid = torch.empty(1, device=dev), torch.empty(1, dtype=torch.int64, device=dev)

    def local():
        ops.cross_entropy_stats(z, tgt, rank * V, stats)
        ops.cross_entropy_combine(stats, tgt, -100, lse, row_loss, loss_sum, n_valid)

    def collective():
        vocab_parallel_cross_entropy_forward(comm, z, tgt, -100, lse, row_loss, loss_sum, n_valid)

    res = alternate({"local": local, "collective": collective}, args.rounds, args.warmup, args.inner)
    worst = {k: comm.comm.allreduce(v[0], op=MPI.MAX) for k, v in res.items()}
    if rank == 0:
        print(json.dumps({"bench": "cross_entropy vocab-parallel forward", "ranks": p,
                          "shared_gpu": comm.dev.shared_device, "T": T, "Vloc": V, "allgather_bytes_per_rank": 16 * stats.shape[0] * T,
                          "local stats+combine median_ms (max over ranks)": round(worst["local"], 4),
                          "collective forward median_ms (max over ranks)": round(worst["collective"], 4),
                          "all-gather overhead ms": round(worst["collective"] - worst["local"], 4)}), flush=True)
    torch.cuda.synchronize()
    comm.dev.check()


if args.ranks:
    ranks()
elif args.model:
    model_ab()
else:
    for V in args.vocabs:
        loss_alone(args.tokens, V)
        torch.cuda.empty_cache()
