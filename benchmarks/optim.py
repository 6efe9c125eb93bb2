"""The fused AdamW kernels (``ops.optim_sqsum``, ``ops.optim_adamw_update``, csrc/device/optim.hip)
on bf16 buckets of Llama-3-8B's parameters, against the eager composition and a yardstick.

    python benchmarks/optim.py                 # one layer (218 M parameters)
    python benchmarks/optim.py --full          # also 2 layers + embedding + head (1.49 G parameters)

One flat bf16 gradient bucket with one segment per parameter, fp32 ``p32``, ``m``, ``v``.  Timed:
``k_optim_sqsum`` alone and with the one-workgroup fp64 sum, ``k_optim_adamw`` with the clip
coefficient, and the whole step (norm, clip, update).  ``bytes`` is what the kernels MUST move, from the shapes: 2
bytes per element for the norm (the gradient, read once), 28 for the update (2 + 12 read, 12 + 2
written).  The eager composition on the same parameters: the gradients cast to fp32 into the
``.grad`` of fp32 master copies, ``clip_grad_norm_``, ``torch.optim.AdamW(fused=True)``, and the cast
back to bf16.  The yardstick: ``k_xent_backward`` (one read pass, one write pass of bf16) at T =
4096, V = 128256.  All paths alternate in one process; one sample = ``inner`` back-to-back calls
between two device events, ``inner`` chosen so that a sample lasts at least ``--window`` ms; median
and minimum over the rounds.

Prints one JSON line per record (``--session`` tags them; ``--out`` appends them to a file)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

from collective_communication_mpi_amd import ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--full", action="store_true", help="also the 2-layer full-vocabulary model")
ap.add_argument("--rounds", type=int, default=8)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--window", type=float, default=300.0, help="least duration of one sample, ms")
ap.add_argument("--session", type=int, default=None)
ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
args = ap.parse_args()
dev = torch.device("cuda")
D, FFN, KV, VOCAB = 4096, 14336, 1024, 128256
LAYER = [("attn_norm", D), ("wq", D * D), ("wk", KV * D), ("wv", KV * D), ("wo", D * D), ("mlp_norm", D),
         ("gate", FFN * D), ("up", FFN * D), ("down", D * FFN)]
BETAS, EPS, LR, WD = (0.9, 0.95), 1e-8, 3e-4, 0.1


def emit(rec):
    if args.session is not None:
        rec = {"session": args.session, **rec}
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


def sample(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / inner


def alternate(paths):
    """paths: name -> callable; every round times every path once.  name -> (median, min, inner)."""
    inner = {}
    for n, fn in paths.items():
        fn()
        inner[n] = max(1, int(args.window / max(sample(fn, 2), 1e-3)) + 1)
    ts = {n: [] for n in paths}
    for r in range(args.warmup + args.rounds):
        for n, fn in paths.items():
            t = sample(fn, inner[n])
            if r >= args.warmup:
                ts[n].append(t)
    return {n: (statistics.median(v), min(v), inner[n]) for n, v in ts.items()}


def stat(res, nbytes=None):
    rec = {"median_ms": round(res[0], 4), "min_ms": round(res[1], 4), "calls_per_sample": res[2]}
    if nbytes is not None:
        rec["bytes"] = nbytes
        rec["TBps_median"] = round(nbytes / res[0] / 1e9, 3)
    return rec


def bucket_bench(name, sizes):
    n, S = sum(sizes), len(sizes)
    g = torch.Generator(device=dev).manual_seed(11)
    params = [(torch.randn(s, device=dev, generator=g) * 0.02).bfloat16() for s in sizes]
    grad = torch.empty(n, dtype=torch.bfloat16, device=dev)
    for lo in range(0, n, 1 << 28):
        grad[lo:lo + (1 << 28)] = (torch.randn(min(1 << 28, n - lo), device=dev, generator=g) * 1e-2).bfloat16()
    off = [0]
    for s in sizes:
        off.append(off[-1] + s)
    seg_off = torch.tensor(off, dtype=torch.int64, device=dev)
    seg_ptr = torch.tensor([p.data_ptr() for p in params], dtype=torch.int64, device=dev)
    seg_flags = torch.tensor([ops.OPTIM_DECAY if s > D else 0 for s in sizes], dtype=torch.int32, device=dev)
    p32 = torch.cat([p.float() for p in params])
    m, v = torch.zeros_like(p32), torch.zeros_like(p32)
    partials = torch.empty(ops.optim_slots(n, S), dtype=torch.float32, device=dev)
    sums = torch.zeros(2, 2, dtype=torch.float64, device=dev)
    clip = torch.empty(2, dtype=torch.float32, device=dev)
    sched = ops.optim_sched(LR, BETAS, WD, 10).to(dev)

    def sqsum():
        ops.optim_sqsum(grad, seg_off, seg_flags, partials, None)

    def norm():
        ops.optim_sqsum(grad, seg_off, seg_flags, partials, sums, 0)

    def update():
        ops.optim_adamw_update(grad, seg_off, seg_ptr, seg_flags, p32, m, v, sched, clip, BETAS, EPS)

    def step():
        norm()
        ops.optim_clip(sums, 1.0, clip)
        update()

    step()
    # the eager composition on its own copies
    masters = [torch.nn.Parameter(p.float()) for p in params]
    for q in masters:
        q.grad = torch.empty_like(q)
    eager_opt = torch.optim.AdamW(masters, lr=LR, betas=BETAS, eps=EPS, weight_decay=WD, fused=True)
    views = [grad[lo:hi] for lo, hi in zip(off, off[1:])]

    def eager():
        torch._foreach_copy_([q.grad for q in masters], views)
        torch.nn.utils.clip_grad_norm_(masters, 1.0)
        eager_opt.step()
        torch._foreach_copy_(params, [q.detach() for q in masters])

    res = alternate({"k_optim_sqsum": sqsum, "k_optim_sqsum + k_optim_sums": norm, "k_optim_adamw": update,
                     "norm + clip + update": step,
                     "eager: cast, clip_grad_norm_, AdamW(fused=True), cast back": eager})
    rec = {"bench": "optim", "bucket": name, "parameters": n, "segments": S, "slots": ops.optim_slots(n, S),
           "rounds": args.rounds, "grad_norm": clip[0].item()}
    required = {"k_optim_sqsum": 2 * n, "k_optim_sqsum + k_optim_sums": 2 * n, "k_optim_adamw": 28 * n,
                "norm + clip + update": 30 * n}
    for k, r in res.items():
        rec[k] = stat(r, required.get(k))
    rec["eager / fused step (median)"] = round(res["eager: cast, clip_grad_norm_, AdamW(fused=True), cast back"][0]
                                               / res["norm + clip + update"][0], 2)
    emit(rec)


def yardstick():
    T, V = 4096, VOCAB
    g = torch.Generator(device=dev).manual_seed(7 + V)
    z = (torch.randn(T, V, device=dev, generator=g) * 2).bfloat16()
    tgt = torch.randint(0, V, (T,), device=dev, generator=g)
    stats = ops.cross_entropy_stats(z, tgt)
    lse, _, _, n_valid = ops.cross_entropy_combine(stats, tgt)
    one = torch.ones(1, device=dev)
    dl = torch.empty_like(z)
    res = alternate({"k": lambda: ops.cross_entropy_backward(z, tgt, lse, n_valid, one, 0, -100, dl)})
    emit({"bench": "yardstick k_xent_backward", "T": T, "V": V, **stat(res["k"], 4 * T * V)})


layer = [s for _, s in LAYER]
bucket_bench("one Llama-3-8B layer", layer)
torch.cuda.empty_cache()
yardstick()
if args.full:
    torch.cuda.empty_cache()
    bucket_bench("embedding, 2 layers, final norm, head", [VOCAB * D] + layer + layer + [D, VOCAB * D])
