"""Causal GQA attention of the Llama-3-8B-shaped block on one rank: ``ops.flash_attention``
against the path ``LlamaBlock`` runs with ``attention="sdpa"``.

    python benchmarks/flash_attention.py

Shapes: B = 2, S in {2048, 8192}, Hq / Hkv = 32 / 8, D = 128, causal; q, k, v and dout are
gaussian bf16 (never zeros), the same tensors for both paths.

sdpa    q, k, v [B, S, H, D] transposed to [B, H, S, D], the kv heads expanded to Hq with
        ``repeat_interleave``, ``F.scaled_dot_product_attention(is_causal=True)``, the output
        transposed back and made contiguous (the input of ``wo``).
flash   ``ops.flash_attention`` on the [B, S, H, D] tensors as they are.
"fwd" is the forward alone under no_grad; "fwd+bwd" adds autograd back to q, k and v (the
gradient of the expansion, a sum over each group's heads, is part of the sdpa path).

Interleaved rounds in one process: one sample = ``--inner`` back-to-back calls, wall clock
around a device synchronise; median and minimum over the rounds.  TFLOP/s count
4 B Hq S^2 D / 2 for the causal forward and 2.5 x that for the backward (five products; the
flash backward executes seven, which is not credited).  Peak memory is the allocator's peak
above the inputs during one fwd+bwd call.  The two paths are first compared (outputs and
gradients, largest absolute difference).  Prints one JSON line per shape."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from collective_communication_mpi_amd import ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=2)
ap.add_argument("--seqs", type=int, nargs="+", default=[2048, 8192])
ap.add_argument("--heads", type=int, default=32)
ap.add_argument("--kv-heads", type=int, default=8)
ap.add_argument("--dim", type=int, default=128)
ap.add_argument("--rounds", type=int, default=10)
ap.add_argument("--inner", type=int, default=3, help="calls per sample")
ap.add_argument("--warmup", type=int, default=2)
args = ap.parse_args()

B, Hq, Hkv, D = args.batch, args.heads, args.kv_heads, args.dim
dev = torch.device("cuda")


def sdpa_path(q, k, v):
    rep = Hq // Hkv
    qt, kt, vt = q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2)
    if rep > 1:
        kt, vt = kt.repeat_interleave(rep, dim=1), vt.repeat_interleave(rep, dim=1)
    o = F.scaled_dot_product_attention(qt, kt, vt, is_causal=True)
    return o.transpose(1, 2).reshape(q.shape[0], q.shape[1], Hq * D)


def flash_path(q, k, v):
    return ops.flash_attention(q, k, v, causal=True).view(q.shape[0], q.shape[1], Hq * D)


def sample(fn, inner):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / inner


for S in args.seqs:
    g = torch.Generator(device=dev).manual_seed(1234 + S)
    q = torch.randn(B, S, Hq, D, generator=g, device=dev).bfloat16().requires_grad_()
    k = torch.randn(B, S, Hkv, D, generator=g, device=dev).bfloat16().requires_grad_()
    v = torch.randn(B, S, Hkv, D, generator=g, device=dev).bfloat16().requires_grad_()
    dout = torch.randn(B, S, Hq * D, generator=g, device=dev).bfloat16()
    paths = {"sdpa": sdpa_path, "flash": flash_path}

    def fwd(name):
        with torch.no_grad():
            return paths[name](q, k, v)

    def fwd_bwd(name):
        q.grad = k.grad = v.grad = None
        paths[name](q, k, v).backward(dout)
        return q.grad, k.grad, v.grad

    # agreement of the two paths, and the peak memory of one fwd+bwd call of each
    results, peak = {}, {}
    for name in paths:
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fwd(name)
        grads = fwd_bwd(name)
        torch.cuda.synchronize()
        peak[name] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
        results[name] = (out.float(), *(t.float().clone() for t in grads))
        del out, grads
    diff = {n: (a - b).abs().max().item() for n, a, b in zip(("out", "dq", "dk", "dv"), results["sdpa"], results["flash"])}
    del results
    q.grad = k.grad = v.grad = None

    times = {(name, kind): [] for name in paths for kind in ("fwd", "fwd+bwd")}
    calls = {"fwd": fwd, "fwd+bwd": fwd_bwd}
    for r in range(args.warmup + args.rounds):
        for kind in ("fwd", "fwd+bwd"):
            for name in paths:  # interleaved: every round times every path once
                t = sample(lambda: calls[kind](name), args.inner)
                if r >= args.warmup:
                    times[(name, kind)].append(t)
    flops = {"fwd": 4 * B * Hq * S * S * D / 2}
    flops["fwd+bwd"] = flops["fwd"] * 3.5
    rec = {"bench": "flash_attention", "B": B, "S": S, "Hq": Hq, "Hkv": Hkv, "D": D, "causal": True,
           "rounds": args.rounds, "inner": args.inner, "max_abs_diff_vs_sdpa": {n: round(x, 5) for n, x in diff.items()}}
    for (name, kind), ts in times.items():
        med, best = statistics.median(ts), min(ts)
        rec[f"{name} {kind}"] = {"median_ms": round(med * 1e3, 3), "min_ms": round(best * 1e3, 3),
                                 "TFLOPs_median": round(flops[kind] / med / 1e12, 1),
                                 "TFLOPs_best": round(flops[kind] / best / 1e12, 1)}
    for name in paths:
        rec[f"{name} peak_MiB"] = round(peak[name], 1)
    print(json.dumps(rec), flush=True)
    del q, k, v, dout
    torch.cuda.empty_cache()
