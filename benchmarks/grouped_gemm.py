"""Grouped expert GEMM (ops.grouped_gemm_nt / grouped_gemm_tn) against what a user of
this library had before it, on one GPU, one rank.

    python benchmarks/grouped_gemm.py

Shape: the per-rank shape of benchmarks/moe_dispatch.py -- 16384 routed rows of D = 7168
bf16 over G = 32 local experts of width 2048 -- with balanced counts (512 rows each) and
skewed ones (Zipf-like, every fifth expert empty), the total equal to the buffer.

forward   grouped     one ``grouped_gemm_nt`` launch, counts read on the device
          loop        ``counts.tolist()`` (a host read, part of what is timed), then G
                      ``gemm_nt`` calls on slices
          loop_torch  the same loop with ``F.linear`` (hipBLASLt), its outputs left per expert
          dense       one ``gemm_nt`` of [rows, K] x [N, K]: the same FLOPs without groups
                      (``gemm_nt`` picks its large-tile kernel at this size)
          dense_128   the same call held to the 128 x 128 kernel the grouped one is built
                      from: the ceiling for this tile
wgrad     grouped_tn  one ``grouped_gemm_tn`` launch
          loop_tn     ``counts.tolist()``, then G ``gemm_tn`` calls (zeroing empty experts)

The grouped results are first checked against the loops.  Timing: interleaved rounds, one
sample = ``--inner`` back-to-back calls, wall clock around a device synchronise; median
and min-max over the rounds.  Prints one JSON line per count vector."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from collective_communication_mpi_amd import _native  # noqa: E402
from collective_communication_mpi_amd.ops import gemm_nt, gemm_tn, grouped_gemm_nt, grouped_gemm_tn  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=16384)
ap.add_argument("--dim", type=int, default=7168)
ap.add_argument("--width", type=int, default=2048)
ap.add_argument("--experts", type=int, default=32)
ap.add_argument("--rounds", type=int, default=10)
ap.add_argument("--inner", type=int, default=5, help="calls per sample")
ap.add_argument("--warmup", type=int, default=2)
args = ap.parse_args()
R, K, N, G = args.rows, args.dim, args.width, args.experts
dev = torch.device("cuda")
D = _native.device()


def count_vectors():
    bal = [R // G] * G
    bal[0] += R - sum(bal)
    wt = [0.0 if g % 5 == 4 else 1.0 / (g + 1) for g in range(G)]
    sk = [int(R * v / sum(wt)) for v in wt]
    sk[0] += R - sum(sk)
    return {"balanced": bal, "skewed": sk}


g = torch.Generator(device=dev).manual_seed(7)
x = torch.randn(R, K, generator=g, device=dev).bfloat16()
w = (torch.randn(G, N, K, generator=g, device=dev) / K ** 0.5).bfloat16()
dy = torch.randn(R, N, generator=g, device=dev).bfloat16()
out = torch.empty(R, N, dtype=torch.bfloat16, device=dev)
out_ref = torch.empty_like(out)
dw = torch.empty(G, N, K, dtype=torch.float32, device=dev)
dw_ref = torch.empty_like(dw)
flops = 2.0 * R * N * K


def bench(counts_list):
    counts = torch.tensor(counts_list, dtype=torch.int64, device=dev)

    def grouped():
        grouped_gemm_nt(x, w, counts, out=out)

    def loop(o=out):
        at = 0
        for e, c in enumerate(counts.tolist()):
            if c:
                gemm_nt(x[at:at + c], w[e], out=o[at:at + c])
            at += c

    def loop_torch():
        at = 0
        for e, c in enumerate(counts.tolist()):
            if c:
                F.linear(x[at:at + c], w[e])
            at += c

    def dense():
        gemm_nt(x, w[0], out=out)

    def dense_128():
        D.gemm_set_kernel(1)
        try:
            gemm_nt(x, w[0], out=out)
        finally:
            D.gemm_set_kernel(0)

    def grouped_tn():
        grouped_gemm_tn(dy, x, counts, out=dw)

    def loop_tn(o=dw):
        at = 0
        for e, c in enumerate(counts.tolist()):
            if c:
                gemm_tn(dy[at:at + c], x[at:at + c], out=o[e])
            else:
                o[e].zero_()
            at += c

    # ---- the grouped kernels against the loops ----
    grouped()
    loop(out_ref)
    grouped_tn()
    loop_tn(dw_ref)
    torch.cuda.synchronize()
    fwd_ok = torch.allclose(out.float(), out_ref.float(), rtol=2e-2, atol=8e-2)
    tn_ok = torch.allclose(dw, dw_ref, rtol=2e-3, atol=2e-3 * max(counts_list) ** 0.5)

    paths = {"grouped": grouped, "loop": loop, "loop_torch": loop_torch, "dense": dense, "dense_128": dense_128,
             "grouped_tn": grouped_tn, "loop_tn": loop_tn}
    for _ in range(args.warmup):
        for fn in paths.values():
            fn()
    samples = {k: [] for k in paths}
    for _ in range(args.rounds):
        for name, fn in paths.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.inner):
                fn()
            torch.cuda.synchronize()
            samples[name].append((time.perf_counter() - t0) / args.inner)
    res = {k: {"median_ms": round(statistics.median(v) * 1e3, 4), "min_ms": round(min(v) * 1e3, 4),
               "max_ms": round(max(v) * 1e3, 4), "tflops": round(flops / statistics.median(v) / 1e12, 1)}
           for k, v in samples.items()}
    med = {k: v["median_ms"] for k, v in res.items()}
    return {"exact": bool(fwd_ok and tn_ok), "max_count": max(counts_list), "empty_experts": counts_list.count(0),
            "results": res,
            "grouped_over_loop": round(med["grouped"] / med["loop"], 4),
            "grouped_over_loop_torch": round(med["grouped"] / med["loop_torch"], 4),
            "grouped_over_dense": round(med["grouped"] / med["dense"], 4),
            "grouped_over_dense_128": round(med["grouped"] / med["dense_128"], 4),
            "grouped_tn_over_loop_tn": round(med["grouped_tn"] / med["loop_tn"], 4)}


bad = False
for kind, cl in count_vectors().items():
    r = bench(cl)
    bad = bad or not r["exact"]
    print(json.dumps({"bench": "grouped_gemm", "counts": kind, "rows": R, "K": K, "N": N, "experts": G, "dtype": "bf16",
                      "rounds": args.rounds, "calls_per_sample": args.inner, **r}), flush=True)
sys.exit(1 if bad else 0)
