"""The backward side of the grouped expert block on one GPU, one rank: the K-major-B dX
kernel (ops.grouped_gemm_nn) and the SwiGLU gate in the gate|up epilogue
(ops.grouped_gemm_nt_swiglu) against the paths they replace, run in the same rounds.

    python benchmarks/grouped_gemm_bwd.py

Shape, count vectors and method of benchmarks/grouped_gemm.py: 16384 routed rows of
D = 7168 bf16 over G = 32 local experts of width 2048, balanced and skewed counts.

dx     nn            one ``grouped_gemm_nn`` launch on the weights as they lie
       transpose_nt  ``transpose`` of [G * N, K] + ``grouped_gemm_nt`` on the [G, K, N] view
       nt_ceiling    ``grouped_gemm_nt`` of the same FLOPs (forward): the tile's ceiling
       nt_on_copy    ``grouped_gemm_nt`` on a transposed copy made outside the timing: what the
                     NT loop takes on dX's own shape (reduction 2048, 7168 columns)
gate   fused         one ``grouped_gemm_nt_swiglu`` launch
       unfused       ``grouped_gemm_nt`` + ``swiglu_pairs`` over the whole buffer
block  GroupedExpertsMLP (d_model = D, d_ff = --dff) forward and forward + backward with
       CCMPI_GROUPED_DX / CCMPI_GROUPED_SWIGLU at nn / fused (new) and transpose / unfused (old),
       and the peak allocation of one backward above the level before it; the same peak for a
       ``grouped_linear`` backward on frozen weights (dX alone), where a copy of the weights shows

Results are checked against the old paths before timing.  Timing: interleaved rounds, one
sample = ``--inner`` back-to-back calls, wall clock around a device synchronise; median and
min-max over the rounds.  Prints one JSON line per count vector."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

from collective_communication_mpi_amd.ops import (  # noqa: E402
    grouped_gemm_nn,
    grouped_gemm_nt,
    grouped_gemm_nt_swiglu,
    grouped_linear,
    swiglu_pairs,
)
from collective_communication_mpi_amd.ops.kernels import _transposed_experts  # noqa: E402
from collective_communication_mpi_amd.parallel import GroupedExpertsMLP  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=16384)
ap.add_argument("--dim", type=int, default=7168)
ap.add_argument("--width", type=int, default=2048)
ap.add_argument("--dff", type=int, default=2048, help="d_ff of the GroupedExpertsMLP block")
ap.add_argument("--experts", type=int, default=32)
ap.add_argument("--rounds", type=int, default=10)
ap.add_argument("--inner", type=int, default=5, help="calls per sample")
ap.add_argument("--warmup", type=int, default=2)
args = ap.parse_args()
R, K, N, G = args.rows, args.dim, args.width, args.experts
dev = torch.device("cuda")


def count_vectors():
    bal = [R // G] * G
    bal[0] += R - sum(bal)
    wt = [0.0 if g % 5 == 4 else 1.0 / (g + 1) for g in range(G)]
    sk = [int(R * v / sum(wt)) for v in wt]
    sk[0] += R - sum(sk)
    return {"balanced": bal, "skewed": sk}


def routes(new: bool):
    os.environ["CCMPI_GROUPED_DX"] = "nn" if new else "transpose"
    os.environ["CCMPI_GROUPED_SWIGLU"] = "fused" if new else "unfused"


g = torch.Generator(device=dev).manual_seed(7)
x = torch.randn(R, K, generator=g, device=dev).bfloat16()
w = (torch.randn(G, N, K, generator=g, device=dev) / K ** 0.5).bfloat16()
dy = torch.randn(R, N, generator=g, device=dev).bfloat16()
dx = torch.empty(R, K, dtype=torch.bfloat16, device=dev)
dx_ref = torch.empty_like(dx)
h = torch.empty(R, N, dtype=torch.bfloat16, device=dev)
h_ref = torch.empty_like(h)
glu = torch.empty(R, N // 2, dtype=torch.bfloat16, device=dev)
glu_ref = torch.empty_like(glu)
wt_view = _transposed_experts(w)
mlp = GroupedExpertsMLP(G, K, args.dff, device=dev)
xg = x.clone().requires_grad_()
dyb = torch.randn(R, K, generator=g, device=dev).bfloat16()
flops = 2.0 * R * N * K


def stats(v):
    return {"median_ms": round(statistics.median(v) * 1e3, 4), "min_ms": round(min(v) * 1e3, 4),
            "max_ms": round(max(v) * 1e3, 4)}


def bench(counts_list):
    counts = torch.tensor(counts_list, dtype=torch.int64, device=dev)

    def nn():
        grouped_gemm_nn(dy, w, counts, out=dx)

    def transpose_nt(o=dx):
        grouped_gemm_nt(dy, _transposed_experts(w), counts, out=o)

    def nt_on_copy():
        grouped_gemm_nt(dy, wt_view, counts, out=dx)

    def nt_ceiling():
        grouped_gemm_nt(x, w, counts, out=h)

    def fused():
        grouped_gemm_nt_swiglu(x, w, counts, h=h, glu=glu)

    def unfused(ho=h, go=glu):
        grouped_gemm_nt(x, w, counts, out=ho)
        swiglu_pairs(ho, out=go)

    def block_fwd(new):
        routes(new)
        with torch.no_grad():
            return mlp(x, counts)

    def block_fwd_bwd(new):
        routes(new)
        xg.grad = None
        mlp.zero_grad(set_to_none=True)
        y = mlp(xg, counts)
        y.backward(dyb)
        return y

    def block_bwd_peak(new):
        routes(new)
        xg.grad = None
        mlp.zero_grad(set_to_none=True)
        y = mlp(xg, counts)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        y.backward(dyb)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - before

    def linear_dx_peak(new):
        # grouped_linear on frozen weights: the backward is dX alone, so a copy of the weights shows
        routes(new)
        xl = x.clone().requires_grad_()
        y = grouped_linear(xl, w, counts)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        y.backward(dy)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - before

    # ---- the new paths against the old ones ----
    nn()
    transpose_nt(dx_ref)
    fused()
    unfused(h_ref, glu_ref)
    torch.cuda.synchronize()
    dx_ok = torch.allclose(dx.float(), dx_ref.float(), rtol=2e-2, atol=8e-2)
    dx_bits = torch.equal(dx, dx_ref)
    gate_bits = torch.equal(h, h_ref) and torch.equal(glu, glu_ref)
    y_new = block_fwd_bwd(True)
    gx_new, gu_new, gd_new = xg.grad.clone(), mlp.gate_up.grad.clone(), mlp.down.grad.clone()
    y_old = block_fwd_bwd(False)
    torch.cuda.synchronize()
    block_ok = (torch.equal(y_new, y_old) and torch.equal(gd_new, mlp.down.grad)
                and torch.allclose(gx_new.float(), xg.grad.float(), rtol=2e-2, atol=8e-2)
                and torch.allclose(gu_new.float(), mlp.gate_up.grad.float(), rtol=2e-2, atol=8e-2))
    block_bits = torch.equal(gx_new, xg.grad) and torch.equal(gu_new, mlp.gate_up.grad)
    del y_new, y_old, gx_new, gu_new, gd_new
    peak = {"new": block_bwd_peak(True), "old": block_bwd_peak(False)}
    dx_peak = {"new": linear_dx_peak(True), "old": linear_dx_peak(False)}

    paths = {"nn": nn, "transpose_nt": transpose_nt, "nt_ceiling": nt_ceiling, "nt_on_copy": nt_on_copy,
             "fused": fused, "unfused": unfused,
             "block_fwd_new": lambda: block_fwd(True), "block_fwd_old": lambda: block_fwd(False),
             "block_fwd_bwd_new": lambda: block_fwd_bwd(True), "block_fwd_bwd_old": lambda: block_fwd_bwd(False)}
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
    res = {k: stats(v) for k, v in samples.items()}
    for k in ("nn", "transpose_nt", "nt_ceiling", "nt_on_copy", "fused", "unfused"):
        res[k]["tflops"] = round(flops / (res[k]["median_ms"] * 1e-3) / 1e12, 1)
    med = {k: v["median_ms"] for k, v in res.items()}
    spread = {k: round(v["max_ms"] - v["min_ms"], 4) for k, v in res.items()}
    return {"exact": bool(dx_ok and gate_bits and block_ok), "dx_bitwise": bool(dx_bits),
            "block_grads_bitwise": bool(block_bits), "max_count": max(counts_list),
            "results": res,
            "nn_over_transpose_nt": round(med["nn"] / med["transpose_nt"], 4),
            "nn_over_nt_ceiling": round(med["nn"] / med["nt_ceiling"], 4),
            "nn_over_nt_on_copy": round(med["nn"] / med["nt_on_copy"], 4),
            "nn_wins_by_more_than_spread": bool(med["transpose_nt"] - med["nn"] > max(spread["nn"], spread["transpose_nt"])),
            "fused_over_unfused": round(med["fused"] / med["unfused"], 4),
            "fused_not_slower_beyond_spread": bool(med["fused"] - med["unfused"] <= max(spread["fused"], spread["unfused"])),
            "block_fwd_new_over_old": round(med["block_fwd_new"] / med["block_fwd_old"], 4),
            "block_fwd_bwd_new_over_old": round(med["block_fwd_bwd_new"] / med["block_fwd_bwd_old"], 4),
            "block_bwd_peak_bytes": peak, "linear_dx_only_bwd_peak_bytes": dx_peak}


bad = False
for kind, cl in count_vectors().items():
    r = bench(cl)
    bad = bad or not r["exact"]
    print(json.dumps({"bench": "grouped_gemm_bwd", "counts": kind, "rows": R, "K": K, "N": N, "dff": args.dff,
                      "experts": G, "dtype": "bf16", "rounds": args.rounds, "calls_per_sample": args.inner, **r}),
          flush=True)
sys.exit(1 if bad else 0)
