"""The router logits of the routed MoE layer on one rank: ``ops.moe_router_logits`` (the fp32
router as three bf16 planes on the matrix cores, csrc/device/moe_router.hip) against
``x.float() @ router.t()``, what ``RoutedMoE(router_logits="torch")`` runs.

    python benchmarks/moe_router_logits.py [--out profiles/moe/moe_router_logits.json]

Shapes: T = 16384 and T = 4096 tokens, E = 256 experts, d_model = 7168 (x bf16, router fp32):
the shape and the sampling scheme of benchmarks/moe_router.py.

torch fwd        ``x.float() @ router.t()`` under no_grad: the fp32 copy of x plus the fp32 GEMM.
composed fwd     three ``ops.gemm_nt(x, plane, accumulate=True, splitk=1)`` calls on planes split
                 beforehand: the same arithmetic from existing kernels, x read three times.  It
                 exists here only, as the comparison the new kernel has to beat.
split            ``ops.split_bf16x3(router)`` alone.
mfma fwd         ``ops.moe_router_logits_forward`` with ``planes`` and ``out`` given: the kernel.
mfma fwd+split   the same with the split inside, what one forward of the layer runs.
mfma fwd, N rows the kernel with its row tile forced to N rows per workgroup ("mfma fwd" takes the
                 largest that gives every CU a workgroup; the bits are the same).
torch bwd        ``(dlogits @ router).bfloat16()`` and ``dlogits.t() @ x.float()`` with the fp32
                 copy made beforehand: what autograd runs for the torch form.
mfma bwd         ``ops.moe_router_logits_backward``.
torch fwd+bwd / mfma fwd+bwd   through autograd, gradients for x and the router.
"peak bytes" is the rise of ``torch.cuda.max_memory_allocated`` over one forward + backward
through autograd above what was allocated before it.

Interleaved rounds: one sample = ``--inner`` back-to-back calls, wall clock around a device
synchronise; median and min-max over the rounds.  The three forwards are first checked against
the fp64 product.  Prints one JSON line per shape and writes the list of them to ``--out``."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

from collective_communication_mpi_amd import ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--tokens", type=int, nargs="+", default=[16384, 4096])
ap.add_argument("--experts", type=int, default=256)
ap.add_argument("--topk", type=int, default=8)
ap.add_argument("--dim", type=int, default=7168)
ap.add_argument("--rounds", type=int, default=10)
ap.add_argument("--inner", type=int, default=5, help="calls per sample")
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "moe",
                                              "moe_router_logits.json"))
args = ap.parse_args()
D = torch.device("cuda")


def run(T, E, K, Dm):
    g = torch.Generator(device=D).manual_seed(1234)
    x = torch.randn(T, Dm, generator=g, device=D).bfloat16()
    router = torch.randn(E, Dm, generator=g, device=D) / Dm ** 0.5
    dl = 1e-2 * torch.randn(T, E, generator=g, device=D)
    planes = ops.split_bf16x3(router)
    out = torch.empty(T, E, device=D)
    out_c = torch.empty(T, E, device=D)
    xf = x.float()
    xg, rg = x.clone().requires_grad_(), router.clone().requires_grad_()

    def composed():
        ops.gemm_nt(x, planes[2], out=out_c, splitk=1)
        ops.gemm_nt(x, planes[1], out=out_c, accumulate=True, splitk=1)
        return ops.gemm_nt(x, planes[0], out=out_c, accumulate=True, splitk=1)

    def torch_fwd():
        with torch.no_grad():
            return x.float() @ router.t()

    def torch_fb():
        return torch.autograd.grad(xg.float() @ rg.t(), (xg, rg), dl)

    def mfma_fb():
        return torch.autograd.grad(ops.moe_router_logits(xg, rg), (xg, rg), dl)

    paths = {
        "torch fwd": torch_fwd,
        "composed fwd": composed,
        "split": lambda: ops.split_bf16x3(router),
        "mfma fwd": lambda: ops.moe_router_logits_forward(x, router, planes=planes, out=out),
        "mfma fwd+split": lambda: ops.moe_router_logits_forward(x, router),
        "mfma fwd, 128 rows": lambda: ops.moe_router_logits_forward(x, router, planes=planes, out=out, row_tile=128),
        "mfma fwd, 64 rows": lambda: ops.moe_router_logits_forward(x, router, planes=planes, out=out, row_tile=64),
        "mfma fwd, 32 rows": lambda: ops.moe_router_logits_forward(x, router, planes=planes, out=out, row_tile=32),
        "torch bwd": lambda: ((dl @ router).bfloat16(), dl.t() @ xf),
        "mfma bwd": lambda: ops.moe_router_logits_backward(dl, x, planes),
        "torch fwd+bwd": torch_fb,
        "mfma fwd+bwd": mfma_fb,
    }

    # ---- agreement with fp64 ---------------------------------------------------------------
    ref = x.double() @ router.double().t()
    err = {"torch": (torch_fwd().double() - ref).abs().max().item(),
           "composed": (composed().double() - ref).abs().max().item(),
           "mfma": (paths["mfma fwd"]().double() - ref).abs().max().item()}
    dx64, dr64 = dl.double() @ router.double(), dl.double().t() @ x.double()
    tb, mb = paths["torch bwd"](), paths["mfma bwd"]()
    err.update({"torch dx": (tb[0].double() - dx64).abs().max().item(), "mfma dx": (mb[0].double() - dx64).abs().max().item(),
                "torch drouter": (tb[1].double() - dr64).abs().max().item(),
                "mfma drouter": (mb[1].double() - dr64).abs().max().item()})
    del ref, dx64, dr64, tb, mb
    torch.cuda.synchronize()
    if not (err["mfma"] <= 8 * err["torch"] and err["mfma drouter"] <= 8 * err["torch drouter"]
            and err["mfma dx"] <= 8 * err["torch dx"]):
        print(json.dumps({"bench": "moe_router_logits", "agree": False, "tokens": T, "max_abs_error": err}), flush=True)
        sys.exit(1)

    # ---- memory: one forward + backward through autograd ------------------------------------
    peak = {}
    for name, fn in (("torch", torch_fb), ("mfma", mfma_fb)):
        fn()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        peak[name] = torch.cuda.max_memory_allocated() - base

    # ---- timing: interleaved rounds ----------------------------------------------------------
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
               "max_ms": round(max(v) * 1e3, 4)} for k, v in samples.items()}
    med = {k: v["median_ms"] for k, v in res.items()}
    rec = {"bench": "moe_router_logits", "agree": True, "tokens": T, "experts": E, "topk": K, "dim": Dm,
           "rounds": args.rounds, "calls_per_sample": args.inner, "results": res,
           "max_abs_error_vs_fp64": {k: float(f"{v:.3e}") for k, v in err.items()},
           "peak_bytes_fwd_bwd": peak,
           "mfma_over_torch_fwd": round(med["mfma fwd+split"] / med["torch fwd"], 4),
           "mfma_over_composed_fwd": round(med["mfma fwd"] / med["composed fwd"], 4),
           "mfma_over_torch_bwd": round(med["mfma bwd"] / med["torch bwd"], 4),
           "mfma_over_torch_fwd_bwd": round(med["mfma fwd+bwd"] / med["torch fwd+bwd"], 4)}
    print(json.dumps(rec), flush=True)
    return rec


records = [run(T, args.experts, args.topk, args.dim) for T in args.tokens]
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(records, f, indent=1)
    f.write("\n")
