"""The routed MoE layer's router on one rank: the fused gate (``ops.moe_gate``) against the
eager composition in ``RoutedMoE`` (gate="torch"), and the logits GEMM beside them.

    python benchmarks/moe_router.py

Shape: T = 16384 tokens, E = 256 experts, K = 8, d_model = 7168 (x bf16, router fp32).

logits       ``x.float() @ router.t()``: the fp32 copy of x plus the fp32 GEMM, which both
             gates take as their input.  Reported on its own so that fusing it into the gate
             can be judged from a number.
eager        softmax -> topk -> sum -> div on [T, E]: today's chain, no statistics.
eager+stats  the same plus prob_sum (a column sum) and expert_tokens (a scatter_add), what
             gate="torch" runs to provide ``aux_loss``.
fused        ``ops.moe_gate``: one kernel plus the partial reduction; always with statistics.
"fwd" is the forward alone under no_grad; "fwd+bwd" adds autograd through ``weights`` (and
through ``prob_sum`` where there are statistics) back to the logits, the small torch ops of
that loss included on every path; "fused bwd (raw)" is ``ops.moe_gate_backward`` alone.

Interleaved rounds: one sample = ``--inner`` back-to-back calls, wall clock around a device
synchronise; median and min-max over the rounds.  The fused gate is first checked against
the eager one (idx equal where the logits have no ties, weights within 1e-5).  Prints one
JSON line."""
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
ap.add_argument("--tokens", type=int, default=16384)
ap.add_argument("--experts", type=int, default=256)
ap.add_argument("--topk", type=int, default=8)
ap.add_argument("--dim", type=int, default=7168)
ap.add_argument("--rounds", type=int, default=10)
ap.add_argument("--inner", type=int, default=5, help="calls per sample")
ap.add_argument("--warmup", type=int, default=2)
args = ap.parse_args()

T, E, K, Dm = args.tokens, args.experts, args.topk, args.dim
D = torch.device("cuda")
g = torch.Generator(device=D).manual_seed(1234)
x = torch.randn(T, Dm, generator=g, device=D).bfloat16()
router = torch.randn(E, Dm, generator=g, device=D) / Dm ** 0.5
dw = torch.randn(T, K, generator=g, device=D)
dps = torch.randn(E, generator=g, device=D)
logits = (x.float() @ router.t()).contiguous()
leaf = logits.clone().requires_grad_()


def eager(lg, stats):
    probs = torch.softmax(lg, dim=-1)
    w, idx = probs.topk(K, dim=-1)
    w = w / w.sum(dim=-1, keepdim=True)
    if not stats:
        return w, idx, None, None
    tokens = torch.zeros(E, dtype=torch.int64, device=D)
    tokens.scatter_add_(0, idx.reshape(-1), torch.ones_like(idx.reshape(-1)))
    return w, idx, probs.sum(dim=0), tokens


def fwd_bwd(fn):
    w, _, ps, _ = fn(leaf)
    loss = (w * dw).sum() if ps is None else (w * dw).sum() + (ps * dps).sum()
    return torch.autograd.grad(loss, leaf)[0]


def no_grad(fn):
    def run():
        with torch.no_grad():
            return fn(logits)
    return run


paths = {
    "logits": lambda: x.float() @ router.t(),
    "eager fwd": no_grad(lambda lg: eager(lg, False)),
    "eager+stats fwd": no_grad(lambda lg: eager(lg, True)),
    "fused fwd": lambda: ops.moe_gate_forward(logits, K, True),
    "eager fwd+bwd": lambda: fwd_bwd(lambda lg: eager(lg, False)),
    "eager+stats fwd+bwd": lambda: fwd_bwd(lambda lg: eager(lg, True)),
    "fused fwd+bwd": lambda: fwd_bwd(lambda lg: ops.moe_gate(lg, K, True)),
    "fused bwd (raw)": lambda: ops.moe_gate_backward(logits, fused_idx, dw, dps, True),
}

# ---- agreement -----------------------------------------------------------------------
we, ie, pe, te = eager(logits, True)
wf, jf, pf, tf = ops.moe_gate_forward(logits, K, True)
fused_idx = jf
ge, gf = fwd_bwd(lambda lg: eager(lg, True)), fwd_bwd(lambda lg: ops.moe_gate(lg, K, True))
torch.cuda.synchronize()
srt = torch.sort(logits, dim=1, descending=True).values
untied = (srt[:, :K] != srt[:, 1:K + 1]).all(dim=1)
exact = bool(torch.equal(jf.long()[untied], ie[untied])
             and torch.equal(tf, torch.bincount(jf.reshape(-1).long(), minlength=E)))
close = bool(torch.allclose(wf[untied], we[untied], rtol=1e-5, atol=1e-7)
             and torch.allclose(pf, pe, rtol=1e-5, atol=1e-6)
             and torch.allclose(gf[untied], ge[untied], rtol=1e-4, atol=1e-6))
if not (exact and close):
    print(json.dumps({"bench": "moe_router", "agree": False, "idx": exact, "values": close}), flush=True)
    sys.exit(1)

# ---- timing: interleaved rounds --------------------------------------------------------
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
print(json.dumps({"bench": "moe_router", "agree": True, "tokens": T, "experts": E, "topk": K, "dim": Dm,
                  "rounds": args.rounds, "calls_per_sample": args.inner, "results": res,
                  "fused_over_eager_fwd": round(med["fused fwd"] / med["eager fwd"], 4),
                  "fused_over_eager_stats_fwd": round(med["fused fwd"] / med["eager+stats fwd"], 4),
                  "fused_over_eager_fwd_bwd": round(med["fused fwd+bwd"] / med["eager fwd+bwd"], 4),
                  "fused_over_eager_stats_fwd_bwd": round(med["fused fwd+bwd"] / med["eager+stats fwd+bwd"], 4),
                  "logits_over_fused_fwd": round(med["logits"] / med["fused fwd"], 2)}), flush=True)
