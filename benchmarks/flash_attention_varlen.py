"""Packed-sequence causal GQA attention (``ops.flash_attention_varlen``) against what a caller had
before it, on one rank.

    python benchmarks/flash_attention_varlen.py

Llama-3-8B head shape (Hq / Hkv = 32 / 8, D = 128, causal), T = 8192 tokens packed four ways:
1 x 8192, 4 x 2048, 64 x 128 and the ragged list ``RAGGED`` below.  q, k, v and dout are gaussian
bf16 (never zeros), the same tensors for every path.

varlen  one ``ops.flash_attention_varlen`` call on the [T, H, D] tensors; ``cu_seqlens`` stays on
        the device.
loop    one ``ops.flash_attention`` call per document on its rows as a [1, len, H, D] view, the
        outputs concatenated to the [T, Hq D] input of ``wo``; the lengths are read from the device
        tensor in every call (``cu_seqlens.tolist()``: the host synchronisation this path needs).
padded  one ``ops.flash_attention`` call on [n, max_len, H, D] tensors that hold each document
        zero-padded to the longest.  Only that call is timed: building the padded tensors and
        gathering the rows back is left out, in this path's favour.
self    for 1 x 8192 only: ``ops.flash_attention`` on the [1, T, H, D] views, the same work.
"fwd" is the forward alone under no_grad; "fwd+bwd" adds autograd back to q, k and v.

Interleaved rounds in one process: one sample = ``--inner`` back-to-back calls, wall clock
around a device synchronise; median and minimum over the rounds.  TFLOP/s count the causal
forward of the documents, sum of 4 Hq len^2 D / 2, and 2.5 x that for the backward, for every path
(padding is not credited).  The varlen output is first compared with the loop's (they are equal
bit for bit).  Prints one JSON line per packing."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

from collective_communication_mpi_amd import ops  # noqa: E402

RAGGED = [3000, 37, 1024, 513, 64, 1, 2049, 129, 700, 675]

ap = argparse.ArgumentParser()
ap.add_argument("--tokens", type=int, default=8192)
ap.add_argument("--heads", type=int, default=32)
ap.add_argument("--kv-heads", type=int, default=8)
ap.add_argument("--dim", type=int, default=128)
ap.add_argument("--rounds", type=int, default=10)
ap.add_argument("--inner", type=int, default=3, help="calls per sample")
ap.add_argument("--warmup", type=int, default=2)
args = ap.parse_args()

T, Hq, Hkv, D = args.tokens, args.heads, args.kv_heads, args.dim
dev = torch.device("cuda")
PACKINGS = {"1 x T": [T], "4 x T/4": [T // 4] * 4, "64 x T/64": [T // 64] * 64}
if T == sum(RAGGED):
    PACKINGS["ragged"] = RAGGED


def sample(fn, inner):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / inner


g = torch.Generator(device=dev).manual_seed(1234 + T)
q = torch.randn(T, Hq, D, generator=g, device=dev).bfloat16().requires_grad_()
k = torch.randn(T, Hkv, D, generator=g, device=dev).bfloat16().requires_grad_()
v = torch.randn(T, Hkv, D, generator=g, device=dev).bfloat16().requires_grad_()
dout = torch.randn(T, Hq * D, generator=g, device=dev).bfloat16()

for label, lengths in PACKINGS.items():
    assert sum(lengths) == T
    n, longest = len(lengths), max(lengths)
    bounds = [0]
    for ln in lengths:
        bounds.append(bounds[-1] + ln)
    cu = torch.tensor(bounds, dtype=torch.int32, device=dev)
    # the padded path's operands, built once outside the timed region
    pads = []
    for t in (q, k, v):
        p = torch.zeros(n, longest, *t.shape[1:], dtype=t.dtype, device=dev)
        for i, (b, e) in enumerate(zip(bounds[:-1], bounds[1:])):
            p[i, :e - b] = t.detach()[b:e]
        pads.append(p.requires_grad_())
    dpad = torch.zeros(n, longest, Hq * D, dtype=dout.dtype, device=dev)
    for i, (b, e) in enumerate(zip(bounds[:-1], bounds[1:])):
        dpad[i, :e - b] = dout[b:e]

    def varlen_path():
        return ops.flash_attention_varlen(q, k, v, cu, causal=True).view(T, Hq * D), dout

    def loop_path():
        at = cu.tolist()  # the host read of the lengths
        outs = [ops.flash_attention(q[b:e].unsqueeze(0), k[b:e].unsqueeze(0), v[b:e].unsqueeze(0), causal=True)
                for b, e in zip(at[:-1], at[1:]) if e > b]
        return torch.cat(outs, dim=1).view(T, Hq * D), dout

    def padded_path():
        return ops.flash_attention(*pads, causal=True).view(n, longest, Hq * D), dpad

    def self_path():
        return ops.flash_attention(q.unsqueeze(0), k.unsqueeze(0), v.unsqueeze(0), causal=True).view(T, Hq * D), dout

    paths = {"varlen": varlen_path, "loop": loop_path, "padded": padded_path}
    if n == 1:
        paths["self"] = self_path

    def fwd(name):
        with torch.no_grad():
            return paths[name]()[0]

    def fwd_bwd(name):
        for t in (q, k, v, *pads):
            t.grad = None
        out, grad = paths[name]()
        out.backward(grad)

    same = torch.equal(fwd("varlen"), fwd("loop"))
    times = {(name, kind): [] for name in paths for kind in ("fwd", "fwd+bwd")}
    calls = {"fwd": fwd, "fwd+bwd": fwd_bwd}
    for r in range(args.warmup + args.rounds):
        for kind in ("fwd", "fwd+bwd"):
            for name in paths:  # interleaved: every round times every path once
                t = sample(lambda: calls[kind](name), args.inner)
                if r >= args.warmup:
                    times[(name, kind)].append(t)
    flops = {"fwd": sum(4 * Hq * ln * ln * D / 2 for ln in lengths)}
    flops["fwd+bwd"] = flops["fwd"] * 3.5
    rec = {"bench": "flash_attention_varlen", "packing": label, "T": T, "n": n, "longest": longest, "Hq": Hq, "Hkv": Hkv,
           "D": D, "causal": True, "rounds": args.rounds, "inner": args.inner, "varlen_equals_loop_bitwise": same}
    for (name, kind), ts in times.items():
        med, best = statistics.median(ts), min(ts)
        rec[f"{name} {kind}"] = {"median_ms": round(med * 1e3, 3), "min_ms": round(best * 1e3, 3),
                                 "TFLOPs_median": round(flops[kind] / med / 1e12, 1)}
    print(json.dumps(rec), flush=True)
    for t in (q, k, v):
        t.grad = None
    del pads, dpad
    torch.cuda.empty_cache()
