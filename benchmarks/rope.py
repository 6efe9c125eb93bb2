"""Rotary position embedding (``ops.rope_apply``, csrc/device/rope.hip) against the eager torch
composition a user would otherwise write.

    python benchmarks/rope.py                 # the op alone
    python benchmarks/rope.py --model         # a 2-layer rope=True LlamaModel step, A/B

The op alone, at the Llama-3-8B shape (T = 8192 tokens as [1, T, H, D], Hq = 32, Hkv = 8, D = 128)
and at ``--big`` times as many tokens (a working set beyond the 256 MiB Infinity Cache):
``rope_apply`` out of place and in place, the packed mode with one document and with 64, and
"eager": gather cos / sin by position, ``rotate_half``, two multiplies and an add, in bf16 on q and
on k (the Hugging Face form).  All paths alternate in one process; one sample = ``--inner``
back-to-back calls between two device events; median and minimum over the rounds.  ``bytes`` is
what the kernel MUST move, from the shapes: q and k read once and written once, the table rows
read once (the kernel reads a token's table row once per head lane, from cache: the GB/s figure
counts it once and so slightly understates the traffic).  ``lanes`` sweeps the kernel's head lanes per token (0 = its own choice).

The yardstick: ``k_xent_backward`` (one read pass, one write pass of bf16), timed in the same
process at T = 4096 and V = 16032 / 128256.

--model: ``LlamaModel`` (Llama-3-8B widths, 2 layers, vocabulary 128256, attention="flash",
loss="fused"), 4096 tokens as 2 x 2048, one rank; the SAME weights with rope=False, rope=True and
rope=True with the eager composition in place of ``ops.rope`` alternating: step time
(zero_grad + forward + backward).

Prints one JSON line per record."""
import argparse
import dataclasses
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

from collective_communication_mpi_amd import ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--tokens", type=int, default=8192)
ap.add_argument("--big", type=int, default=4, help="also run at this multiple of --tokens")
ap.add_argument("--heads", type=int, nargs=2, default=[32, 8])
ap.add_argument("--dim", type=int, default=128)
ap.add_argument("--rounds", type=int, default=20)
ap.add_argument("--inner", type=int, default=20, help="calls per sample")
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--model", action="store_true")
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


def alternate(paths, rounds, warmup, inner):
    """paths: name -> callable; every round times every path once.  name -> (median, min) ms."""
    ts = {n: [] for n in paths}
    for r in range(warmup + rounds):
        for n, fn in paths.items():
            t = sample(fn, inner)
            if r >= warmup:
                ts[n].append(t)
    return {n: (statistics.median(v), min(v)) for n, v in ts.items()}


def stat(pair, nbytes=None):
    rec = {"median_ms": round(pair[0], 4), "min_ms": round(pair[1], 4)}
    if nbytes is not None:
        rec["GBps_median"] = round(nbytes / pair[0] / 1e6, 1)
    return rec


def rotate_half(x):
    h = x.shape[-1] // 2
    return torch.cat((-x[..., h:], x[..., :h]), dim=-1)


def eager_rope(q, k, table, pos0=0, cu_seqlens=None, interleaved=False):
    """What a user writes without the kernel (half-split, batched): bf16 throughout, autograd-able."""
    assert cu_seqlens is None and not interleaved
    pos = torch.arange(pos0, pos0 + q.shape[1], device=q.device)
    rows = table[pos].to(q.dtype)  # [S, 2, D / 2]
    cos = torch.cat((rows[:, 0], rows[:, 0]), dim=-1)[None, :, None, :]
    sin = torch.cat((rows[:, 1], rows[:, 1]), dim=-1)[None, :, None, :]
    return q * cos + rotate_half(q) * sin, k * cos + rotate_half(k) * sin


def op_alone(T):
    Hq, Hkv = args.heads
    D = args.dim
    g = torch.Generator(device=dev).manual_seed(7 + T)
    q = torch.randn(1, T, Hq, D, device=dev, generator=g).bfloat16()
    k = torch.randn(1, T, Hkv, D, device=dev, generator=g).bfloat16()
    table = ops.rope_table(T, D, device=dev)
    qo, ko = torch.empty_like(q), torch.empty_like(k)
    qi, ki = q.clone(), k.clone()  # rotated again and again in place: values stay bounded (a rotation)
    qp, kp = q[0], k[0]
    cu1 = torch.tensor([0, T], dtype=torch.int32, device=dev)
    cu64 = torch.tensor([T * i // 64 for i in range(65)], dtype=torch.int32, device=dev)
    nbytes = 2 * 2 * T * (Hq + Hkv) * D + 4 * T * D

    got = ops.rope_apply(q, k, table)
    want = eager_rope(q, k, table)
    diff = max((a.float() - b.float()).abs().max().item() for a, b in zip(got, want))
    one = ops.rope_apply(qp, kp, table, cu_seqlens=cu1)
    assert torch.equal(one[0], got[0][0]) and torch.equal(one[1], got[1][0])

    paths = {
        "out of place": lambda: ops.rope_apply(q, k, table, q_out=qo, k_out=ko),
        "in place": lambda: ops.rope_apply(qi, ki, table, q_out=qi, k_out=ki),
        "packed, 1 document": lambda: ops.rope_apply(qp, kp, table, cu_seqlens=cu1, q_out=qo[0], k_out=ko[0]),
        "packed, 64 documents": lambda: ops.rope_apply(qp, kp, table, cu_seqlens=cu64, q_out=qo[0], k_out=ko[0]),
        "eager": lambda: eager_rope(q, k, table),
    }
    res = alternate(paths, args.rounds, args.warmup, args.inner)
    rec = {"bench": "rope_apply", "T": T, "Hq": Hq, "Hkv": Hkv, "D": D, "rounds": args.rounds, "inner": args.inner,
           "bytes": nbytes, "max_abs_difference_to_eager_bf16": diff}
    for n in paths:
        rec[n] = stat(res[n], None if n == "eager" else nbytes)
    rec["eager / out of place (median)"] = round(res["eager"][0] / res["out of place"][0], 2)
    print(json.dumps(rec), flush=True)

    sweep = {f"lanes={h}": (lambda h=h: ops.rope_apply(q, k, table, q_out=qo, k_out=ko, _lanes=h))
             for h in (0, 1, 2, 4, 8, 16, 40) if h <= Hq + Hkv}
    res = alternate(sweep, args.rounds, args.warmup, args.inner)
    from collective_communication_mpi_amd import _native

    rec = {"bench": "rope_apply lanes sweep", "T": T, "chosen": _native.device().rope_head_lanes(D // 16, Hq + Hkv, False),
           "chosen_packed": _native.device().rope_head_lanes(D // 16, Hq + Hkv, True)}
    for n in sweep:
        rec[n] = stat(res[n], nbytes)
    print(json.dumps(rec), flush=True)

    sweep = {f"lanes={h}": (lambda h=h: ops.rope_apply(qp, kp, table, cu_seqlens=cu64, q_out=qo[0], k_out=ko[0], _lanes=h))
             for h in (0, 4, 8, 16, 40) if h <= Hq + Hkv}
    res = alternate(sweep, args.rounds, args.warmup, args.inner)
    rec = {"bench": "rope_apply lanes sweep, packed 64 documents", "T": T,
           "chosen": _native.device().rope_head_lanes(D // 16, Hq + Hkv, True)}
    for n in sweep:
        rec[n] = stat(res[n], nbytes)
    print(json.dumps(rec), flush=True)


def yardstick():
    T = 4096
    for V in (16032, 128256):
        g = torch.Generator(device=dev).manual_seed(7 + V)
        z = (torch.randn(T, V, device=dev, generator=g) * 2).bfloat16()
        tgt = torch.randint(0, V, (T,), device=dev, generator=g)
        stats = ops.cross_entropy_stats(z, tgt)
        lse, _, _, n_valid = ops.cross_entropy_combine(stats, tgt)
        one = torch.ones(1, device=dev)
        dl = torch.empty_like(z)
        res = alternate({"k": lambda: ops.cross_entropy_backward(z, tgt, lse, n_valid, one, 0, -100, dl)}, args.rounds,
                        args.warmup, args.inner)
        print(json.dumps({"bench": "yardstick k_xent_backward", "T": T, "V": V, "bytes": 4 * T * V,
                          **stat(res["k"], 4 * T * V)}), flush=True)
        del z, dl
        torch.cuda.empty_cache()


def model_ab():
    from collective_communication_mpi_amd import MPI, Communicator
    from collective_communication_mpi_amd.parallel import llama_dp
    from collective_communication_mpi_amd.parallel.llama_dp import LLAMA3_8B, LlamaModel, _self_comm

    comm = Communicator(MPI.COMM_WORLD)
    cfg = dataclasses.replace(LLAMA3_8B, layers=2, attention="flash", loss="fused", rope=True)
    model = LlamaModel(cfg, _self_comm(comm), dev)
    plain = dataclasses.replace(cfg, rope=False)
    tokens = 4096
    ids = torch.randint(0, cfg.vocab, (2, tokens // 2), device=dev, generator=torch.Generator(device=dev).manual_seed(3))
    kernel = llama_dp.rope

    def step(kind):
        def run():
            c = plain if kind == "no rope" else cfg
            model.cfg = c
            for blk in model.blocks:
                blk.cfg = c
            llama_dp.rope = eager_rope if kind == "eager rope" else kernel
            model.zero_grad()
            loss = model(ids)
            loss.backward()
            llama_dp.rope = kernel
            return loss
        return run

    kinds = ("no rope", "ops.rope", "eager rope")
    losses = {k: step(k)().item() for k in kinds}
    res = alternate({k: step(k) for k in kinds}, args.rounds, args.warmup, 2)
    rec = {"bench": "rope model A/B", "model": "LlamaModel 2 layers, d 4096, vocab 128256, flash attention, fused loss",
           "tokens": tokens, "rounds": args.rounds, "loss": losses}
    for k in kinds:
        rec[f"{k} step"] = stat(res[k])
    rec["ops.rope over no rope ms (median)"] = round(res["ops.rope"][0] - res["no rope"][0], 3)
    rec["eager rope over no rope ms (median)"] = round(res["eager rope"][0] - res["no rope"][0], 3)
    print(json.dumps(rec), flush=True)


if args.model:
    model_ab()
else:
    op_alone(args.tokens)
    if args.big > 1:
        torch.cuda.empty_cache()
        op_alone(args.tokens * args.big)
    yardstick()
