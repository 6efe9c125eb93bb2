"""RMSNorm with the residual add in front of it (``ops.rms_norm`` / ``ops.add_rms_norm``,
csrc/device/rmsnorm.hip) against ``F.rms_norm`` and ``x + r`` followed by ``F.rms_norm``.

    python benchmarks/rms_norm.py                 # the ops alone
    python benchmarks/rms_norm.py --model         # a 2-layer LlamaModel step, norm="torch" against "fused"

The ops alone at ``d = 4096`` with ``T = 8192`` (64 MB per tensor: inside the 256 MiB Infinity
Cache) and ``--big`` times as many rows (256 MB per tensor: beyond it), bf16 weight.  Forward:
the raw ops with every buffer passed in against torch's forward.  Backward: the raw
``rms_norm_backward`` (``dh`` and ``dw``, buffers passed in) and the autograd forms, against
autograd through the torch composition; both sides differentiate a graph built once
(``torch.autograd.grad(..., retain_graph=True)``), so only the backward is timed.  All paths
alternate in one process; one sample = ``--inner`` back-to-back calls between two device events;
median and minimum over the rounds.  ``bytes`` is what the op MUST move, from the shapes: every
[T, d] operand read once and every [T, d] result written once, plus ``rstd`` and the weight
(the backward's ``dw`` partials are not counted: they are the kernel's own).

The yardstick: ``k_xent_backward`` (one read pass, one write pass of bf16), timed in the same
process at T = 4096 and V = 16032 / 128256.

--model: ``LlamaModel`` (Llama-3-8B widths, 2 layers, vocabulary 128256, attention="flash",
loss="fused"), 4096 tokens as 2 x 2048, one rank; the SAME weights with norm="torch" and
norm="fused" alternating: step time (zero_grad + forward + backward) and both losses.

Prints one JSON line per record (``--session`` tags them; ``--out`` appends them to a file)."""
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
ap.add_argument("--tokens", type=int, default=8192)
ap.add_argument("--big", type=int, default=4, help="also run at this multiple of --tokens")
ap.add_argument("--dim", type=int, default=4096)
ap.add_argument("--rounds", type=int, default=20)
ap.add_argument("--inner", type=int, default=20, help="calls per sample")
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--model", action="store_true")
ap.add_argument("--session", type=int, default=None)
ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
args = ap.parse_args()
dev = torch.device("cuda")
EPS = 1e-5


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


def op_alone(T):
    d = args.dim
    g = torch.Generator(device=dev).manual_seed(7 + T)
    x, r, dy, dres = (torch.randn(T, d, device=dev, generator=g).bfloat16() for _ in range(4))
    w = (0.5 + torch.rand(d, device=dev, generator=g)).bfloat16()
    h, y, dh = (torch.empty_like(x) for _ in range(3))
    rstd = torch.empty(T, dtype=torch.float32, device=dev)
    dw = torch.empty(d, dtype=torch.float32, device=dev)
    chunk = ops.rms_norm_row_chunk(T, d)
    parts = torch.empty(((T + chunk - 1) // chunk, d), dtype=torch.float32, device=dev)
    row, small = 2 * T * d, 4 * T + 2 * d  # one [T, d] bf16 tensor; rstd and the weight

    # the same values on both sides, to what bf16 allows
    ops.add_rms_norm_forward(x, r, w, EPS, h=h, y=y, rstd=rstd)
    want = F.rms_norm(x + r, (d,), w, EPS)
    diff = (y.float() - want.float()).abs().max().item()

    # graphs built once; only their backward is timed
    leaves = lambda *ts: [t.clone().requires_grad_() for t in ts]
    xa, wa = leaves(x, w)
    ya = ops.rms_norm(xa, wa, EPS)
    xt, wt = leaves(x, w)
    yt = F.rms_norm(xt, (d,), wt, EPS)
    xb, rb, wb = leaves(x, r, w)
    hb, yb = ops.add_rms_norm(xb, rb, wb, EPS)
    xu, ru, wu = leaves(x, r, w)
    hu = xu + ru
    yu = F.rms_norm(hu, (d,), wu, EPS)
    grad = lambda outs, ins, gs: (lambda: torch.autograd.grad(outs, ins, gs, retain_graph=True))

    paths = {
        "rms_norm forward": lambda: ops.rms_norm_forward(x, w, EPS, y=y, rstd=rstd),
        "F.rms_norm forward": lambda: F.rms_norm(x, (d,), w, EPS),
        "add_rms_norm forward": lambda: ops.add_rms_norm_forward(x, r, w, EPS, h=h, y=y, rstd=rstd),
        "x + r, F.rms_norm forward": lambda: F.rms_norm(x + r, (d,), w, EPS),
        "rms_norm_backward": lambda: ops.rms_norm_backward(dy, h, w, rstd, dh=dh, dw=dw, partials=parts),
        "rms_norm_backward, no dw": lambda: ops.rms_norm_backward(dy, h, w, rstd, dh=dh, need_dw=False),
        "rms_norm_backward with dres": lambda: ops.rms_norm_backward(dy, h, w, rstd, dres, dh=dh, dw=dw, partials=parts),
        "rms_norm autograd backward": grad(ya, (xa, wa), dy),
        "F.rms_norm autograd backward": grad(yt, (xt, wt), dy),
        "add_rms_norm autograd backward": grad((hb, yb), (xb, rb, wb), (dres, dy)),
        "x + r, F.rms_norm autograd backward": grad((hu, yu), (xu, ru, wu), (dres, dy)),
    }
    nbytes = {
        "rms_norm forward": 2 * row + small,
        "add_rms_norm forward": 4 * row + small,
        "rms_norm_backward": 3 * row + small + 4 * d,
        "rms_norm_backward, no dw": 3 * row + small,
        "rms_norm_backward with dres": 4 * row + small + 4 * d,
        "rms_norm autograd backward": 3 * row + small + 4 * d,
        "add_rms_norm autograd backward": 4 * row + small + 4 * d,
    }
    res = alternate(paths, args.rounds, args.warmup, args.inner)
    rec = {"bench": "rms_norm", "T": T, "d": d, "rounds": args.rounds, "inner": args.inner, "row_chunk": chunk,
           "bytes_per_tensor": row, "max_abs_difference_to_torch_bf16": diff}
    for n in paths:
        rec[n] = stat(res[n], nbytes.get(n))
        if n in nbytes:
            rec[n]["bytes"] = nbytes[n]
    ratio = lambda a, b: round(res[a][0] / res[b][0], 2)
    rec["F.rms_norm / rms_norm forward (median)"] = ratio("F.rms_norm forward", "rms_norm forward")
    rec["torch / add_rms_norm forward (median)"] = ratio("x + r, F.rms_norm forward", "add_rms_norm forward")
    rec["F.rms_norm / rms_norm backward (median)"] = ratio("F.rms_norm autograd backward", "rms_norm autograd backward")
    rec["torch / add_rms_norm backward (median)"] = ratio("x + r, F.rms_norm autograd backward", "add_rms_norm autograd backward")
    emit(rec)


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
        emit({"bench": "yardstick k_xent_backward", "T": T, "V": V, "bytes": 4 * T * V, **stat(res["k"], 4 * T * V)})
        del z, dl
        torch.cuda.empty_cache()


def model_ab():
    from collective_communication_mpi_amd import MPI, Communicator
    from collective_communication_mpi_amd.parallel.llama_dp import LLAMA3_8B, LlamaModel, _self_comm

    comm = Communicator(MPI.COMM_WORLD)
    cfgs = {kind: dataclasses.replace(LLAMA3_8B, layers=2, attention="flash", loss="fused", norm=kind)
            for kind in ("torch", "fused")}
    model = LlamaModel(cfgs["torch"], _self_comm(comm), dev)
    tokens = 4096
    ids = torch.randint(0, LLAMA3_8B.vocab, (2, tokens // 2), device=dev, generator=torch.Generator(device=dev).manual_seed(3))

    def step(kind):
        def run():
            model.cfg = cfgs[kind]
            for blk in model.blocks:
                blk.cfg = cfgs[kind]
            model.zero_grad()
            loss = model(ids)
            loss.backward()
            return loss
        return run

    losses = {k: step(k)().item() for k in cfgs}
    res = alternate({k: step(k) for k in cfgs}, args.rounds, args.warmup, 2)
    rec = {"bench": "rms_norm model A/B", "model": "LlamaModel 2 layers, d 4096, vocab 128256, flash attention, fused loss",
           "tokens": tokens, "rounds": args.rounds, "loss": losses}
    for k in cfgs:
        rec[f'norm="{k}" step'] = stat(res[k])
    rec["fused - torch ms (median)"] = round(res["fused"][0] - res["torch"][0], 3)
    emit(rec)


if args.model:
    model_ab()
else:
    op_alone(args.tokens)
    if args.big > 1:
        torch.cuda.empty_cache()
        op_alone(args.tokens * args.big)
    yardstick()
