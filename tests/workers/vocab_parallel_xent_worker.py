"""Vocab-parallel cross-entropy (parallel/vocab_parallel.py) on p ranks sharing the GPU.

Every rank rebuilds the full logits [37, p Vloc] (N(0, 2^2) in bf16, Vloc in {8, W + 8}) and the
targets from one seed and takes its columns as a VIEW of the full tensor.  Row r has its target in
rank r's shard, rows p + 2 r and p + 2 r + 1 at the first and last column of rank r's shard, row
20 is ignored, row 21 is -inf over the whole shard of rank 1.

* loss, lse, row_loss and n_valid of the raw collective form are bitwise equal on all ranks
  (compared through the host plane) and within the single-GPU test's tolerance
  (test_gpu_cross_entropy.py: 4 x torch's own fp32 error, floor 2 ulps of |lse|) of the fp64
  reference on the full vocabulary; each rank's dlogits within |err| <= 2^-7 |ref| + 2^-20 scale
  of its slice of the reference.
* the autograd form equals the raw form bitwise.
* at 2 ranks, the head end to end: ``ColumnParallelLinear(256, 512, tp)`` +
  ``vocab_parallel_cross_entropy`` against the one-rank layer on the full weight of the same seed
  + ``F.cross_entropy(logits.float())``: the loss within the tolerance above (plus the exact fp64
  effect of any difference between the two layers' logits, printed; 0 when they are bitwise
  equal), the gradients of the weight shard and of x at cosine >= 0.999.
* at 2 ranks, the tiny model with ``loss="fused"`` on the 2-rank ``tp``, both attention kinds,
  against the one-rank ``loss="torch"`` model of the same seed: loss within 2^-7 relative, every
  parameter gradient (its shard of the one-rank gradient) at cosine >= 0.999 -- as the
  context-parallel worker judges its model.  At one rank "fused" against "torch" the same way, once
  with ``cu_seqlens`` and -100 targets.

Prints "vocab parallel xent OK" and the worst error / tolerance ratio."""
import os
import sys
import time
from types import SimpleNamespace

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import test_gpu_cross_entropy as gx  # noqa: E402

T = 37
IGNORE = gx.IGNORE
GRAD = gx.GRAD


def full_case(p, Vloc, device):
    g = torch.Generator().manual_seed(77 + 13 * p + Vloc)
    z = (torch.randn(T, p * Vloc, generator=g) * 2).bfloat16()
    tg = torch.randint(0, p * Vloc, (T,), generator=g)
    for r in range(p):
        tg[r] = r * Vloc + int(tg[r]) % Vloc
        tg[p + 2 * r], tg[p + 2 * r + 1] = r * Vloc, (r + 1) * Vloc - 1
    tg[20] = IGNORE
    z[21, Vloc:2 * Vloc] = float("-inf")
    tg[21] = 3
    return z.to(device), tg.to(device)


def forward_bounds(z, tg):
    """(fp64 lse, row_loss, dlogits, bound of lse, bound of row_loss) on the full vocabulary."""
    _, lse, row_loss, dl = gx.cross_entropy_reference(z, tg, 0, IGNORE, grad=GRAD)
    zf = z.float()
    y_lse = (torch.logsumexp(zf, 1).double() - lse).abs().max().item()
    y_loss = (F.cross_entropy(zf, tg, reduction="none", ignore_index=IGNORE).double() - row_loss).abs().max().item()
    floor = 2 * gx.ulp32(lse)
    return (lse, row_loss, dl, torch.maximum(torch.full_like(floor, 4 * y_lse), floor),
            torch.maximum(torch.full_like(floor, 4 * y_loss), floor))


def mean_bound(row_loss, b_loss, valid):
    """Tolerance of the mean loss: the rows' bounds, the summation tree, one division."""
    n = max(int(valid.sum()), 1)
    total = row_loss.abs().sum().item()
    return b_loss[valid].sum().item() / n + 2.0 ** -20 * total / n + 2.0 ** -23 * total / n


def cosine(a, b):
    return F.cosine_similarity(a.double().flatten(), b.double().flatten(), dim=0).item()


def shard_of(full, like, rank):
    """The part of the one-rank tensor ``full`` that a TP rank holds as ``like``."""
    if full.shape == like.shape:
        return full
    dim = [i for i, (a, b) in enumerate(zip(full.shape, like.shape)) if a != b]
    assert len(dim) == 1
    k = like.shape[dim[0]]
    return full.narrow(dim[0], rank * k, k)


def main():
    from collective_communication_mpi_amd import MPI, Communicator, ops
    from collective_communication_mpi_amd.parallel import (ColumnParallelLinear, vocab_parallel_cross_entropy,
                                                           vocab_parallel_cross_entropy_backward,
                                                           vocab_parallel_cross_entropy_forward)
    from collective_communication_mpi_amd.parallel.llama_dp import LlamaConfig, LlamaModel, _self_comm

    comm = Communicator(MPI.COMM_WORLD)
    rank, p = comm.Get_rank(), comm.Get_size()
    dev = comm.dev
    DEV = dev.device
    fails = []
    worst = 0.0
    t0 = time.time()

    for Vloc in (8, ops.XENT_SWEEP + 8):
        tag = f"Vloc={Vloc}"
        z, tg = full_case(p, Vloc, DEV)
        shard = z[:, rank * Vloc:(rank + 1) * Vloc]  # a column view: row stride p Vloc
        mean = torch.empty(1, device=DEV)
        lse, row_loss, loss_sum, n_valid = vocab_parallel_cross_entropy_forward(comm, shard, tg, IGNORE, mean=mean)
        g = torch.tensor([GRAD], device=DEV)
        dl = vocab_parallel_cross_entropy_backward(comm, shard, tg, lse, n_valid, g, IGNORE)
        torch.cuda.synchronize()

        mine = tuple(t.cpu().numpy().tobytes() for t in (mean, lse, row_loss, loss_sum, n_valid))
        for r, other in enumerate(comm.comm.allgather(mine)):
            if other != mine:
                fails.append(f"{tag}: loss / lse / row_loss / n_valid differ bitwise from rank {r}'s")

        r_lse, r_loss, r_dl, b_lse, b_loss = forward_bounds(z, tg)
        valid = tg != IGNORE
        n = int(valid.sum())
        ratios = {"lse": ((lse.double() - r_lse).abs() / b_lse).max().item(),
                  "row_loss": ((row_loss.double() - r_loss).abs() / b_loss).max().item(),
                  "loss": abs(mean.double().item() - r_loss.sum().item() / n) / mean_bound(r_loss, b_loss, valid)}
        if int(n_valid.item()) != n or bool((row_loss[~valid] != 0).any()) or torch.isnan(lse).any():
            fails.append(f"{tag}: n_valid {int(n_valid.item())} (expected {n}), an ignored row's loss, or a NaN in lse")
        col = tg - rank * Vloc
        here = valid & (col >= 0) & (col < Vloc)
        ref = SimpleNamespace(dlogits=r_dl[:, rank * Vloc:(rank + 1) * Vloc], valid=valid, here=here, col=col,
                              n_valid=n, scale=GRAD / n)
        problems, ratios["dlogits"] = gx.check_backward(SimpleNamespace(dlogits=dl), ref)
        fails += [f"{tag} {x}" for x in problems]
        for name, x in ratios.items():
            if not x <= 1.0:
                fails.append(f"{tag} {name}: error is {x:.3f} x the tolerance")
        worst = max(worst, *ratios.values())
        print(f"[rank {rank}] {tag}: worst error / tolerance " + " ".join(f"{k}={v:.3f}" for k, v in ratios.items()),
              flush=True)

        s = shard.clone().requires_grad_()
        loss = vocab_parallel_cross_entropy(comm, s, tg, IGNORE)
        (loss * GRAD).backward()
        if not torch.equal(loss.detach().reshape(1), mean) or not torch.equal(s.grad, dl):
            fails.append(f"{tag}: the autograd form differs bitwise from the raw form")
    torch.cuda.synchronize()
    dev.check()

    one = _self_comm(comm)
    if p == 2:
        # the head end to end
        Tn, d, V = 64, 256, 512
        gen = torch.Generator().manual_seed(19)
        x0 = (torch.randn(Tn, d, generator=gen) * 0.5).bfloat16().to(DEV)
        tg = torch.randint(0, V, (Tn,), generator=gen).to(DEV)
        tg[5] = IGNORE
        kw = dict(bias=False, device=DEV, dtype=torch.bfloat16, seed=11, init="device")
        head, head1 = ColumnParallelLinear(d, V, comm, **kw), ColumnParallelLinear(d, V, one, **kw)
        x, x1 = x0.clone().requires_grad_(), x0.clone().requires_grad_()
        logits = head(x)
        loss = vocab_parallel_cross_entropy(comm, logits, tg)
        loss.backward()
        logits1 = head1(x1)
        want = F.cross_entropy(logits1.float(), tg)
        want.backward()
        parts = comm.comm.allgather(logits.detach().cpu())
        tp_logits = torch.cat(parts, dim=1).to(DEV)
        r_lse, r_loss, _, _, b_loss = forward_bounds(tp_logits, tg)
        valid = tg != IGNORE
        n = int(valid.sum())
        r1 = gx.cross_entropy_reference(logits1.detach(), tg, 0, IGNORE)[2].sum().item() / n
        shift = abs(r1 - r_loss.sum().item() / n)  # fp64 effect of the two layers' logits differing
        tol = mean_bound(r_loss, b_loss, valid)
        e_ref, e_torch = abs(loss.item() - r_loss.sum().item() / n), abs(loss.item() - want.item())
        cw = cosine(head.weight.grad, shard_of(head1.weight.grad, head.weight.grad, rank))
        cx = cosine(x.grad, x1.grad)
        print(f"[rank {rank}] head: loss {loss.item():.6f}, one rank {want.item():.6f}; logits bitwise equal: "
              f"{torch.equal(tp_logits, logits1.detach())} (fp64 effect {shift:.3e}); worst error / tolerance "
              f"vs fp64 {e_ref / tol:.3f}, vs one rank {e_torch / (2 * tol + shift):.3f}; worst gradient cosine "
              f"{min(cw, cx):.6f}", flush=True)
        worst = max(worst, e_ref / tol)
        if not e_ref <= tol:
            fails.append(f"head: loss error {e_ref:.3e} against fp64 above the tolerance {tol:.3e}")
        if not e_torch <= 2 * tol + shift:  # both sides carry their own fp32 error
            fails.append(f"head: loss differs from the one-rank loss by {e_torch:.3e}, tolerance {2 * tol + shift:.3e}")
        if not min(cw, cx) >= 0.999:
            fails.append(f"head: gradient cosines weight {cw:.6f}, x {cx:.6f}")

        # the tiny model
        Bm, S = 2, 67
        ids = torch.randint(0, 512, (Bm, S), device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
        targets = torch.roll(ids, -1, dims=1)
        cu = torch.tensor([0, 40, 67, 100, Bm * S], dtype=torch.int32, device=DEV)
        packed = targets.clone().reshape(-1)
        packed[cu[1:].long() - 1] = IGNORE
        packed = packed.view(Bm, S)

        def compare(tag, model, base, r, **kw):
            base.zero_grad()
            model.zero_grad()
            a = base(ids, **kw)
            a.backward()
            b = model(ids, **kw)
            b.backward()
            rel = abs(a.item() - b.item()) / abs(a.item())
            low = 1.0
            for (name, pa), (_, pb) in zip(base.named_parameters(), model.named_parameters()):
                if pa.grad is None or pb.grad is None:
                    fails.append(f"{tag}: no gradient of {name}")
                    continue
                low = min(low, cosine(shard_of(pa.grad, pb.grad, r), pb.grad))
            print(f"[rank {rank}] {tag}: loss {b.item():.6f}, torch at one rank {a.item():.6f}, relative difference "
                  f"{rel:.3e}; worst gradient cosine {low:.6f}", flush=True)
            if not rel <= 2.0 ** -7:
                fails.append(f"{tag}: the loss differs by {rel:.3e} relative")
            if not low >= 0.999:
                fails.append(f"{tag}: worst gradient cosine {low:.6f}")

        tiny = dict(d=256, heads=4, kv_heads=2, ffn=256, vocab=512, layers=2)
        for kind in ("sdpa", "flash"):
            base = LlamaModel(LlamaConfig(**tiny, attention=kind, loss="torch"), one, DEV, seed=3)
            model = LlamaModel(LlamaConfig(**tiny, attention=kind, loss="fused"), comm, DEV, seed=3)
            compare(f"model {kind} tp=2", model, base, rank, targets=targets)
            same = LlamaModel(LlamaConfig(**tiny, attention=kind, loss="fused"), one, DEV, seed=3)
            compare(f"model {kind} tp=1", same, base, 0)
            if kind == "flash":
                compare("model flash tp=1 packed", same, base, 0, targets=packed, cu_seqlens=cu)
                compare("model flash tp=2 packed", model, base, rank, targets=packed, cu_seqlens=cu)

    torch.cuda.synchronize()
    dev.check()
    bad = comm.comm.allreduce(len(fails), op=MPI.SUM)
    if fails:
        print(f"[rank {rank}] " + "\n".join(fails[:20]), flush=True)
    if rank == 0:
        print(f"vocab parallel xent OK: worst error / tolerance {worst:.3f} ({time.time() - t0:.1f}s)" if bad == 0
              else f"vocab parallel xent FAILED ({bad})", flush=True)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
