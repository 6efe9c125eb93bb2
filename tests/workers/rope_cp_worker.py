"""Rotary position embedding under context parallelism, on p ranks sharing the GPU.

* op: every rank rebuilds the full q, k [B, p S_loc, H, D] from shared seeds; ``ops.rope_apply`` on
  its shard of S_loc consecutive positions with ``pos0 = r S_loc`` equals BITWISE its rows of the
  ``pos0 = 0`` call on the full sequence (both pairings, both directions), and is held to the
  accuracy bound of test_gpu_rope.py against the fp64 reference.
* model: the tiny ``rope=True`` flash model with ``cp``, explicit targets, against the
  single-process ``rope=True`` model on the full sequence (S_loc = 67, B = 2): mean of the ranks'
  losses within 2^-7 relative, every parameter gradient (all-reduce-averaged over cp) at cosine >=
  0.999.  The same split WITHOUT the rank's offset would not pass: the ranks' models see the
  positions their rows have in the full sequence.

Prints "rope context parallel OK" on success."""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", ".."))

B, S_LOC = 2, 67
SHAPES = [(4, 2, 64), (3, 5, 80)]  # Hq, Hkv, D


def main():
    from collective_communication_mpi_amd import MPI, Communicator, ops
    from collective_communication_mpi_amd.parallel.llama_dp import LlamaConfig, LlamaModel, _self_comm

    comm = Communicator(MPI.COMM_WORLD)
    rank, p = comm.Get_rank(), comm.Get_size()
    dev = comm.dev
    DEV = dev.device
    fails = []
    t0 = time.time()
    S = p * S_LOC
    lo, hi = rank * S_LOC, (rank + 1) * S_LOC

    worst = 0.0
    for Hq, Hkv, D in SHAPES:
        g = torch.Generator(device=DEV).manual_seed(77 + 17 * Hq + 3 * Hkv + D)
        q = torch.randn(B, S, Hq, D, device=DEV, generator=g).bfloat16()
        k = torch.randn(B, S, Hkv, D, device=DEV, generator=g).bfloat16()
        table = ops.rope_table(S, D, device=DEV)
        pos = torch.arange(lo, hi, device=DEV).repeat(B, 1)
        for interleaved in (False, True):
            for inverse in (False, True):
                tag = f"H={Hq}x{Hkv} D={D} interleaved={interleaved} inverse={inverse}"
                full = ops.rope_apply(q, k, table, 0, interleaved=interleaved, inverse=inverse)
                mine = ops.rope_apply(q[:, lo:hi], k[:, lo:hi], table, lo, interleaved=interleaved, inverse=inverse)
                for name, got, want, x in (("q", mine[0], full[0], q), ("k", mine[1], full[1], k)):
                    if not torch.equal(got, want[:, lo:hi]):
                        fails.append(f"{tag} {name}: the shard at pos0 = {lo} is not bitwise its rows of the full call")
                    xs = x[:, lo:hi]
                    exact = ops.rope_reference(xs, table, pos, interleaved, inverse)
                    a = xs.double().abs()
                    s = a[..., 0::2] + a[..., 1::2] if interleaved else a[..., :D // 2] + a[..., D // 2:]
                    s = torch.stack((s, s), dim=-1).reshape(a.shape) if interleaved else torch.cat((s, s), dim=-1)
                    r = ((got.double() - exact).abs() / (2.0 ** -8 * exact.abs() + 2.0 ** -22 * s)).max().item()
                    worst = max(worst, r)
                    if not r <= 1.0:
                        fails.append(f"{tag} {name}: error is {r:.3f} x the tolerance")
    print(f"[rank {rank}] rope op: worst error / tolerance {worst:.3f}", flush=True)
    torch.cuda.synchronize()
    dev.check()

    # model: the sequence split over the ranks against the single-process model on all of it
    tp = _self_comm(comm)
    cfg = LlamaConfig(d=256, heads=4, kv_heads=2, ffn=256, vocab=512, layers=2, attention="flash", rope=True)
    single = LlamaModel(cfg, tp, DEV, seed=3)
    split = LlamaModel(cfg, tp, DEV, seed=3, cp=comm)
    for a, b in zip(single.parameters(), split.parameters()):
        assert torch.equal(a, b)
    assert [(blk.cp_size, blk.cp_rank) for blk in split.blocks] == [(p, rank)] * cfg.layers
    ids = torch.randint(0, 512, (B, S), device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    targets = torch.roll(ids, -1, dims=1)
    want = single(ids, targets=targets)
    want.backward()
    loss = split(ids[:, lo:hi].contiguous(), targets=targets[:, lo:hi].contiguous())
    loss.backward()
    mean = comm.comm.allreduce(loss.item(), op=MPI.SUM) / p
    rel = abs(mean - want.item()) / abs(want.item())
    worst = 1.0
    for (name, a), (_, b) in zip(single.named_parameters(), split.named_parameters()):
        if a.grad is None or b.grad is None:
            fails.append(f"model: no gradient of {name}")
            continue
        g = torch.empty_like(b.grad, dtype=torch.float32)
        comm.Allreduce(b.grad.float().contiguous(), g, MPI.SUM)
        cos = torch.nn.functional.cosine_similarity(a.grad.double().flatten(), (g / p).double().flatten(), dim=0).item()
        worst = min(worst, cos)
    print(f"[rank {rank}] model: loss single {want.item():.6f}, mean over cp {mean:.6f}, relative difference {rel:.3e}; "
          f"worst gradient cosine {worst:.6f}", flush=True)
    if not rel <= 2.0 ** -7:
        fails.append(f"model: the mean loss differs by {rel:.3e} relative")
    if not worst >= 0.999:
        fails.append(f"model: worst gradient cosine {worst:.6f}")
    # a sequence of cp_size * seq positions beyond max_positions is refused before any launch,
    # on every rank alike (no collective is entered)
    small = LlamaModel(LlamaConfig(**{**cfg.__dict__, "max_positions": S - 1}), tp, DEV, seed=3, cp=comm)
    try:
        small(ids[:, lo:hi].contiguous(), targets=targets[:, lo:hi].contiguous())
        fails.append("model: cp_size * seq beyond max_positions was accepted")
    except ValueError as e:
        if "max_positions" not in str(e):
            fails.append(f"model: unexpected refusal {e}")

    torch.cuda.synchronize()
    dev.check()
    bad = comm.comm.allreduce(len(fails), op=MPI.SUM)
    if fails:
        print(f"[rank {rank}] " + "\n".join(fails[:20]), flush=True)
    if rank == 0:
        print(f"rope context parallel OK ({time.time() - t0:.1f}s)" if bad == 0 else f"rope context parallel FAILED ({bad})",
              flush=True)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
