"""Context-parallel attention (parallel/context_parallel.py) on p ranks sharing the GPU.

Every rank rebuilds the full q, k, v and dout [B, p S_loc, H, D] from shared seeds and takes its
shard of S_loc consecutive positions.  Shapes: S_loc = 67 with 4 / 2 heads and D = 64, S_loc = 128
with 8 / 1 heads and D = 128; B = 2; causal and full.

* out, lse, dq of the raw collective form equal BITWISE the local ``ops.flash_attention_chunk_*``
  call on the full contiguous k, v (the all-gather is a copy).
* dk, dv: the rank computes all p ranks' bf16 partials locally (one chunk backward per shard of q).
  The result must lie within 2^-8 x the largest magnitude of the fp64 sum of those partials (one
  bf16 rounding of an fp32 sum is 2^-9 relative; factor 2); whether it equals the rank-ordered fp32
  sum bitwise is printed.  Against the fp64 reference of the full sequence the tolerance is the
  single-GPU recipe's (test_gpu_flash_attention.py) plus 2^-8 x p x the largest partial magnitude,
  for the p extra roundings.  out and dq are held to the recipe as they are.
* the autograd form equals the raw form bitwise; the last rank asks for no gradient of q and still
  completes the collectives.
* model: the tiny flash model of test_gpu_flash_attention.py with ``cp``, explicit targets, against
  the single-process model on the full sequence: mean of the ranks' losses within 2^-7 relative,
  every parameter gradient (all-reduce-averaged over cp) at cosine >= 0.999.

Prints "context parallel OK" on success."""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from test_gpu_flash_attention import FLOOR, NAMES, _compose  # noqa: E402

B = 2
SHAPES = [(67, 4, 2, 64), (128, 8, 1, 128)]  # S_loc, Hq, Hkv, D


def full_inputs(S, Hq, Hkv, D, causal, device):
    g = torch.Generator(device=device).manual_seed(991 + 131 * S + 17 * Hq + 3 * Hkv + D + int(causal))
    mk = lambda h: torch.randn(B, S, h, D, device=device, generator=g).bfloat16()
    return mk(Hq), mk(Hkv), mk(Hkv), mk(Hq)  # q, k, v, dout


def main():
    from collective_communication_mpi_amd import MPI, Communicator, ops
    from collective_communication_mpi_amd.parallel import (context_parallel_attention,
                                                           context_parallel_attention_backward,
                                                           context_parallel_attention_forward)
    from collective_communication_mpi_amd.parallel.llama_dp import LlamaConfig, LlamaModel, _self_comm

    comm = Communicator(MPI.COMM_WORLD)
    rank, p = comm.Get_rank(), comm.Get_size()
    dev = comm.dev
    DEV = dev.device
    fails = []
    t0 = time.time()

    def same(tag, got, want):
        if not torch.equal(got, want):
            fails.append(f"{tag}: not bitwise equal (worst difference {(got.double() - want.double()).abs().max().item():.3e})")

    for S_loc, Hq, Hkv, D in SHAPES:
        for causal in (True, False):
            tag = f"S_loc={S_loc} H={Hq}x{Hkv} D={D} {'causal' if causal else 'full'}"
            S = p * S_loc
            q, k, v, dout = full_inputs(S, Hq, Hkv, D, causal, DEV)
            lo, hi = rank * S_loc, (rank + 1) * S_loc
            qs, ks, vs, dos = (t[:, lo:hi].contiguous() for t in (q, k, v, dout))

            out, lse = context_parallel_attention_forward(comm, qs, ks, vs, causal)
            dq, dk, dv = context_parallel_attention_backward(comm, dos, qs, ks, vs, out, lse, causal)

            # the local chunk calls on the full contiguous k, v: every shard of q, so all p partials
            parts = []
            for r in range(p):
                a, b = r * S_loc, (r + 1) * S_loc
                qr, dor = q[:, a:b].contiguous(), dout[:, a:b].contiguous()
                o_r, l_r = ops.flash_attention_chunk_forward(qr, k, v, causal, q_pos0=a)
                parts.append((o_r, l_r, *ops.flash_attention_chunk_backward(dor, qr, k, v, o_r, l_r, causal, q_pos0=a)))
            same(f"{tag} out", out, parts[rank][0])
            same(f"{tag} lse", lse, parts[rank][1])
            same(f"{tag} dq", dq, parts[rank][2])

            ref = _compose(q, k, v, dout, causal, torch.float64)
            f32 = _compose(q, k, v, dout, causal, torch.float32)
            tol = {n: max(8 * (c.bfloat16().double() - r).abs().max().item(), FLOOR * r.abs().max().item())
                   for n, r, c in zip(NAMES, (ref[0], *ref[2:]), (f32[0], *f32[2:]))}
            ratios = {}
            for name, got, i in (("out", out, 0), ("dq", dq, 2)):
                ratios[name] = (got.double() - ref[i][:, lo:hi]).abs().max().item() / tol[name]
            for name, got, i in (("dk", dk, 3), ("dv", dv, 4)):
                p64 = [pt[i][:, lo:hi].double() for pt in parts]
                sum64 = sum(p64)
                sum32 = parts[0][i][:, lo:hi].float()
                for pt in parts[1:]:
                    sum32 = sum32 + pt[i][:, lo:hi].float()
                bound = 2.0 ** -8 * sum64.abs().max().item()
                err = (got.double() - sum64).abs().max().item()
                ratios[name + "/partials"] = err / bound
                extra = 2.0 ** -8 * p * max(x.abs().max().item() for x in p64)
                ratios[name] = (got.double() - ref[i][:, lo:hi]).abs().max().item() / (tol[name] + extra)
                print(f"[rank {rank}] {tag} {name}: equals the rank-ordered fp32 sum bitwise: "
                      f"{torch.equal(got, sum32.bfloat16())}", flush=True)
            lse_err = ((lse.double() - ref[1][:, :, lo:hi]).abs() / (1 + ref[1][:, :, lo:hi].abs())).max().item() * 2.0 ** 20
            print(f"[rank {rank}] {tag}: worst error / tolerance " + " ".join(f"{n}={x:.3f}" for n, x in ratios.items())
                  + f" lse={lse_err:.3f}", flush=True)
            for n, x in ratios.items():
                if not x <= 1.0:
                    fails.append(f"{tag} {n}: error is {x:.3f} x the tolerance")
            if not lse_err <= 1.0:
                fails.append(f"{tag} lse: error {lse_err:.3f} x 2^-20 (1 + |lse|)")

            # autograd form; the last rank needs no gradient of q and must still run the collectives
            need_q = rank != p - 1
            ql, kl, vl = qs.clone().requires_grad_(need_q), ks.clone().requires_grad_(), vs.clone().requires_grad_()
            o2 = context_parallel_attention(comm, ql, kl, vl, causal)
            o2.backward(dos)
            same(f"{tag} autograd out", o2.detach(), out)
            same(f"{tag} autograd dk", kl.grad, dk)
            same(f"{tag} autograd dv", vl.grad, dv)
            if need_q:
                same(f"{tag} autograd dq", ql.grad, dq)
            elif ql.grad is not None:
                fails.append(f"{tag}: a gradient of q appeared on a rank that asked for none")
    torch.cuda.synchronize()
    dev.check()

    # model: the sequence split over the ranks against the single-process model on all of it
    S_loc, Bm = 67, 2
    S = p * S_loc
    tp = _self_comm(comm)
    cfg = LlamaConfig(d=256, heads=4, kv_heads=2, ffn=256, vocab=512, layers=2, attention="flash")
    single = LlamaModel(cfg, tp, DEV, seed=3)
    split = LlamaModel(cfg, tp, DEV, seed=3, cp=comm)
    for a, b in zip(single.parameters(), split.parameters()):
        assert torch.equal(a, b)
    ids = torch.randint(0, 512, (Bm, S), device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    targets = torch.roll(ids, -1, dims=1)
    want = single(ids, targets=targets)
    want.backward()
    lo, hi = rank * S_loc, (rank + 1) * S_loc
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

    torch.cuda.synchronize()
    dev.check()
    bad = comm.comm.allreduce(len(fails), op=MPI.SUM)
    if fails:
        print(f"[rank {rank}] " + "\n".join(fails[:20]), flush=True)
    if rank == 0:
        print(f"context parallel OK ({time.time() - t0:.1f}s)" if bad == 0 else f"context parallel FAILED ({bad})",
              flush=True)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
