"""One training step of RoutedMoE(gate="fused", router_logits="mfma", expert_capacity=Ce,
aux_loss_coef > 0) on p ranks sharing the GPU: moe_capacity_train_worker.py with the router
logits on the matrix cores (``ops.moe_router_logits``), whose tokens, router, capacity, dense
fp64 model and tolerances are used as they are.

The one difference: the dense fp64 model routes every rank's tokens with the idx the LAYER
chose (``last_handle.topk_idx``, gathered from all ranks after the forward), not with a top-k
of its own.  The MFMA logits sum in another order than ``x.float() @ router.t()``, so across a
gap of rounding size the two may legitimately select differently.  That freedom is bounded
separately: with tol the forward tolerance of test_gpu_moe_router_logits.py on this rank's
tokens (8 x the error of the fp32 torch GEMM against fp64, floor 2^-22 x the largest logit),
every token whose fp64 K-th and (K + 1)-th largest logits differ by more than 2 tol must have
the fp64 top-k set, and those tokens must be at least 90 % of all tokens.

Compared as in moe_capacity_train_worker.py: x.grad, router.grad, down.grad and gate_up.grad
with its tolerances, aux_loss to 1e-5 relative, num_dropped and the kept rows exactly (the mask
from ``moe_kept`` on the host over all ranks' idx).  Prints "moe router train OK" on success."""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", ".."))
from moe_capacity_train_worker import AUX_COEF, biased_tokens, kept_masks, reference, shared_router  # noqa: E402
from moe_train_worker import COMBINE, DFF, DM, EL, GEMM, K, MODULE_G, expert_weights  # noqa: E402


def main():
    from collective_communication_mpi_amd import MPI, Communicator
    from collective_communication_mpi_amd.parallel import RoutedMoE
    assert EL == 2

    comm = Communicator(MPI.COMM_WORLD)
    rank, p = comm.Get_rank(), comm.Get_size()
    dev = comm.dev
    DEV = dev.device
    E = EL * p
    fails = []
    t0 = time.time()

    def check(tag, got, want, rtol, atol):
        if got is None:
            fails.append(f"{tag}: no gradient")
            return
        big = want.abs().max().item()
        err = (got.double() - want).abs()
        ratio = (err / (atol + rtol * want.abs())).max().item()
        print(f"[rank {rank}] {tag}: worst abs error {err.max().item():.4f} (|ref| max {big:.2f}), "
              f"worst error / tolerance {ratio:.3f}", flush=True)
        if not 1.0 <= big <= 10.0:
            fails.append(f"{tag}: the reference's largest magnitude {big:.3f} is outside [1, 10]")
        if not ratio <= 1.0:
            fails.append(f"{tag}: error exceeds rtol {rtol} atol {atol} (ratio {ratio:.3f})")

    GU, DN = expert_weights(E, DEV)
    router = shared_router(E, DEV)
    data = [biased_tokens(r, E, DEV, router) for r in range(p)]
    Ce = RoutedMoE.capacity_for(sum(d[0].shape[0] for d in data), K, E, 0.5)

    torch.manual_seed(4242)
    layer = RoutedMoE(dev, DM, DFF, E, K, EL * Ce, expert_capacity=Ce, gate="fused", aux_loss_coef=AUX_COEF,
                      router_logits="mfma")
    with torch.no_grad():
        layer.router.copy_(router)
        layer.experts.gate_up.copy_(GU[rank * EL:(rank + 1) * EL])
        layer.experts.down.copy_(DN[rank * EL:(rank + 1) * EL])
    xm = data[rank][0].clone().requires_grad_()
    gm = (data[rank][3].float() * MODULE_G).bfloat16()
    out = layer(xm)
    ((out * gm).sum() + layer.aux_loss_coef * layer.aux_loss).backward()
    torch.cuda.synchronize()
    dev.check()
    h = layer.last_handle

    # every rank's idx as its layer chose it
    idxs = [torch.as_tensor(i, device=DEV).long() for i in comm.comm.allgather(h.topk_idx.cpu().numpy())]
    for r, (i, d) in enumerate(zip(idxs, data)):
        if tuple(i.shape) != (d[0].shape[0], K) or i.min().item() < 0 or i.max().item() >= E:
            fails.append(f"rank {r}'s idx has shape {tuple(i.shape)} or entries outside [0, {E})")
    masks, counts, kept = kept_masks(idxs, E, Ce)
    dropped = (counts - kept).sum(axis=1)
    if not ((dropped > 0) & (kept.sum(axis=1) >= 20)).all():
        fails.append(f"the routing must show drops and at least 20 kept entries on every rank: dropped "
                     f"{dropped.tolist()}, kept {kept.sum(axis=1).tolist()} (Ce = {Ce})")

    # the layer's selection against fp64, wherever the gap is larger than rounding
    x = data[rank][0]
    l64 = x.double() @ router.double().t()
    own = ((x.float() @ router.t()).double() - l64).abs().max().item()
    tol = max(8 * own, 2.0 ** -22 * l64.abs().max().item())
    srt = torch.sort(l64, dim=1, descending=True)
    clear = (srt.values[:, K - 1] - srt.values[:, K]) > 2 * tol
    got_set = torch.sort(idxs[rank], dim=1).values
    want_set = torch.sort(srt.indices[:, :K], dim=1).values
    same = (got_set == want_set).all(dim=1)
    share = clear.double().mean().item()
    print(f"[rank {rank}] forward tolerance {tol:.3e} (fp32 torch error {own:.3e}); {int(clear.sum())} of "
          f"{clear.numel()} tokens have a K-th gap above 2 tol, smallest gap "
          f"{(srt.values[:, K - 1] - srt.values[:, K]).min().item():.3e}", flush=True)
    if share < 0.9:
        fails.append(f"only {share:.3f} of the tokens have a K-th gap above 2 tol: the selection check is vacuous")
    if not same[clear].all():
        fails.append(f"{int((~same[clear]).sum())} tokens with a clear gap do not have the fp64 top-k set")

    ref_dx, ref_dr, ref_aux, ref_dgu, ref_ddn = reference(data, idxs, masks, router, GU, DN, AUX_COEF)
    if h.num_dropped.item() != int(dropped[rank]):
        fails.append(f"num_dropped {h.num_dropped.item()} != {int(dropped[rank])} (moe_kept)")
    if not torch.equal(h.row_of >= 0, masks[rank]):
        fails.append("the rows the dispatch kept are not those of moe_kept")
    aux, want_aux = layer.aux_loss.item(), ref_aux[rank].item()
    print(f"[rank {rank}] aux_loss {aux:.6f} (fp64 {want_aux:.6f}), dropped {int(dropped[rank])} of "
          f"{int(counts[rank].sum())} entries, Ce = {Ce}", flush=True)
    if not abs(aux - want_aux) <= 1e-5 * abs(want_aux):
        fails.append(f"aux_loss {aux} != {want_aux}")
    rows = kept.sum(axis=0)[rank * EL:(rank + 1) * EL]
    dw_atol = 2e-3 * float(rows.max()) ** 0.5
    T = xm.shape[0]
    check("x.grad", xm.grad, ref_dx[rank], 3 * GEMM[0] + COMBINE[0], 3 * GEMM[1] + COMBINE[1])
    check("router.grad", layer.router.grad, ref_dr[rank], 2 * GEMM[0] + 2e-3, 2 * GEMM[1] + 2e-3 * T ** 0.5)
    check("down.grad", layer.experts.down.grad, ref_ddn[rank * EL:(rank + 1) * EL], GEMM[0] + 2e-3,
          GEMM[1] + dw_atol)
    check("gate_up.grad", layer.experts.gate_up.grad, ref_dgu[rank * EL:(rank + 1) * EL], 2 * GEMM[0] + 2e-3,
          2 * GEMM[1] + dw_atol)

    torch.cuda.synchronize()
    dev.check()
    bad = comm.comm.allreduce(len(fails), op=MPI.SUM)
    if fails:
        print(f"[rank {rank}] " + "\n".join(fails[:20]), flush=True)
    if rank == 0:
        print(f"moe router train OK ({time.time() - t0:.1f}s)" if bad == 0 else f"moe router train FAILED ({bad})",
              flush=True)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
