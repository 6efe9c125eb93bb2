"""One training step of RoutedMoE(gate="fused", expert_capacity=Ce, aux_loss_coef > 0) on p
ranks sharing the GPU, at the shapes of moe_train_worker.py (whose tokens, expert weights,
dense layer and tolerances are used as they are): D = 128, d_ff = 64, two local experts per
rank, K = 2, T = 100 + 7 * rank tokens, loss = (out * 2.5 g_r).sum() + coef * layer.aux_loss.

Entries are kept in source-rank order, so under balanced routing rank 0 would lose nothing
or the last rank everything.  Rank r's tokens are therefore shifted by 0.75 (router[2 r] +
router[2 r + 1]): it sends most of its entries to experts 2 r and 2 r + 1 and a few to the
others.  With Ce = ceil(0.5 * all tokens * K / E), half the balanced load, every rank then
loses entries on its preferred experts and keeps some (both asserted from the oracle; a
collapsing router is also the case the capacity is for).

Every rank rebuilds every rank's tokens, the router and all expert weights from shared seeds and routes every rank's tokens as the
layer's torch gate would (fp32 softmax of the same logits, ``topk``); its own fused ``idx``
must equal that exactly (the inputs have no ties).  The kept mask comes from ``moe_kept`` on
the host, never from the handle: rank i keeps the first kept[i][e] of its entries for expert e
in (token, slot) order.  The reference is the dense fp64 autograd model of all ranks' tokens
with a dropped slot's weight masked to zero (after the renormalisation over all K selected:
nothing is renormalised again after a drop) and coef * E * sum_e f_e P_e added per rank.

Compared, with moe_train_worker.py's composed tolerances and its requirement that every
reference gradient's largest magnitude lies in [1, 10]: x.grad and router.grad of this rank
(module path rows), gate_up.grad and down.grad of this rank's experts (functional path rows,
the weight gradients' atol from the largest kept row count); aux_loss itself to 1e-5 relative
(an fp32 sum of T * E probabilities against fp64), num_dropped exactly.
Prints "moe capacity train OK" on success."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", ".."))
from moe_train_worker import COMBINE, DFF, DM, EL, GEMM, K, MODULE_G, dense_layer, expert_weights, tokens  # noqa: E402

AUX_COEF = 20.0


def shared_router(E, dev):
    return torch.randn(E, DM, generator=torch.Generator(device=dev).manual_seed(77), device=dev) / DM ** 0.5


BIAS = 0.75


def biased_tokens(r, E, dev, router):
    """moe_train_worker's tokens of rank r (x, g), x shifted towards experts 2 r and 2 r + 1."""
    x, _, _, gr = tokens(r, E, dev)
    return (x.float() + BIAS * (router[2 * r] + router[2 * r + 1])).bfloat16(), None, None, gr


def torch_gate(x, router):
    """The layer's torch gate on one rank's tokens: (fp32 logits, idx [T, K])."""
    logits = x.float() @ router.t()
    return logits, torch.softmax(logits, dim=-1).topk(K, dim=-1).indices


def kept_masks(idxs, E, Ce):
    """Per rank the [T, K] mask of entries that survive, from moe_kept on the host."""
    from collective_communication_mpi_amd.device import moe_kept

    counts = np.stack([np.bincount(i.reshape(-1).cpu().numpy(), minlength=E) for i in idxs])
    kept = moe_kept(counts, Ce)
    masks = []
    for r, idx in enumerate(idxs):
        flat = idx.reshape(-1).cpu()
        m = torch.zeros_like(flat, dtype=torch.bool)
        for e in range(E):
            at = (flat == e).nonzero().reshape(-1)            # this rank's entries of e in (token, slot) order
            m[at[:int(kept[r, e])]] = True
        masks.append(m.view_as(idx).to(idx.device))
    return masks, counts, kept


def reference(data, idxs, masks, router, gu, dn, coef):
    """fp64 autograd over all ranks' tokens: per rank (x.grad, router.grad, aux), and the expert grads."""
    E = gu.shape[0]
    gu64, dn64 = gu.double().requires_grad_(), dn.double().requires_grad_()
    xs = [d[0].double().requires_grad_() for d in data]
    rs = [router.double().clone().requires_grad_() for _ in data]
    loss, auxs = 0.0, []
    for x, r, d, idx, m in zip(xs, rs, data, idxs, masks):
        T = x.shape[0]
        probs = torch.softmax(x @ r.T, dim=-1)
        w = probs.gather(1, idx)
        w = w / w.sum(dim=-1, keepdim=True)
        f = torch.bincount(idx.reshape(-1), minlength=E).double() / (T * K)
        aux = E * (f * probs.sum(dim=0) / T).sum()
        auxs.append(aux.detach())
        g = (d[3].float() * MODULE_G).bfloat16().double()
        loss = loss + (dense_layer(x, idx, w * m, gu64, dn64) * g).sum() + coef * aux
    loss.backward()
    return [x.grad for x in xs], [r.grad for r in rs], auxs, gu64.grad, dn64.grad


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
    gates = [torch_gate(d[0], router) for d in data]
    idxs = [g[1] for g in gates]
    masks, counts, kept = kept_masks(idxs, E, Ce)
    dropped = (counts - kept).sum(axis=1)
    if not ((dropped > 0) & (kept.sum(axis=1) >= 20)).all():
        fails.append(f"the oracle must show drops and at least 20 kept entries on every rank: dropped "
                     f"{dropped.tolist()}, kept {kept.sum(axis=1).tolist()} (Ce = {Ce})")
    srt = torch.sort(gates[rank][0], dim=1, descending=True).values
    if (srt[:, :K] == srt[:, 1:K + 1]).any():
        fails.append("the logits have a tie among the first K + 1")
    ref_dx, ref_dr, ref_aux, ref_dgu, ref_ddn = reference(data, idxs, masks, router, GU, DN, AUX_COEF)

    torch.manual_seed(4242)
    layer = RoutedMoE(dev, DM, DFF, E, K, EL * Ce, expert_capacity=Ce, gate="fused", aux_loss_coef=AUX_COEF)
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
    if not torch.equal(h.topk_idx.long(), idxs[rank]):
        fails.append("the fused gate's idx differs from torch.topk of the same probabilities")
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
        print(f"moe capacity train OK ({time.time() - t0:.1f}s)" if bad == 0 else f"moe capacity train FAILED ({bad})",
              flush=True)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
