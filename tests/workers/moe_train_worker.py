"""One training step through the routed MoE layer on p ranks sharing the GPU: the autograd
moe_dispatch -> GroupedExpertsMLP -> autograd moe_combine, then the RoutedMoE module.

Functional path.  The set-up of moe_experts_worker.py: D = 128, d_ff = 64, two local experts
per rank, K = 2, T = 100 + 7 * rank tokens; every token's first slot goes to expert 0 (well
over one 128-row tile), nobody chooses expert 1, second slots spread over the other experts,
some dropped.  x and the combine weights are leaves, the loss is (out * g_r).sum() on every
rank.  Every rank rebuilds every rank's tokens, routing, weights, g_r and all expert weights
from shared seeds, evaluates the whole layer for all ranks' tokens densely in fp64 with torch
autograd, and compares x.grad, weights.grad and gate_up.grad / down.grad of its own experts.

Tolerances, composed as in moe_experts_worker.py from the project's own: rtol 2e-2 / atol 8e-2
per bf16 GEMM in the chain to a gradient, the combine's 1e-2 K / 4e-2 K where a slot sum is
involved, and for a weight gradient test_gpu_grouped_gemm.py's rtol 2e-3 / atol 2e-3
sqrt(largest count):
  x.grad        gate|up forward, down dX, gate|up dX, slot sum   rtol 8e-2    atol 4.0e-1
  weights.grad  gate|up forward, down forward (a dot, no slot sum) rtol 4e-2  atol 1.6e-1
  down.grad     gate|up forward + the weight gradient            rtol 2.2e-2  atol 8e-2 + 2e-3 sqrt(rows)
  gate_up.grad  gate|up forward, down dX + the weight gradient   rtol 4.2e-2  atol 1.6e-1 + 2e-3 sqrt(rows)
The atol terms were set for values of a few units, so g_r, the combine weights and x against
gate_up are scaled until every reference gradient's largest magnitude lies in [1, 10] (asserted).
Worst error / tolerance measured on an MI355X (2 and 3 ranks, every rank): x.grad 0.029,
weights.grad 0.054, down.grad 0.207, gate_up.grad 0.090 (reference maxima 1.7 to 6.1);
module path x.grad 0.022, router.grad 0.141 (reference maxima 1.4 to 6.9).

Module path.  One RoutedMoE (E = 2 p, K = 2) forward + backward with loss (out * 2.5 g_r).sum(),
the factor chosen so that both reference gradients again have their largest magnitude in
[1, 10] (asserted):
the router gradient is finite and non-zero; x.grad and the router gradient match an fp64
evaluation that routes as the forward did (handle.topk_idx), so a tie in the top-k cannot
flip the comparison.  x.grad: the functional path's tolerance (the router's part is fp32
torch).  router.grad = dlogits^T x is a weight gradient over the T rows of this rank whose
input comes from dweights: composed like gate_up.grad, the weights.grad terms plus the weight
gradient's rtol 2e-3 / atol 2e-3 sqrt(T).
Prints "moe train OK" on success."""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", ".."))

DM, DFF, EL, K = 128, 64, 2, 2
GEMM, COMBINE = (2e-2, 8e-2), (1e-2 * K, 4e-2 * K)
G_SCALE = 0.1           # of g_r
W_SCALE = 2.0           # of the combine weights: every gradient but their own grows with them
W0_SCALE = 0.5          # of the first slot's weights (expert 0 takes every token)
MODULE_G = 2.5          # of g_r on the module path: its renormalised weights sum to 1 per token, not to about 2
X_SCALE = 0.5           # of x, and its inverse of gate_up: the same hidden values, x.grad up, gate_up.grad down


def tokens(r, E, dev):
    """Rank r's (x, topk_idx, combine weights, g): identical on every rank that asks."""
    T = 100 + 7 * r
    g = torch.Generator(device=dev).manual_seed(50_021 + 977 * r)
    x = (torch.randn(T, DM, generator=g, device=dev) * X_SCALE).bfloat16()
    first = torch.zeros(T, 1, dtype=torch.int64, device=dev)
    second = torch.randint(2, E, (T, 1), generator=g, device=dev)
    second[torch.rand(T, 1, generator=g, device=dev) < 0.1] = -1      # some dropped slots
    w = (torch.rand(T, K, generator=g, device=dev) + 0.25) * W_SCALE
    w[:, 0] *= W0_SCALE
    gr = (torch.randn(T, DM, generator=g, device=dev) * G_SCALE).bfloat16()
    return x, torch.cat([first, second], dim=1), w, gr


def expert_weights(E, dev):
    g = torch.Generator(device=dev).manual_seed(123_457)
    gu = (torch.randn(E, 2 * DFF, DM, generator=g, device=dev) / (X_SCALE * DM ** 0.5)).bfloat16()
    dn = (torch.randn(E, DM, DFF, generator=g, device=dev) / DFF ** 0.5).bfloat16()
    return gu, dn


def dense_layer(x, idx, w, gu, dn):
    """Per token: sum_k w[t, k] * down[e] . swiglu(gate_up[e] . x[t]), e = idx[t, k] (differentiable)."""
    out = torch.zeros(x.shape[0], DM, dtype=x.dtype, device=x.device)
    for k in range(idx.shape[1]):
        for e in range(gu.shape[0]):
            m = idx[:, k] == e
            if not m.any():
                continue
            h = x[m] @ gu[e].T
            a = torch.nn.functional.silu(h[:, 0::2]) * h[:, 1::2]
            out = out.index_add(0, m.nonzero().reshape(-1), w[m, k:k + 1] * (a @ dn[e].T))
    return out


def reference(data, gu, dn):
    """fp64 autograd over all ranks' tokens: ([x.grad], [weights.grad], gate_up.grad, down.grad)."""
    gu64, dn64 = gu.double().requires_grad_(), dn.double().requires_grad_()
    xs = [d[0].double().requires_grad_() for d in data]
    ws = [d[2].double().requires_grad_() for d in data]
    loss = sum((dense_layer(x, d[1], w, gu64, dn64) * d[3].double()).sum() for x, w, d in zip(xs, ws, data))
    loss.backward()
    return [x.grad for x in xs], [w.grad for w in ws], gu64.grad, dn64.grad


def main():
    from collective_communication_mpi_amd import MPI, Communicator
    from collective_communication_mpi_amd.parallel import GroupedExpertsMLP, RoutedMoE, moe_combine, moe_dispatch

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

    # ---- functional path ------------------------------------------------------------
    GU, DN = expert_weights(E, DEV)
    data = [tokens(r, E, DEV) for r in range(p)]
    rows = torch.bincount(torch.cat([d[1][d[1] >= 0] for d in data]), minlength=E).tolist()
    if not (max(rows) > 128 and min(rows) == 0):
        fails.append(f"routing is not skewed enough: rows per expert {rows}")
    cap = sum(d[0].shape[0] for d in data) * K + 8        # host-known bound: everything lands on one rank
    ref_dx, ref_dw, ref_dgu, ref_ddn = reference(data, GU, DN)

    mlp = GroupedExpertsMLP(EL, DM, DFF, device=DEV)
    with torch.no_grad():
        mlp.gate_up.copy_(GU[rank * EL:(rank + 1) * EL])
        mlp.down.copy_(DN[rank * EL:(rank + 1) * EL])
    x = data[rank][0].clone().requires_grad_()
    w = data[rank][2].clone().requires_grad_()
    recv, h = moe_dispatch(dev, x, data[rank][1], E, cap)
    out = moe_combine(dev, mlp(recv, h.expert_counts), h, w)
    (out * data[rank][3]).sum().backward()
    torch.cuda.synchronize()
    dev.check()
    dw_atol = 2e-3 * max(rows[rank * EL:(rank + 1) * EL]) ** 0.5
    check("x.grad", x.grad, ref_dx[rank], 3 * GEMM[0] + COMBINE[0], 3 * GEMM[1] + COMBINE[1])
    check("weights.grad", w.grad, ref_dw[rank], 2 * GEMM[0], 2 * GEMM[1])
    check("down.grad", mlp.down.grad, ref_ddn[rank * EL:(rank + 1) * EL], GEMM[0] + 2e-3, GEMM[1] + dw_atol)
    check("gate_up.grad", mlp.gate_up.grad, ref_dgu[rank * EL:(rank + 1) * EL], 2 * GEMM[0] + 2e-3,
          2 * GEMM[1] + dw_atol)
    if rank == 0 and mlp.gate_up.grad is not None and mlp.gate_up.grad[1].abs().max().item() != 0:
        fails.append("the empty expert's weight gradient is not zero")
    del recv, out, h

    # ---- module path ----------------------------------------------------------------
    torch.manual_seed(4242)                                  # the same router and experts everywhere
    layer = RoutedMoE(dev, DM, DFF, E, K, cap)
    router = torch.randn(E, DM, generator=torch.Generator(device=DEV).manual_seed(77), device=DEV) / DM ** 0.5
    with torch.no_grad():
        layer.router.copy_(router)
        layer.experts.gate_up.copy_(GU[rank * EL:(rank + 1) * EL])
        layer.experts.down.copy_(DN[rank * EL:(rank + 1) * EL])
    xm = data[rank][0].clone().requires_grad_()
    gm = (data[rank][3].float() * MODULE_G).bfloat16()
    out = layer(xm)
    (out * gm).sum().backward()
    torch.cuda.synchronize()
    dev.check()
    idx = layer.last_handle.topk_idx.long()
    x64 = data[rank][0].double().requires_grad_()
    r64 = router.double().requires_grad_()
    probs = torch.softmax(x64 @ r64.T, dim=-1)
    w64 = probs.gather(1, idx)
    w64 = w64 / w64.sum(dim=-1, keepdim=True)
    (dense_layer(x64, idx, w64, GU.double(), DN.double()) * gm.double()).sum().backward()
    rg = layer.router.grad
    if rg is None or not torch.isfinite(rg).all() or rg.abs().max().item() == 0:
        fails.append("module: the router gradient is missing, not finite or zero")
    if not torch.equal(idx, probs.topk(K, dim=-1).indices) and rank == 0:
        print("[rank 0] module: the fp64 top-k differs from the forward's (a tie); the forward's is used", flush=True)
    check("module x.grad", xm.grad, x64.grad, 3 * GEMM[0] + COMBINE[0], 3 * GEMM[1] + COMBINE[1])
    check("module router.grad", rg, r64.grad, 2 * GEMM[0] + 2e-3, 2 * GEMM[1] + 2e-3 * xm.shape[0] ** 0.5)

    torch.cuda.synchronize()
    dev.check()
    bad = comm.comm.allreduce(len(fails), op=MPI.SUM)
    if fails:
        print(f"[rank {rank}] " + "\n".join(fails[:20]), flush=True)
    if rank == 0:
        print(f"moe train OK ({time.time() - t0:.1f}s)" if bad == 0 else f"moe train FAILED ({bad})", flush=True)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
