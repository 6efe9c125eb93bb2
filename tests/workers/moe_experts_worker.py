"""moe_dispatch -> GroupedExpertsMLP -> moe_combine on p ranks sharing the GPU.

D = 128, d_ff = 64, two local experts per rank, K = 2, T = 100 + 7 * rank tokens.  The
routing is skewed: every token's first slot goes to expert 0 (rank 0's first expert gets
every token of every rank, well over one 128-row tile) and nobody chooses expert 1 (rank
0's second expert is empty); second slots spread over the other experts, some dropped.
Every rank rebuilds every rank's tokens, routing, combine weights and all expert weights
from shared seeds and evaluates the layer densely in fp64, per token.

Tolerance: the weighted combine alone is held to rtol = 1e-2 * K, atol = 4e-2 * K in bf16
(moe_worker.check_close); the two bf16 GEMMs in front of it each add the grouped forward's
rtol 2e-2 / atol 8e-2: rtol 6e-2, atol 2.4e-1 at K = 2.  The worst error is printed
(measured on an MI355X: 0.026 absolute at |ref| up to 5.6, 7 % of the tolerance at worst).
On 2 ranks the three calls are also captured in one graph and replayed with new tokens and
routing.  Prints "moe experts OK" on success."""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", ".."))
from collective_communication_mpi_amd import MPI, Communicator  # noqa: E402
from collective_communication_mpi_amd.parallel import GroupedExpertsMLP  # noqa: E402

comm = Communicator(MPI.COMM_WORLD)
rank, p = comm.Get_rank(), comm.Get_size()
dev = comm.dev
DEV = dev.device
DM, DFF, EL, K = 128, 64, 2, 2
E = EL * p
RTOL, ATOL = 1e-2 * K + 2 * 2e-2, 4e-2 * K + 2 * 8e-2
fails = []


def tokens(r, salt):
    """Rank r's (x, topk_idx, combine weights): identical on every rank that asks."""
    T = 100 + 7 * r
    g = torch.Generator(device=DEV).manual_seed(40_009 * (salt + 1) + 977 * r + 5)
    x = torch.randn(T, DM, generator=g, device=DEV).bfloat16()
    first = torch.zeros(T, 1, dtype=torch.int64, device=DEV) if salt == 0 else \
        torch.full((T, 1), E - 1, dtype=torch.int64, device=DEV)      # the replay overloads the last expert
    second = torch.randint(2, E, (T, 1), generator=g, device=DEV) if salt == 0 else \
        torch.randint(0, E - 2, (T, 1), generator=g, device=DEV)      # ... and leaves expert E - 2 empty
    second[torch.rand(T, 1, generator=g, device=DEV) < 0.1] = -1      # some dropped slots
    w = torch.rand(T, K, generator=g, device=DEV) + 0.25
    return x, torch.cat([first, second], dim=1), w


def expert_weights():
    g = torch.Generator(device=DEV).manual_seed(123_457)
    gu = (torch.randn(E, 2 * DFF, DM, generator=g, device=DEV) / DM ** 0.5).bfloat16()
    dn = (torch.randn(E, DM, DFF, generator=g, device=DEV) / DFF ** 0.5).bfloat16()
    return gu, dn


GU, DN = expert_weights()


def dense_reference(x, idx, w):
    """fp64, per token: sum_k w[t, k] * down[e] . swiglu(gate_up[e] . x[t]), e = idx[t, k]."""
    out = torch.zeros(x.shape[0], DM, dtype=torch.float64, device=DEV)
    xd = x.double()
    for k in range(K):
        for e in range(E):
            m = idx[:, k] == e
            if not m.any():
                continue
            h = xd[m] @ GU[e].double().T
            a = torch.nn.functional.silu(h[:, 0::2]) * h[:, 1::2]
            out[m] += w[m, k:k + 1].double() * (a @ DN[e].double().T)
    return out


def check(tag, got, x, idx, w):
    want = dense_reference(x, idx, w)
    err = (got.double() - want).abs()
    ratio = (err / (ATOL + RTOL * want.abs())).max().item()
    print(f"[rank {rank}] {tag}: worst abs error {err.max().item():.4f} (|ref| max {want.abs().max().item():.2f}), "
          f"worst error / tolerance {ratio:.3f}", flush=True)
    if not ratio <= 1.0:
        fails.append(f"{tag}: error exceeds rtol {RTOL} atol {ATOL} (ratio {ratio:.3f})")


def received(idxs):
    """Rows every local expert of this rank receives (host side, from all ranks' routing)."""
    allidx = torch.cat([i.reshape(-1) for i in idxs])
    return torch.bincount(allidx[allidx >= 0], minlength=E)[rank * EL:(rank + 1) * EL].tolist()


mlp = GroupedExpertsMLP(EL, DM, DFF, device=DEV)
with torch.no_grad():
    mlp.gate_up.copy_(GU[rank * EL:(rank + 1) * EL])
    mlp.down.copy_(DN[rank * EL:(rank + 1) * EL])

data = [tokens(r, 0) for r in range(p)]
cap = sum(d[0].shape[0] for d in data) * K + 8        # host-known bound: everything lands on one rank
rows = torch.bincount(torch.cat([d[1][d[1] >= 0] for d in data]), minlength=E).tolist()
if not (max(rows) > 128 and min(rows) == 0):
    fails.append(f"routing is not skewed enough: rows per expert {rows}")

x, idx, w = (t.clone() for t in data[rank])
recv = dev.empty((cap, DM), torch.bfloat16)
y = dev.empty((cap, DM), torch.bfloat16)
out = torch.empty_like(x)
t0 = time.time()


def pipeline():
    h = dev.moe_dispatch(x, idx, E, recv)
    with torch.no_grad():
        y.copy_(mlp(recv, h.expert_counts))
    dev.moe_combine(y, h, w, out=out)
    return h


h = pipeline()
torch.cuda.synchronize()
dev.check()
if h.expert_counts.tolist() != received([d[1] for d in data]):
    fails.append(f"expert_counts {h.expert_counts.tolist()} != {received([d[1] for d in data])}")
check("eager", out, x, idx, w)

if p == 2 and dev.ranks_per_device <= 2:
    cs = torch.cuda.Stream()
    cs.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(cs):
        with torch.cuda.graph(graph, stream=cs):
            hg = pipeline()
    torch.cuda.current_stream().wait_stream(cs)
    data2 = [tokens(r, 1) for r in range(p)]
    x.copy_(data2[rank][0]); idx.copy_(data2[rank][1]); w.copy_(data2[rank][2])
    out.zero_()
    torch.cuda.synchronize()
    dev.host.Barrier()
    graph.replay()
    torch.cuda.synchronize()
    dev.check()
    if hg.expert_counts.tolist() != received([d[1] for d in data2]):
        fails.append(f"graph: expert_counts {hg.expert_counts.tolist()} != {received([d[1] for d in data2])}")
    check("graph replay", out, x, idx, w)
    del graph

torch.cuda.synchronize()
dev.check()
bad = comm.comm.allreduce(len(fails), op=MPI.SUM)
if fails:
    print(f"[rank {rank}] " + "\n".join(fails[:20]), flush=True)
if rank == 0:
    print(f"moe experts OK ({time.time() - t0:.1f}s)" if bad == 0 else f"moe experts FAILED ({bad})", flush=True)
sys.exit(1 if bad else 0)
