"""Multi-rank check of ``parallel.AdamW`` over ``DistributedDataParallel`` buckets (GPU, bf16).

    scripts/mpirun -n 2 python tests/workers/optim_worker.py --tp 2     # TP = 2
    scripts/mpirun -n 2 python tests/workers/optim_worker.py --tp 1     # DP = 2
    scripts/mpirun -n 4 python tests/workers/optim_worker.py --tp 2     # DP 2 x TP 2

The model of tp_ddp_worker.py (mp-major grid from get_info) plus one replicated norm weight:
  ColumnParallelLinear(D->H) -> GELU -> RowParallelLinear(H->D) -> * norm
  -> ColumnParallelLinear(D->H, gather_output) -> RowParallelLinear(H->D, input_is_parallel=False)
Three steps of AdamW with gradient clipping.  Every step: ``clip`` is the same bits on every TP
rank; the norm is within 2^-16 of the fp64 norm of the gathered gradient (sharded parts summed
over the TP ranks, replicated parts counted once); every rank's update is the fp32 mirror of its
own buckets and the measured coefficient, bit for bit.  Afterwards: replicated parameters are the
same bits on every TP rank, all parameters on every DP rank, and on 4 ranks the weights are those
of a single-process fp32 ``torch.optim.AdamW`` + ``clip_grad_norm_`` within the relative Frobenius
tolerance tp_ddp_worker.py uses for its weights.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", ".."))
from collective_communication_mpi_amd import MPI, Communicator, get_info, ops, parallel  # noqa: E402
from collective_communication_mpi_amd.parallel import (  # noqa: E402
    ColumnParallelLinear, DistributedDataParallel, RowParallelLinear)
from collective_communication_mpi_amd.parallel.tensor_parallel import _init_full, full_weight  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--tp", type=int, default=2)
args = ap.parse_args()
comm = Communicator(MPI.COMM_WORLD)
rank, world = comm.Get_rank(), comm.Get_size()
tp = args.tp
dp = world // tp
D, H, S, per = 64, 128, 4, 3
LR, BETAS, EPS, WD, MAX_NORM, STEPS = 1e-3, (0.9, 0.999), 1e-8, 0.1, 0.01, 3  # the norm is near 0.03: clipping is active
TOL = 6e-2  # tp_ddp_worker.py's relative Frobenius tolerance for bf16 weights
mp_idx, dp_idx, mp_comm, dp_comm, _, _ = get_info(comm, rank, tp, dp, "fc_q", D, H)
torch.cuda.set_device(0 if torch.cuda.device_count() == 1 else rank % torch.cuda.device_count())
dev, dt = torch.device("cuda"), torch.bfloat16


def norm_init():
    return 0.5 + torch.rand(D, generator=torch.Generator().manual_seed(9))


class TPModel(torch.nn.Module):
    def __init__(self):
        super().__init__()
        kw = dict(device=dev, dtype=dt)
        self.c1 = ColumnParallelLinear(D, H, mp_comm, seed=1, **kw)
        self.r1 = RowParallelLinear(H, D, mp_comm, seed=2, **kw)
        self.norm = torch.nn.Parameter(norm_init().to(dev, dt))
        self.c2 = ColumnParallelLinear(D, H, mp_comm, gather_output=True, seed=3, **kw)
        self.r2 = RowParallelLinear(H, D, mp_comm, input_is_parallel=False, seed=4, **kw)

    def forward(self, x):
        return self.r2(self.c2(self.r1(torch.nn.functional.gelu(self.c1(x))) * self.norm))


class RefModel(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.ls = torch.nn.ModuleList()
        for seed, (i, o) in zip((1, 2, 3, 4), ((D, H), (H, D), (D, H), (H, D))):
            lin = torch.nn.Linear(i, o)
            w, b = _init_full(o, i, seed, torch.float32, True)
            with torch.no_grad():
                lin.weight.copy_(w.to(dt).float())
                lin.bias.copy_(b.to(dt).float())
            self.ls.append(lin)
        self.norm = torch.nn.Parameter(norm_init().to(dt).float())

    def forward(self, x):
        c1, r1, c2, r2 = self.ls
        return r2(c2(r1(torch.nn.functional.gelu(c1(x))) * self.norm))


def rel(a, b):
    return ((a.float().cpu() - b.float().cpu()).norm() / b.float().cpu().norm().clamp_min(1e-12)).item()


def same_everywhere(hc, t):
    parts = hc.allgather(t.detach().cpu().contiguous().view(torch.uint8))
    return all(torch.equal(parts[0], q) for q in parts)


model = DistributedDataParallel(TPModel(), dp_comm, bucket_bytes=16 << 10)
opt = parallel.AdamW(model, LR, BETAS, EPS, WD, max_grad_norm=MAX_NORM, tp=mp_comm)
ref = RefModel()
decayed = [q for q in ref.parameters() if q.ndim >= 2]
plain = [q for q in ref.parameters() if q.ndim < 2]
ropt = torch.optim.AdamW([dict(params=decayed, weight_decay=WD), dict(params=plain, weight_decay=0.0)], lr=LR, betas=BETAS,
                         eps=EPS)
names = {id(q): n for n, q in model.module.named_parameters()}
fails = []
flagged = {n: f for s in opt.states for n, f in zip(s.names, s.flags)}
want_sharded = {"c1.weight", "c1.bias", "r1.weight", "c2.weight", "c2.bias", "r2.weight"} if tp > 1 else set()
got_sharded = {n for n, f in flagged.items() if f & ops.OPTIM_SHARDED}
if got_sharded != want_sharded:
    fails.append(f"sharded set {sorted(got_sharded)} != {sorted(want_sharded)}")
if {n for n, f in flagged.items() if f & ops.OPTIM_DECAY} != {n for n in flagged if n.endswith(".weight")}:
    fails.append("decay set is not the weights")
g = torch.Generator().manual_seed(123)
worst_norm = 0.0
for step in range(1, STEPS + 1):
    xg = torch.randn(dp * per, S, D, generator=g)
    xl = xg[dp_idx * per:(dp_idx + 1) * per]
    model.zero_grad()
    out = model(xl.to(dev, dt))
    (out.float() ** 2).mean().backward()
    model.finish()
    before = [(s.buf.cpu(), s.p32.cpu(), s.m.cpu(), s.v.cpu()) for s in opt.states]
    opt.step()
    clip = opt.clip.cpu()
    norm, coef = clip[0].item(), clip[1]
    # --- the norm: sharded squares summed over the TP ranks, replicated ones counted once
    grads, flags = [], []
    for s, (gb, _, _, _) in zip(opt.states, before):
        for lo, hi, f in zip(s.offsets, s.offsets[1:], s.flags):
            grads.append(gb[lo:hi])
            flags.append(bool(f & ops.OPTIM_SHARDED))
    _, sh, rep = ops.grad_norm_reference(grads, flags)
    exact = (sum(mp_comm.comm.allgather(sh)) + rep) ** 0.5
    ratio = abs(norm - exact) / (2.0 ** -16 * exact)
    worst_norm = max(worst_norm, ratio)
    if not ratio <= 1.0:
        fails.append(f"step {step}: norm {norm!r} against {exact!r}: {ratio:.3f} of the bound")
    if not same_everywhere(mp_comm.comm, clip):
        fails.append(f"step {step}: clip differs across the TP ranks")
    if not same_everywhere(dp_comm.comm, clip):
        fails.append(f"step {step}: clip differs across the DP ranks")
    # --- the update: the fp32 mirror of this rank's buckets and the measured coefficient
    sched = ops.optim_sched(LR, BETAS, WD, step)
    for i, (s, (gb, p0, m0, v0)) in enumerate(zip(opt.states, before)):
        decays = torch.cat([torch.full((hi - lo,), bool(f & ops.OPTIM_DECAY))
                            for lo, hi, f in zip(s.offsets, s.offsets[1:], s.flags)])
        p, m, v = ops.adamw_reference(gb, p0, m0, v0, sched, coef, BETAS, EPS, decays)
        for what, got, want in (("p32", s.p32, p), ("m", s.m, m), ("v", s.v, v)):
            if not torch.equal(got.cpu().view(torch.int32), want.view(torch.int32)):
                fails.append(f"step {step} bucket {i}: {what} is not the mirror's")
        for q, lo, hi in zip(s.params, s.offsets, s.offsets[1:]):
            if not torch.equal(q.detach().cpu().reshape(-1).view(torch.int16), p[lo:hi].to(dt).view(torch.int16)):
                fails.append(f"step {step}: {names[id(q)]} is not bf16(master)")
    # --- the reference
    ropt.zero_grad()
    (ref(xg.to(dt).float()) ** 2).mean().backward()
    rnorm = torch.nn.utils.clip_grad_norm_(ref.parameters(), MAX_NORM).item()
    ropt.step()
    if abs(norm - rnorm) > TOL * rnorm:
        fails.append(f"step {step}: norm {norm:.5f} against the fp32 reference's {rnorm:.5f}")
    last = (norm, coef.item(), rnorm)
    if not 0.0 < last[1] < 1.0:
        fails.append(f"step {step}: the test means to clip, coef = {last[1]}")
# --- after three steps
replicated = torch.cat([q.detach().reshape(-1) for n, q in model.module.named_parameters() if n not in got_sharded])
if not same_everywhere(mp_comm.comm, replicated):
    fails.append("replicated parameters differ across the TP ranks")
everything = torch.cat([q.detach().reshape(-1) for q in model.module.parameters()])
if not same_everywhere(dp_comm.comm, everything):
    fails.append("parameters differ across the DP ranks")
worst_w = 0.0
for name, lyr, rl in (("c1", model.module.c1, ref.ls[0]), ("r1", model.module.r1, ref.ls[1]),
                      ("c2", model.module.c2, ref.ls[2]), ("r2", model.module.r2, ref.ls[3])):
    e = rel(full_weight(lyr, mp_comm), rl.weight.detach())
    worst_w = max(worst_w, e)
    if e > TOL:
        fails.append(f"{name} weight after {STEPS} AdamW steps rel err {e:.2e}")
e = rel(model.module.norm.detach(), ref.norm.detach())
if e > TOL:
    fails.append(f"norm weight after {STEPS} AdamW steps rel err {e:.2e}")
if len(opt.states) < 2:
    fails.append(f"expected several buckets, got {model.bucket_sizes}")
comm.Barrier()
if fails:
    print(f"[rank {rank}] FAIL: {fails}", flush=True)
    sys.exit(1)
if rank == 0:
    print(f"optim OK world={world} tp={tp} dp={dp} buckets={len(opt.states)} norm={last[0]:.5f} coef={last[1]:.5f} "
          f"reference norm={last[2]:.5f} worst norm ratio={worst_norm:.3f} worst weight rel err={worst_w:.2e}", flush=True)
