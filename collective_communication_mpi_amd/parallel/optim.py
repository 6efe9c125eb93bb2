"""AdamW over the gradient buckets of ``DistributedDataParallel``, with the global gradient norm
computed and applied on the device (csrc/device/optim.hip through ``ops.optim_*``).

``DistributedDataParallel`` leaves every gradient, DP-averaged, in flat buckets; ``AdamW`` consumes
them in place.  Per bucket it keeps flat fp32 state indexed like the bucket -- master weights
``p32`` (bf16 buckets; an fp32 parameter is its own master), ``exp_avg`` and ``exp_avg_sq`` -- and a
segment table (offset, parameter address, flags) on the device.  A step is

    ddp.finish()
    opt.step(lr)            # = opt.advance(lr); opt.launch()

``advance`` is host only: ``t += 1`` and ``(lr, 1 - b1^t, 1 - b2^t, 1 - lr wd)``, computed in fp64,
sent to the device by one asynchronous copy from pinned memory.  ``launch`` runs kernels only and
can be captured in a graph: with ``max_grad_norm``, per bucket the slot sums of squares and their
fp64 sum (split into tensor-parallel sharded and replicated parameters), one rank-ordered fp64
all-reduce of the sharded sums over ``tp``, the clip coefficient ``min(1, max / (norm + 1e-6))``,
then per bucket the update, which reads the coefficient from the device.  Nothing synchronises with
the host; ``grad_norm`` is a device view.

Under tensor parallelism a sharded parameter's squares are summed over the TP ranks and a
replicated parameter's (norms, the embedding, row-parallel biases: identical gradients on every
rank) are counted once, so every rank gets the same norm, bit for bit, and replicated parameters
stay identical.

Out of scope: sharding the state over DP, parameters sharded over another group than ``tp`` (expert
parallelism), loss scaling or skipping a step on a non-finite norm (it propagates, as in torch),
zeroing the gradients.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import torch

from .. import ops
from .ddp import DistributedDataParallel
from .layout import _host_comm, device_group_for

_SCHED_RING = 8  # pinned (lr, bc1, bc2, decay) rows in flight


class _State:
    """One bucket's optimizer state."""

    __slots__ = ("bucket", "buf", "names", "params", "offsets", "flags", "ptrs", "seg_off", "seg_ptr", "seg_flags",
                 "p32", "m", "v")


class AdamW:
    """``parallel.AdamW(ddp, lr, ...)``: fused AdamW with fp32 master weights and moments over
    ``ddp``'s buckets.  ``decay(name, p)`` says which parameters get weight decay (default: those
    with two or more dimensions).  ``tp`` is the tensor-parallel communicator of the model's
    layers; ``sharded`` says which parameters are sharded over it: None (default: the weights and
    biases of ``ColumnParallelLinear`` and the weights of ``RowParallelLinear`` layers whose own
    group has more than one rank), a callable ``(name, p) -> bool``, or a collection of names."""

    def __init__(self, ddp: DistributedDataParallel, lr: float, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.0, max_grad_norm: Optional[float] = None, tp=None,
                 decay=lambda name, p: p.ndim >= 2, sharded=None):
        if not isinstance(ddp, DistributedDataParallel):
            raise TypeError(f"parallel.AdamW takes a DistributedDataParallel, got {type(ddp).__name__}")
        if ddp.device.type != "cuda":
            raise ValueError("parallel.AdamW: the kernels run on the GPU; the model is on " + str(ddp.device))
        self.ddp = ddp
        self.device = ddp.device
        self.betas = (float(betas[0]), float(betas[1]))
        self.eps = float(eps)
        self.lr = float(lr)
        self.weight_decay = float(weight_decay)
        ops.optim_sched(self.lr, self.betas, self.weight_decay, 1)  # the argument rules
        if not 0.0 <= self.eps < float("inf"):
            raise ValueError(f"parallel.AdamW: eps must be non-negative and finite, got {eps!r}")
        self.max_grad_norm = None if max_grad_norm is None else ops.kernels._optim_max_norm(max_grad_norm)
        self.t = 0
        self.tp = tp
        self.tp_size = 1 if tp is None else _host_comm(tp).Get_size()
        self.tpdev = device_group_for(tp) if self.tp_size > 1 else None
        name_of = {id(q): name for name, q in ddp.module.named_parameters()}
        is_sharded = self._sharded_rule(sharded)
        self.states: List[_State] = []
        for b in ddp.buckets:
            self.states.append(self._make_state(b, name_of, decay, is_sharded))
        dev = self.device
        nb = len(self.states)
        nbp = (nb + 1) // 2 * 2  # rows of whole 16 bytes; the padding stays zero
        self.partials = torch.zeros(max(ops.optim_slots(s.buf.numel(), len(s.params)) for s in self.states),
                                    dtype=torch.float32, device=dev)
        if self.tpdev is not None:
            # rows: this rank's sharded sums, their all-reduce over tp, the replicated sums
            blk = self.tpdev.zeros((3, nbp), torch.float64)
            self._sums_local, self._sums_all = blk[0::2], blk[1:3]
            self._sums_block = blk
        else:
            self._sums_block = torch.zeros((2, nbp), dtype=torch.float64, device=dev)
            self._sums_local = self._sums_all = self._sums_block
        self.clip = torch.zeros(2, dtype=torch.float32, device=dev)
        self.sched = torch.zeros(4, dtype=torch.float32, device=dev)
        self._sched_host = torch.zeros((_SCHED_RING, 4), dtype=torch.float32).pin_memory()
        self._sched_events: List[Optional[torch.cuda.Event]] = [None] * _SCHED_RING

    # ------------------------------------------------------------------ setup
    def _sharded_rule(self, sharded):
        if sharded is None:
            if self.tp_size == 1:
                return lambda name, q: False
            from .tensor_parallel import ColumnParallelLinear, RowParallelLinear

            ids = set()
            for mod in self.ddp.module.modules():
                if isinstance(mod, ColumnParallelLinear) and mod.p > 1:
                    ids.add(id(mod.weight))
                    if mod.bias is not None:
                        ids.add(id(mod.bias))
                elif isinstance(mod, RowParallelLinear) and mod.p > 1:
                    ids.add(id(mod.weight))
            return lambda name, q: id(q) in ids
        if callable(sharded):
            return sharded
        names = set(sharded)
        return lambda name, q: name in names

    def _make_state(self, b, name_of: Dict[int, str], decay, is_sharded) -> _State:
        buf = b.buf
        if buf.dtype not in (torch.bfloat16, torch.float32):
            raise TypeError(f"parallel.AdamW: buckets are bf16 or fp32, got {buf.dtype}")
        s = _State()
        s.bucket, s.buf, s.params = b, buf, list(b.params)
        s.names = [name_of[id(q)] for q in s.params]
        s.offsets, s.flags = [0], []
        for name, q in zip(s.names, s.params):
            if not q.is_contiguous() or q.numel() < 1:
                raise ValueError(f"parallel.AdamW: parameter {name} is empty or not contiguous")
            if q.dtype != buf.dtype or q.device != buf.device:
                raise ValueError(f"parallel.AdamW: parameter {name} ({q.dtype}, {q.device}) does not match its bucket")
            s.offsets.append(s.offsets[-1] + q.numel())
            s.flags.append((ops.OPTIM_DECAY if decay(name, q) else 0) | (ops.OPTIM_SHARDED if is_sharded(name, q) else 0))
        n, dev = buf.numel(), buf.device
        s.seg_off = torch.tensor(s.offsets, dtype=torch.int64).to(dev)
        s.seg_flags = torch.tensor(s.flags, dtype=torch.int32).to(dev)
        s.ptrs = [q.data_ptr() for q in s.params]
        s.seg_ptr = torch.tensor(s.ptrs, dtype=torch.int64).to(dev)
        s.m = torch.zeros(n, dtype=torch.float32, device=dev)
        s.v = torch.zeros(n, dtype=torch.float32, device=dev)
        if buf.dtype == torch.bfloat16:
            s.p32 = torch.empty(n, dtype=torch.float32, device=dev)
            with torch.no_grad():
                for q, lo, hi in zip(s.params, s.offsets, s.offsets[1:]):
                    s.p32[lo:hi].copy_(q.detach().reshape(-1))
        else:
            s.p32 = None
        return s

    def _check_table(self) -> None:
        """Every parameter's storage is still where its table says (host only); a table whose
        parameters moved (``.data`` replaced, a loaded checkpoint) is rebuilt."""
        for s in self.states:
            ptrs = [q.data_ptr() for q in s.params]
            if ptrs != s.ptrs:
                for name, q in zip(s.names, s.params):
                    if not q.is_contiguous() or q.dtype != s.buf.dtype:
                        raise ValueError(f"parallel.AdamW: parameter {name} is no longer a contiguous {s.buf.dtype} tensor")
                s.ptrs = ptrs
                s.seg_ptr.copy_(torch.tensor(ptrs, dtype=torch.int64))

    # ------------------------------------------------------------------- step
    def advance(self, lr: Optional[float] = None) -> None:
        """Host only: ``t += 1`` (and a new learning rate), then this step's ``(lr, bc1, bc2,
        decay)`` to the device through one asynchronous copy from pinned memory."""
        if lr is not None:
            self.lr = float(lr)
        vals = ops.optim_sched(self.lr, self.betas, self.weight_decay, self.t + 1)
        self.t += 1
        k = self.t % _SCHED_RING
        if self._sched_events[k] is not None:
            self._sched_events[k].synchronize()  # the copy of step t - 8 has long been done
        self._sched_host[k].copy_(vals)
        self.sched.copy_(self._sched_host[k], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        self._sched_events[k] = ev

    def launch(self) -> None:
        """Kernels only (capturable on one rank): the norm and the clip coefficient when
        ``max_grad_norm`` is set, then the update of every bucket."""
        self._check_table()
        clip = None
        if self.max_grad_norm is not None:
            for i, s in enumerate(self.states):
                ops.optim_sqsum(s.buf, s.seg_off, s.seg_flags, self.partials, self._sums_local, i)
            if self.tpdev is not None:
                # rank order: every TP rank gets the same bits
                self.tpdev.allreduce(self._sums_block[0], self._sums_block[1], "SUM", "oneshot", symmetric=True)
            clip = ops.optim_clip(self._sums_all, self.max_grad_norm, self.clip)
        for s in self.states:
            ops.optim_adamw_update(s.buf, s.seg_off, s.seg_ptr, s.seg_flags, s.p32, s.m, s.v, self.sched, clip,
                                   self.betas, self.eps)

    def step(self, lr: Optional[float] = None) -> None:
        """``advance(lr)`` and ``launch()``; call after ``ddp.finish()``."""
        self.advance(lr)
        self.launch()

    @property
    def grad_norm(self) -> Optional[torch.Tensor]:
        """The unclipped global gradient norm of the last step: a [1] fp32 device view (reading
        it is the only synchronisation); None without ``max_grad_norm``."""
        return None if self.max_grad_norm is None else self.clip[0:1]

    @property
    def clip_coef(self) -> Optional[torch.Tensor]:
        """``min(1, max_grad_norm / (norm + 1e-6))`` of the last step: a [1] fp32 device view."""
        return None if self.max_grad_norm is None else self.clip[1:2]

    # ------------------------------------------------------------------ state
    def _entries(self):
        for s in self.states:
            for name, q, lo, hi in zip(s.names, s.params, s.offsets, s.offsets[1:]):
                yield s, name, q, lo, hi

    def state_dict(self) -> dict:
        """``{"step": t, "state": {name: {"master", "exp_avg", "exp_avg_sq"}}}``: fp32 copies in the
        parameter's shape, keyed by parameter name, so the state does not depend on ``bucket_bytes``."""
        state = {}
        for s, name, q, lo, hi in self._entries():
            master = q.detach().clone() if s.p32 is None else s.p32[lo:hi].clone().view_as(q)
            state[name] = {"master": master, "exp_avg": s.m[lo:hi].clone().view_as(q),
                           "exp_avg_sq": s.v[lo:hi].clone().view_as(q)}
        return {"step": self.t, "state": state}

    def load_state_dict(self, sd: dict) -> None:
        """Takes ``state_dict()``'s form; the parameters are set from the master weights."""
        state = sd["state"]
        missing = [name for _, name, _, _, _ in self._entries() if name not in state]
        if missing or len(state) != sum(len(s.params) for s in self.states):
            raise KeyError(f"parallel.AdamW.load_state_dict: the state's parameter names do not match the model's "
                           f"(missing: {missing[:4]})")
        with torch.no_grad():
            for s, name, q, lo, hi in self._entries():
                e = state[name]
                for t in e.values():
                    if tuple(t.shape) != tuple(q.shape) or t.dtype != torch.float32:
                        raise ValueError(f"parallel.AdamW.load_state_dict: {name} expects fp32 {tuple(q.shape)} tensors")
                s.m[lo:hi].copy_(e["exp_avg"].reshape(-1))
                s.v[lo:hi].copy_(e["exp_avg_sq"].reshape(-1))
                if s.p32 is not None:
                    s.p32[lo:hi].copy_(e["master"].reshape(-1))
                q.copy_(e["master"])  # bf16: one rounding to nearest even, as the kernel stores it
        self.t = int(sd["step"])


__all__ = ["AdamW"]
