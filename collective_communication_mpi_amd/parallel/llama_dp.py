"""BASELINE config 5 on a real backward: "DP8 gradient all-reduce, Llama-3-8B-sized grad
(~16 GB bf16) overlapped with backward on 8xMI355X".

A Llama-3-8B-shaped decoder (token embedding, ``layers`` blocks of RMSNorm -> q/k/v/o
projections + causal GQA attention -> RMSNorm -> SwiGLU MLP, final norm, LM head: 8.03 B
weights = 16.06 GB of bf16 gradients at 32 layers) built from the framework's own layers
(``ColumnParallelLinear`` / ``RowParallelLinear`` / ``ParallelSwiGLUMLP`` at TP = 1: the
hand-written MFMA GEMMs forward and backward), wrapped in ``DistributedDataParallel`` over
the DP communicator.  ``loss.backward()`` runs the whole autograd backward (dX and dW
GEMMs, attention, norms, embedding scatter); each bucket's all-reduce is launched from
the backward itself -- by the dW GEMM that completes it (gradient sinks) or by the
post-accumulate hook -- on the communication stream, and ``finish()`` joins it.

The reference's DP is sharding plus ``dp_comm`` (data/data_parallel_preprocess.py:45-59,
model/func_impl.py:61-62, README.md:177); this is the gradient synchronisation the north
star adds on that communicator.  Attention is chosen by ``LlamaConfig.attention``: "sdpa"
(the default) is PyTorch's SDPA on transposed q/k/v with the kv heads expanded by
``repeat_interleave``; "flash" is the project's own kernel (``ops.flash_attention``,
csrc/device/flash_attn.hip), which reads the projections' [B, S, H, hd] views as they are,
never expands K or V and writes the [B * S, d] input of ``wo`` directly (head dim 64 or 128).
With ``cp`` (a communicator) and "flash" the sequence axis is split: every rank of ``cp`` runs the
model on its shard of consecutive positions and the block calls ``context_parallel_attention``
(parallel/context_parallel.py); everything else in the block is per token.  The caller passes
explicit ``targets`` (a shard's last target lives on the next rank) and averages the parameter
gradients over ``cp``.
With ``cu_seqlens`` (int32 [n + 1] on the device, "flash" without ``cp``) the batch is PACKED:
the boundaries are positions on the flattened ``batch * seq`` token axis, document ``i`` owns
tokens ``[cu_seqlens[i], cu_seqlens[i + 1])`` with ``cu_seqlens[n] = batch * seq``, and the block
calls ``ops.flash_attention_varlen``, so no token sees another document.  The caller passes explicit
``targets`` with -100 (``F.cross_entropy``'s ``ignore_index``) at each document's last token.
The loss is chosen by ``LlamaConfig.loss``: "torch" (the default) is ``F.cross_entropy`` on an fp32
copy of the logits; "fused" is the project's own kernel family (``vocab_parallel_cross_entropy``,
parallel/vocab_parallel.py, csrc/device/xent.hip): one read pass over the bf16 logits forward, one
read and one write pass backward, no fp32 [T, vocab] tensor, and -- the head being a
``ColumnParallelLinear`` over ``tp`` -- each rank reduces its own ``vocab / p`` columns and one
small all-gather combines the rows' statistics, so the logits are never gathered.  It takes
explicit ``targets``, -100 entries, ``cp`` and ``cu_seqlens`` as "torch" does; when every target is
-100 its loss is 0 with zero gradients where torch gives NaN.  A TP group of more than one rank with
a vocabulary NEEDS "fused": ``F.cross_entropy`` on a ``vocab / p``-wide shard with global targets
never computed a loss (it indexed past the shard), so that combination is refused at construction.
Under TP the block's attention runs on this rank's ``heads / p`` query and ``kv_heads / p`` key /
value heads (``p`` must divide both).
Positions: by default RoPE is left out (no effect on gradient sizes or the GEMM work) and the
model has no notion of position beyond the causal mask.  ``LlamaConfig.rope = True`` rotates q and k
(never v) right after the projections, on their [.., H, hd] views, with the project's own kernel
(``ops.rope``, csrc/device/rope.hip) in all four attention paths: "sdpa" (before the transposes),
"flash", "flash" with ``cp`` (row ``s`` of rank ``r`` sits at position ``r * seq + s``) and "flash"
with ``cu_seqlens`` (a token's position is its index inside its document, the boundaries read on
the device).  The model builds one cos / sin table of ``max_positions`` rows (``ops.rope_table``,
``rope_theta``) and shares it with its blocks; a sequence -- under ``cp`` the whole one, ``cp_size *
seq`` -- longer than that raises before any launch (a packed document longer than it is the
caller's to avoid).  With ``rope = False`` the forward never enters that code.
Norms: ``LlamaConfig.norm = "torch"`` (the default) is ``F.rms_norm`` and plain ``x + ...`` adds;
"fused" is the project's own kernel family (``ops.rms_norm`` / ``ops.add_rms_norm``,
csrc/device/rmsnorm.hip) in all four attention paths: every residual add is computed by the norm
that follows it (a block hands its MLP output on as a pending addend, which the next block's
``attn_norm`` or the model's final ``norm`` adds), and the norm weights' gradients are summed in a
fixed order.  Random-init weights, synthetic token ids.
"""
from __future__ import annotations

import time
from dataclasses import dataclass
from typing import Dict, List, Optional

import torch
import torch.nn.functional as F

from ..ops.kernels import (FLASH_HEAD_DIMS, RMS_NORM_MAX_D, add_rms_norm, flash_attention, flash_attention_varlen,
                           rms_norm, rope, rope_table)
from .context_parallel import context_parallel_attention
from .ddp import DistributedDataParallel
from .tensor_parallel import ColumnParallelLinear, ParallelSwiGLUMLP, RowParallelLinear, _size_rank
from .vocab_parallel import vocab_parallel_cross_entropy


@dataclass
class LlamaConfig:
    d: int = 4096
    heads: int = 32
    kv_heads: int = 8
    ffn: int = 14336
    vocab: int = 128256
    layers: int = 32
    eps: float = 1e-5
    attention: str = "sdpa"  # "sdpa" (PyTorch) or "flash" (ops.flash_attention, head dim 64 / 128)
    loss: str = "torch"  # "torch" (F.cross_entropy on fp32 logits) or "fused" (vocab_parallel_cross_entropy)
    rope: bool = False  # rotate q and k by their positions (ops.rope); False: no notion of position
    rope_theta: float = 500000.0
    max_positions: int = 8192  # rows of the cos / sin table: the longest sequence rope=True accepts
    norm: str = "torch"  # "torch" (F.rms_norm, x + ... adds) or "fused" (ops.rms_norm / ops.add_rms_norm)

    @property
    def head_dim(self) -> int:
        return self.d // self.heads

    def params(self, vocab: bool = True) -> int:
        d, kv = self.d, self.kv_heads * self.head_dim
        per_layer = d * d * 2 + 2 * kv * d + 3 * self.ffn * d + 2 * d
        return per_layer * self.layers + d + (2 * self.vocab * d if vocab else 0)


LLAMA3_8B = LlamaConfig()
ATTENTION_KINDS = ("sdpa", "flash")
LOSS_KINDS = ("torch", "fused")
NORM_KINDS = ("torch", "fused")


class RMSNorm(torch.nn.Module):
    def __init__(self, d: int, eps: float, device=None, dtype=torch.bfloat16):
        super().__init__()
        self.eps = eps
        self.weight = torch.nn.Parameter(torch.ones(d, device=device, dtype=dtype))

    def forward(self, x):
        return F.rms_norm(x, (x.shape[-1],), self.weight, self.eps)


def _check_rope_config(cfg: LlamaConfig) -> None:
    if not cfg.rope:
        return
    if cfg.head_dim % 16 or not 16 <= cfg.head_dim <= 256:
        raise ValueError(f"rope=True needs a head dim that is a multiple of 16 in [16, 256], got {cfg.head_dim}")
    if isinstance(cfg.max_positions, bool) or not isinstance(cfg.max_positions, int) or cfg.max_positions < 1:
        raise ValueError(f"LlamaConfig.max_positions must be a positive int, got {cfg.max_positions!r}")
    if not cfg.rope_theta > 0:
        raise ValueError(f"LlamaConfig.rope_theta must be positive, got {cfg.rope_theta!r}")


def _check_norm_config(cfg: LlamaConfig) -> None:
    if cfg.norm not in NORM_KINDS:
        raise ValueError(f"LlamaConfig.norm must be one of {NORM_KINDS}, got {cfg.norm!r}")
    if cfg.norm == "fused" and (cfg.d % 8 or not 8 <= cfg.d <= RMS_NORM_MAX_D):
        raise ValueError(f'norm="fused" needs d to be a multiple of 8 in [8, {RMS_NORM_MAX_D}], got {cfg.d}')


class LlamaBlock(torch.nn.Module):
    def __init__(self, cfg: LlamaConfig, tp, seed: int, device, dtype=torch.bfloat16, cp=None, rope_table=None):
        super().__init__()
        d, kv = cfg.d, cfg.kv_heads * cfg.head_dim
        self.cfg = cfg
        self.cp = cp  # context-parallel communicator: x holds this rank's shard of the sequence
        _check_rope_config(cfg)
        _check_norm_config(cfg)
        if cfg.rope and rope_table is None:
            raise ValueError("LlamaConfig.rope needs the model's cos / sin table (rope_table)")
        self.rope_table = rope_table if cfg.rope else None  # shared by every block: a plain attribute, no buffer
        if cfg.attention not in ATTENTION_KINDS:
            raise ValueError(f"LlamaConfig.attention must be one of {ATTENTION_KINDS}, got {cfg.attention!r}")
        if cfg.attention == "flash" and cfg.head_dim not in FLASH_HEAD_DIMS:
            raise ValueError(f'attention="flash" needs a head dim in {FLASH_HEAD_DIMS}, got {cfg.head_dim}')
        if cp is not None and cfg.attention != "flash":
            raise ValueError(f'context parallelism (cp) needs attention="flash", got {cfg.attention!r}')
        p = _size_rank(tp)[0]
        if cfg.heads % p or cfg.kv_heads % p:
            raise ValueError(f"the TP size {p} must divide heads ({cfg.heads}) and kv_heads ({cfg.kv_heads})")
        self.heads, self.kv_heads = cfg.heads // p, cfg.kv_heads // p  # this rank's heads
        self.cp_size, self.cp_rank = _size_rank(cp) if cfg.rope and cp is not None else (1, 0)
        kw = dict(bias=False, device=device, dtype=dtype, init="device")
        self.attn_norm = RMSNorm(d, cfg.eps, device, dtype)
        self.wq = ColumnParallelLinear(d, d, tp, seed=seed, **kw)
        self.wk = ColumnParallelLinear(d, kv, tp, seed=seed + 1, **kw)
        self.wv = ColumnParallelLinear(d, kv, tp, seed=seed + 2, **kw)
        self.wo = RowParallelLinear(d, d, tp, seed=seed + 3, **kw)
        self.mlp_norm = RMSNorm(d, cfg.eps, device, dtype)
        self.mlp = ParallelSwiGLUMLP(d, cfg.ffn, tp, device=device, dtype=dtype, seed=seed + 4, init="device")

    def check_positions(self, seq: int, cu_seqlens=None) -> None:
        """rope: the whole sequence (``cp_size * seq``) fits the table.  Packed documents are not
        checked: their lengths live on the device (the kernel clamps the table row)."""
        cfg = self.cfg
        if cfg.rope and cu_seqlens is None and self.cp_size * seq > cfg.max_positions:
            raise ValueError(f"rope: {self.cp_size} x {seq} positions exceed LlamaConfig.max_positions = "
                             f"{cfg.max_positions}")

    def _enter(self, x, addend):
        """(residual stream, attn_norm of it).  norm="fused": the previous block's pending addend is
        added by this norm's kernel."""
        if self.cfg.norm != "fused":
            return x, self.attn_norm(x)
        if addend is None:
            return x, rms_norm(x, self.attn_norm.weight, self.attn_norm.eps)
        return add_rms_norm(x, addend, self.attn_norm.weight, self.attn_norm.eps)

    def _leave(self, x, attn_out):
        """The block's second half.  norm="fused": the pair (residual stream, pending addend), the
        MLP output left for the next norm to add."""
        if self.cfg.norm != "fused":
            h = x + attn_out
            return h + self.mlp(self.mlp_norm(h))
        h, n = add_rms_norm(x, attn_out, self.mlp_norm.weight, self.mlp_norm.eps)
        return h, self.mlp(n)

    def forward(self, x, batch: int, seq: int, cu_seqlens: Optional[torch.Tensor] = None, addend=None):
        """norm="torch": the block's output.  norm="fused": takes the pair (``x``, ``addend``: the
        residual stream and what is still to be added to it, None at the first block) and returns
        such a pair."""
        cfg = self.cfg
        if addend is not None and cfg.norm != "fused":
            raise ValueError('a pending addend needs norm="fused"')
        hd, hq, hkv = cfg.head_dim, self.heads, self.kv_heads
        self.check_positions(seq, cu_seqlens)  # before any launch of this block
        if cu_seqlens is not None:  # packed documents: boundaries on the flattened batch * seq token axis
            if cfg.attention != "flash" or self.cp is not None:
                raise ValueError('cu_seqlens needs attention="flash" and no context parallelism (cp), got '
                                 f"attention={cfg.attention!r}, cp {'set' if self.cp is not None else 'None'}")
            x, n = self._enter(x, addend)
            q, k = self.wq(n).view(batch * seq, hq, hd), self.wk(n).view(batch * seq, hkv, hd)
            if cfg.rope:  # a token's position is its index inside its document
                q, k = rope(q, k, self.rope_table, cu_seqlens=cu_seqlens)
            o = flash_attention_varlen(q, k, self.wv(n).view(batch * seq, hkv, hd), cu_seqlens, causal=True)
            return self._leave(x, self.wo(o.view(batch * seq, hq * hd)))
        x, n = self._enter(x, addend)
        if cfg.attention == "flash":  # the projections' views as they are; K and V stay at kv_heads
            q, k, v = (self.wq(n).view(batch, seq, hq, hd), self.wk(n).view(batch, seq, hkv, hd),
                       self.wv(n).view(batch, seq, hkv, hd))
            if cfg.rope:  # under cp this rank's rows start at position cp_rank * seq
                q, k = rope(q, k, self.rope_table, pos0=self.cp_rank * seq)
            if self.cp is not None:  # seq is this rank's shard; K | V of the other shards are gathered
                o = context_parallel_attention(self.cp, q, k, v, causal=True)
            else:
                o = flash_attention(q, k, v, causal=True)
            return self._leave(x, self.wo(o.view(batch * seq, hq * hd)))
        q, k = self.wq(n).view(batch, seq, hq, hd), self.wk(n).view(batch, seq, hkv, hd)
        if cfg.rope:
            q, k = rope(q, k, self.rope_table)
        q, k = q.transpose(1, 2), k.transpose(1, 2)
        v = self.wv(n).view(batch, seq, hkv, hd).transpose(1, 2)
        rep = hq // hkv
        if rep > 1:  # GQA: expand the kv heads (keeps SDPA on its fused path)
            k = k.repeat_interleave(rep, dim=1)
            v = v.repeat_interleave(rep, dim=1)
        o = F.scaled_dot_product_attention(q, k, v, is_causal=True)
        o = o.transpose(1, 2).reshape(batch * seq, hq * hd)
        return self._leave(x, self.wo(o))


class LlamaModel(torch.nn.Module):
    """Token ids [batch, seq] -> mean next-token cross-entropy (fp32).  With ``cp``, ``ids`` (and
    ``targets``) are this rank's shard of consecutive positions and the loss is the shard's mean.
    With ``cu_seqlens`` the ``batch * seq`` tokens are packed documents (module docstring): pass
    ``targets`` with -100 at each document's last token.  ``cfg.loss`` picks the loss (module
    docstring): "fused" is a collective over ``tp`` and the only choice when ``tp`` has more than
    one rank."""

    def __init__(self, cfg: LlamaConfig, tp, device, dtype=torch.bfloat16, seed: int = 0, vocab: bool = True,
                 cp=None):
        super().__init__()
        self.cfg = cfg
        self.vocab = vocab
        self.tp = tp
        _check_rope_config(cfg)
        _check_norm_config(cfg)
        if cfg.loss not in LOSS_KINDS:
            raise ValueError(f"LlamaConfig.loss must be one of {LOSS_KINDS}, got {cfg.loss!r}")
        if vocab and cfg.loss == "torch" and _size_rank(tp)[0] > 1:
            raise ValueError(f'a TP group of {_size_rank(tp)[0]} ranks shards the vocabulary: it needs loss="fused" '
                             '(loss="torch" would index past the shard)')
        if vocab:
            self.embed = torch.nn.Embedding(cfg.vocab, cfg.d, device=device, dtype=dtype)
            with torch.no_grad():
                g = torch.Generator(device=device).manual_seed(seed)
                self.embed.weight.normal_(0.0, 0.02, generator=g)
        # one cos / sin table for every block (fp32 [max_positions, 2, head_dim / 2]); None without rope
        self.rope_table = rope_table(cfg.max_positions, cfg.head_dim, cfg.rope_theta, device=device) if cfg.rope else None
        self.blocks = torch.nn.ModuleList(LlamaBlock(cfg, tp, seed + 10 * (i + 1), device, dtype, cp=cp,
                                                     rope_table=self.rope_table)
                                          for i in range(cfg.layers))
        self.norm = RMSNorm(cfg.d, cfg.eps, device, dtype)
        if vocab:
            self.head = ColumnParallelLinear(cfg.d, cfg.vocab, tp, bias=False, device=device, dtype=dtype,
                                             seed=seed + 7, init="device")

    def forward(self, ids, x0: Optional[torch.Tensor] = None, targets: Optional[torch.Tensor] = None,
                cu_seqlens: Optional[torch.Tensor] = None):
        b, s = ids.shape
        for blk in self.blocks[:1]:  # a sequence beyond max_positions is refused before the embedding runs
            blk.check_positions(s, cu_seqlens)
        x = self.embed(ids).view(b * s, self.cfg.d) if self.vocab else x0
        if self.cfg.norm == "fused":  # every residual add happens in the norm that follows it
            addend = None
            for blk in self.blocks:
                x, addend = blk(x, b, s, cu_seqlens, addend)
            x = (rms_norm(x, self.norm.weight, self.norm.eps) if addend is None
                 else add_rms_norm(x, addend, self.norm.weight, self.norm.eps)[1])
        else:
            for blk in self.blocks:
                x = blk(x, b, s, cu_seqlens)
            x = self.norm(x)
        if not self.vocab:
            return x.float().pow(2).mean()
        logits = self.head(x)
        # explicit targets [batch, seq] replace the roll (context parallel: a shard's last target is
        # the next rank's first id)
        tgt = (torch.roll(ids, -1, dims=1) if targets is None else targets).reshape(-1)
        if self.cfg.loss == "fused":
            return vocab_parallel_cross_entropy(self.tp, logits, tgt.contiguous())
        return F.cross_entropy(logits.float(), tgt)


def _self_comm(comm):
    """A one-rank communicator (this rank alone): the TP group of a pure-DP run."""
    r = comm.Get_rank()
    return comm.Split(r, r)  # reference order (key, color)


def measure_ddp_overlap(comm, layers: int = 32, tokens: int = 4096, seq: int = 2048, vocab: bool = True,
                        iters: int = 2, cfg: LlamaConfig = LLAMA3_8B, bucket_mb: Optional[int] = None,
                        blocks_sweep: List[int] = (32, 64, 128, 256), verbose: bool = False) -> Dict:
    """Compute-only, comm-only, overlapped and deferred step times (forward + backward +
    finish, max over ranks) of the Llama-3-8B-shaped model under DDP over ``comm``, and the
    signed hidden fraction ``(compute + comm - overlapped) / comm``; the bucket all-reduces'
    CTA budget swept over ``blocks_sweep`` (the best overlapped one is the record), then the
    deferred schedule (all buckets after the backward at the full budget).  ``step_ms`` is
    the faster schedule (``schedule``), both on record.  Collective: every rank calls."""
    from .. import mpi as MPI

    hc = comm.comm
    p, rank = comm.Get_size(), comm.Get_rank()
    dev = comm.dev
    device = dev.device
    seq = min(seq, tokens)
    batch = max(1, tokens // seq)
    c = LlamaConfig(**{**cfg.__dict__, "layers": layers})

    def say(msg: str) -> None:
        if verbose and rank == 0:
            import sys

            print(f"[llama_dp] {msg}", file=sys.stderr, flush=True)

    t0 = time.perf_counter()
    tp = _self_comm(comm)
    model = LlamaModel(c, tp, device, vocab=vocab)
    nparams = sum(q.numel() for q in model.parameters())
    say(f"model: {nparams / 1e9:.2f} B params, {time.perf_counter() - t0:.1f}s")
    # the schedules are timed explicitly below (overlapped per budget, then deferred)
    ddp = DistributedDataParallel(model, comm, bucket_bytes=(bucket_mb << 20) if bucket_mb else None,
                                  broadcast_params=False, schedule="overlap")
    say(f"DDP: {len(ddp.buckets)} buckets, {time.perf_counter() - t0:.1f}s")
    g = torch.Generator(device=device).manual_seed(1234 + rank)  # each DP rank its own data shard
    ids = torch.randint(0, c.vocab, (batch, seq), generator=g, device=device)
    x0 = None if vocab else (torch.randn(batch * seq, c.d, generator=g, device=device) * 0.5).bfloat16().requires_grad_()

    def step():
        ddp.zero_grad()
        loss = ddp(ids, x0)
        loss.backward()
        ddp.finish()
        return loss

    def timed(fn) -> float:
        fn()
        torch.cuda.synchronize()
        dev.check()
        hc.Barrier()
        s0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        return hc.allreduce((time.perf_counter() - s0) / iters, op=MPI.MAX)

    ddp.require_backward_grad_sync = False
    t_compute = timed(step)
    say(f"compute-only {t_compute * 1e3:.1f} ms")
    ddp.require_backward_grad_sync = True

    def hidden_of(t_c: float, t_o: float):
        # signed: negative when the overlapped step is slower than compute + comm back to back
        return None if p == 1 or t_c == 0 else (t_compute + t_c - t_o) / t_c

    # comm-only at the group's full CTA budget (max_blocks): the bound the links set, with no
    # compute beside it
    t_full = 0.0
    if p > 1:
        def allreduce_full():
            for b in ddp.buckets:
                dev.allreduce(b.buf, b.buf, "SUM", ddp.algo, max_blocks=dev.max_blocks, symmetric=True)

        t_full = timed(allreduce_full)
        say(f"comm-only at the full budget ({dev.max_blocks} CTAs) {t_full * 1e3:.1f} ms")
    # every budget: comm-only and overlapped at the SAME bucket CTA budget, so each hidden
    # fraction compares like with like; budgets above the group's overlap cap would only be
    # clamped to it (on a shared GPU: half the CUs, the deadlock bound -- DeviceComm.overlap_cap)
    cap = getattr(dev, "overlap_cap", None)
    budgets = sorted({min(mb, cap) if cap else mb for mb in blocks_sweep}) if p > 1 else [0]
    sweep, per = {}, {}
    for mb in budgets:
        ddp.max_blocks = mb or None
        t_c = timed(ddp.allreduce_all) if p > 1 else 0.0
        sweep[mb] = timed(step)
        per[mb] = {"comm_ms": round(t_c * 1e3, 2), "overlapped_ms": round(sweep[mb] * 1e3, 2),
                   "hidden": None if hidden_of(t_c, sweep[mb]) is None else round(hidden_of(t_c, sweep[mb]), 3)}
        say(f"{mb} CTAs per bucket all-reduce: comm-only {t_c * 1e3:.1f} ms, overlapped {sweep[mb] * 1e3:.1f} ms")
    best_mb = min(sweep, key=sweep.get)
    ddp.max_blocks = best_mb or None
    t_over = sweep[best_mb]
    t_comm = per[best_mb]["comm_ms"] / 1e3
    # deferred: every bucket all-reduced after the backward at the full budget (nothing
    # beside the GEMMs); the step is the faster of the two schedules -- DDP's own
    # schedule="auto" makes the same choice in a training loop
    t_def = None
    if p > 1:
        ddp.schedule = "deferred"
        t_def = timed(step)
        say(f"deferred (post-backward, {dev.max_blocks} CTAs) {t_def * 1e3:.1f} ms")
    chosen = "deferred" if (t_def is not None and t_def < t_over) else "overlap"
    ddp.schedule = chosen
    t_both = t_def if chosen == "deferred" else t_over
    loss = float(step().item())
    torch.cuda.synchronize()
    dev.check()
    hidden = hidden_of(t_comm, t_over)
    gbytes = sum(b.buf.numel() * b.buf.element_size() for b in ddp.buckets)
    nonemb = nparams - (c.vocab * c.d if vocab else 0)
    flops = 6 * nonemb * batch * seq  # fwd + bwd GEMM work (attention scores not counted)
    from .tensor_parallel import CALLS

    out = {"model": f"Llama-3-8B-shaped, {layers} layers" + ("" if vocab else ", no embedding/LM head"),
           "ranks": p, "params": nparams, "grad_bytes_bf16": gbytes, "tokens_per_rank": batch * seq,
           "seq_len": seq, "backward": "autograd (real dX + dW GEMMs, attention, norms, embedding)",
           "compute_ms": round(t_compute * 1e3, 2), "comm_ms": round(t_comm * 1e3, 2),
           "step_ms": round(t_both * 1e3, 2), "schedule": chosen,
           "overlapped_ms": round(t_over * 1e3, 2), "deferred_ms": None if t_def is None else round(t_def * 1e3, 2),
           # signed: (compute + comm - overlapped) / comm of the overlapped schedule
           "comm_hidden_fraction": None if hidden is None else round(hidden, 3),
           "comm_algbw_GBps": round(gbytes / t_comm / 1e9, 2) if t_comm else None,
           "comm_full_ms": round(t_full * 1e3, 2), "comm_full_blocks": dev.max_blocks if p > 1 else None,
           "comm_full_algbw_GBps": round(gbytes / t_full / 1e9, 2) if t_full else None,
           "per_budget": {str(k): v for k, v in per.items()},
           "step_TFLOPs_per_rank": round(flops / t_both / 1e12, 1),
           "bucket_MiB": round(max(ddp.bucket_sizes) / (1 << 20), 1), "buckets": len(ddp.buckets),
           "bucket_ctas": best_mb, "bucket_ctas_sweep_ms": {str(k): round(v * 1e3, 2) for k, v in sweep.items()},
           "grad_sink_gemms": CALLS.get("wgrad_sink", 0), "shared_gpu": dev.shared_device,
           "loss": round(loss, 4), "setup_s": round(time.perf_counter() - t0, 1)}
    del ddp, model
    torch.cuda.empty_cache()
    return out
