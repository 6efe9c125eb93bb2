"""The rules of the fused cross-entropy that need no GPU.

* ``ops.cross_entropy_validate`` refusals, ``ops.xent_row_splits``, the fp64 mirror
  ``ops.cross_entropy_reference`` against ``F.cross_entropy`` and the partial-merge rule.
* ``LlamaConfig.loss`` and the TP head counts of ``LlamaBlock``, on a stub communicator.
* The checkers of tests/test_gpu_cross_entropy.py against a torch emulation of the three ops
  (fp32 math, one rounding to bf16): every shape must pass.  Then against mutants of that
  emulation, each a way a kernel can be subtly wrong: every one must be reported.
"""
import pytest
import torch
import torch.nn.functional as F

import test_gpu_cross_entropy as gx
from test_gpu_cross_entropy import BF16, F32, I64, IGNORE, SHAPES, W

from collective_communication_mpi_amd import ops
from collective_communication_mpi_amd.parallel import vocab_parallel_cross_entropy  # noqa: F401
from collective_communication_mpi_amd.parallel.llama_dp import LlamaBlock, LlamaConfig, LlamaModel

CPU = "cpu"
NINF = float("-inf")


# ---------------------------------------------------------------------------
# argument rules
# ---------------------------------------------------------------------------
def _ok(T=5, V=64):
    return torch.zeros(T, V, dtype=BF16), torch.zeros(T, dtype=I64)


def test_validate_accepts_the_head_output_and_views():
    z, tg = _ok()
    assert ops.cross_entropy_validate(z, tg) == (5, 64)
    big = torch.zeros(9, 128, dtype=BF16)
    assert ops.cross_entropy_validate(big[2:7, 64:], tg, 64) == (5, 64)  # a column and row view
    assert ops.cross_entropy_validate(big[:1, :8], tg[:1]) == (1, 8)


@pytest.mark.parametrize("name,exc,make", [
    ("fp32 logits", TypeError, lambda z, tg: (z.float(), tg)),
    ("fp16 logits", TypeError, lambda z, tg: (z.half(), tg)),
    ("int32 targets", TypeError, lambda z, tg: (z, tg.int())),
    ("Vloc % 8", ValueError, lambda z, tg: (z[:, :60], tg)),
    ("row stride % 8", ValueError, lambda z, tg: (torch.zeros(5, 68, dtype=BF16)[:, :64], tg)),
    ("misaligned base", ValueError, lambda z, tg: (torch.zeros(5, 72, dtype=BF16)[:, 4:68], tg)),
    ("column stride", ValueError, lambda z, tg: (torch.zeros(5, 128, dtype=BF16)[:, ::2], tg)),
    ("transposed", ValueError, lambda z, tg: (torch.zeros(64, 8, dtype=BF16).t()[:5], tg)),
    ("overlapping rows", ValueError, lambda z, tg: (z[:1].expand(5, 64), tg)),
    ("targets too short", ValueError, lambda z, tg: (z, tg[:4])),
    ("targets 2-D", ValueError, lambda z, tg: (z, tg[:, None])),
    ("targets strided", ValueError, lambda z, tg: (z, torch.zeros(10, dtype=I64)[::2])),
    ("targets on another device", ValueError, lambda z, tg: (z, tg.to("meta"))),
    ("T = 0", ValueError, lambda z, tg: (z[:0], tg[:0])),
    ("1-D logits", ValueError, lambda z, tg: (z[0], tg[:1])),
])
def test_validate_refuses(name, exc, make):
    z, tg = make(*_ok())
    with pytest.raises(exc):
        ops.cross_entropy_validate(z, tg)
    with pytest.raises(exc):  # the launching forms refuse before they reach the extension
        ops.cross_entropy_stats(z, tg)
    with pytest.raises(exc):
        ops.cross_entropy(z, tg)


def test_validate_refuses_a_negative_vocab_start():
    with pytest.raises(ValueError):
        ops.cross_entropy_validate(*_ok(), vocab_start=-1)


def test_row_splits_are_a_pure_function():
    for T in (1, 2, 37, 1023, 1024, 4096):
        for V in (8, W, 7 * W, 7 * W + 8, 16032, 128256):
            s = ops.xent_row_splits(T, V)
            assert s >= 1 and s == ops.xent_row_splits(T, V)
            assert s <= (V + W - 1) // W
            per = ops.kernels._xent_split_sweeps(T, V)
            assert (s - 1) * per * W < V <= s * per * W  # no empty split, every column covered
    assert ops.xent_row_splits(4096, 128256) == 1 and ops.xent_row_splits(1, 128256) > 1
    assert gx._smallest_split_shape() == (1, 7 * W + 8)
    with pytest.raises(ValueError):
        ops.xent_row_splits(0, 8)


# ---------------------------------------------------------------------------
# the fp64 mirror
# ---------------------------------------------------------------------------
def _masked_case(T=9, V=7 * W + 8, seed=3):
    g = torch.Generator().manual_seed(seed)
    z = (torch.randn(T, V, generator=g) * 2).to(BF16)
    tg = torch.randint(0, V, (T,), generator=g)
    z[1, :4 * W] = NINF  # the whole first split of row 1 (T = 9 splits this shard in two)
    tg[1] = V - 3
    z[2, 5::2] = NINF
    tg[2] = 4
    tg[4] = IGNORE
    return z, tg


def test_reference_agrees_with_torch_in_fp64():
    z, tg = _masked_case()
    stats, lse, row_loss, dl = ops.cross_entropy_reference(z, tg, 0, IGNORE, grad=2.5)
    zz = z.double().requires_grad_()
    want = F.cross_entropy(zz, tg, reduction="none", ignore_index=IGNORE)
    (want.sum() / 8 * 2.5).backward()
    assert torch.allclose(row_loss, want.detach(), rtol=0, atol=1e-12) and row_loss[4] == 0
    assert torch.allclose(lse, torch.logsumexp(z.double(), 1), rtol=0, atol=1e-12)
    assert torch.allclose(dl, zz.grad, rtol=0, atol=1e-15) and not bool((dl[4] != 0).any())
    # a shard: global targets, vocab_start, the whole vocabulary's lse
    lo = 4 * W
    _, _, _, dshard = ops.cross_entropy_reference(z[:, lo:], tg, lo, IGNORE, grad=2.5, lse=lse, n_valid=8)
    assert torch.allclose(dshard, zz.grad[:, lo:], rtol=0, atol=1e-15)
    none = torch.full_like(tg, IGNORE)
    _, _, rl0, dl0 = ops.cross_entropy_reference(z, none, 0, IGNORE)
    assert not bool((rl0 != 0).any()) and not bool((dl0 != 0).any())  # no valid row: 0, not NaN


def test_partials_merge_in_index_order():
    z, tg = _masked_case()
    stats, lse, row_loss, _ = ops.cross_entropy_reference(z, tg, 0, IGNORE)
    assert stats.shape[0] == ops.xent_row_splits(*z.shape) == 2
    assert stats[0, 1, 0] == NINF and stats[0, 1, 1] == 0  # an all -inf partial: (-inf, 0)
    l2, r2, s2, n2 = ops.cross_entropy_merge_reference(stats, tg, IGNORE)
    assert not torch.isnan(l2).any()
    assert torch.allclose(l2, lse, rtol=0, atol=1e-12) and torch.allclose(r2, row_loss, rtol=0, atol=1e-12)
    assert int(n2) == 8 and abs(float(s2) - float(row_loss.sum())) < 1e-11
    # TP ranks x splits, rank-major: three shards of the vocabulary, each with its own splits
    V3 = z.shape[1] // 24 * 8
    parts = [ops.cross_entropy_reference(z[:, r * V3:(r + 1) * V3], tg, r * V3, IGNORE)[0] for r in range(3)]
    l3, r3, _, _ = ops.cross_entropy_merge_reference(torch.cat(parts), tg, IGNORE)
    kept = torch.where(tg < 3 * V3, tg, torch.full_like(tg, IGNORE))
    full = ops.cross_entropy_reference(z[:, :3 * V3], kept, 0, IGNORE)
    assert torch.allclose(l3, full[1], rtol=0, atol=1e-12)
    inside = (tg < 3 * V3) & (tg != IGNORE)
    assert torch.allclose(r3[inside], full[2][inside], rtol=0, atol=1e-12)


# ---------------------------------------------------------------------------
# the Llama path's rules
# ---------------------------------------------------------------------------
class StubComm:
    def __init__(self, size, rank=0):
        self.size, self.rank = size, rank

    def Get_size(self):
        return self.size

    def Get_rank(self):
        return self.rank


TINY = dict(d=256, heads=4, kv_heads=2, ffn=256, vocab=512, layers=1)


def test_loss_default_and_unknown_value():
    assert LlamaConfig().loss == "torch"
    with pytest.raises(ValueError, match="loss"):
        LlamaModel(LlamaConfig(**TINY, loss="triton"), StubComm(1), CPU)


def test_torch_loss_refuses_a_sharded_vocabulary():
    with pytest.raises(ValueError, match="fused"):
        LlamaModel(LlamaConfig(**TINY, loss="torch"), StubComm(2), CPU)


def test_block_refuses_head_counts_the_group_does_not_divide():
    with pytest.raises(ValueError, match="heads"):
        LlamaBlock(LlamaConfig(**TINY), StubComm(3), 0, CPU)
    with pytest.raises(ValueError, match="kv_heads"):
        LlamaBlock(LlamaConfig(**TINY), StubComm(4), 0, CPU)
    blk = LlamaBlock(LlamaConfig(**TINY), StubComm(2, 1), 0, CPU)
    assert (blk.heads, blk.kv_heads) == (2, 1) and blk.wq.weight.shape == (128, 256)
    one = LlamaBlock(LlamaConfig(**TINY), StubComm(1), 0, CPU)
    assert (one.heads, one.kv_heads) == (4, 2)


# ---------------------------------------------------------------------------
# the GPU test's checkers on an emulation and on mutants of it
# ---------------------------------------------------------------------------
def _trunc_bf16(t32):
    return (t32.view(torch.int32) & ~0xFFFF).view(F32).to(BF16)


class Emu:
    """The three ops in torch fp32; ``mut`` names the one way in which this instance is wrong."""

    def __init__(self, mut=None):
        self.mut = mut

    def _col(self, tg, vocab_start, V):
        col = tg - (0 if self.mut == "vocab_start" else vocab_start)
        if self.mut == "target+1":
            col = col + 1
        return col, (col >= 0) & (col < V)

    def stats(self, z, tg, vocab_start=0, stats=None):
        T, V = ops.cross_entropy_validate(z, tg, vocab_start)
        splits = ops.xent_row_splits(T, V)
        width = ops.kernels._xent_split_sweeps(T, V) * W
        if stats is None:
            stats = torch.empty((splits, T, 4), dtype=F32)
        zf = z.float()
        col, hit = self._col(tg, vocab_start, V)
        safe = torch.where(hit, col, torch.zeros_like(col))
        end = V - 8 if self.mut == "drop8" and V > 8 else V
        for i in range(splits):
            c0, c1 = i * width, min((i + 1) * width, end)
            m = zf[:, c0:c1].max(dim=1).values
            base = torch.where(m == NINF, torch.zeros_like(m), m)
            here = hit & (col >= c0) & (col < min((i + 1) * width, V))
            stats[i, :, 0] = m
            stats[i, :, 1] = torch.exp(zf[:, c0:c1] - base[:, None]).sum(dim=1)
            stats[i, :, 2] = torch.where(here, zf.gather(1, safe[:, None])[:, 0], torch.zeros_like(m))
            stats[i, :, 3] = here.float()
        return stats

    def combine(self, stats, tg, ignore_index=IGNORE, lse=None, row_loss=None, loss_sum=None, n_valid=None):
        P, T, _ = stats.shape
        M = stats[:, :, 0].max(dim=0).values
        S, zt = torch.zeros(T), torch.zeros(T)
        for i in range(P):
            m = stats[i, :, 0]
            live = m != NINF
            e = torch.exp(torch.where(live, m - M, torch.zeros(T)))
            S = S + torch.where(live, stats[i, :, 1] * e, torch.zeros(T))
            zt = zt + stats[i, :, 2]
        L = M + torch.log(S)
        valid = tg != ignore_index
        loss = L - zt if self.mut == "ignored" else torch.where(valid, L - zt, torch.zeros(T))
        outs = []
        for buf, val, dtype in ((lse, L, F32), (row_loss, loss, F32), (loss_sum, loss.sum().reshape(1), F32),
                                (n_valid, valid.sum().reshape(1), I64)):
            buf = torch.empty(val.shape, dtype=dtype) if buf is None else buf
            buf.copy_(val)
            outs.append(buf)
        return tuple(outs)

    def backward(self, z, tg, lse, n_valid, grad=None, vocab_start=0, ignore_index=IGNORE, dlogits=None):
        T, V = ops.cross_entropy_validate(z, tg, vocab_start)
        g = torch.ones(1) if grad is None else grad
        n = torch.tensor([T]) if self.mut == "scale_T" else n_valid
        scale = torch.where(n > 0, g / n.float(), torch.zeros(1))
        col, hit = self._col(tg, vocab_start, V)
        onehot = torch.zeros(T, V)
        onehot.scatter_(1, torch.where(hit, col, torch.zeros_like(col))[:, None], hit.float()[:, None])
        d = (torch.exp(z.float() - lse[:, None]) - onehot) * scale
        if self.mut != "ignored":
            d = torch.where((tg != ignore_index)[:, None], d, torch.zeros(T, V))
        d = torch.where(n_valid > 0, d, torch.zeros(T, V))
        d16 = _trunc_bf16(d) if self.mut == "trunc" else d.to(BF16)
        if dlogits is None:
            dlogits = torch.empty((T, V), dtype=BF16)
        if self.mut == "drop8" and V > 8:
            dlogits[:, :V - 8].copy_(d16[:, :V - 8])
        else:
            dlogits.copy_(d16)
        return dlogits


@pytest.mark.parametrize("framed", [False, True], ids=["contiguous", "framed"])
@pytest.mark.parametrize("T,V", SHAPES)
def test_checkers_pass_the_emulation(T, V, framed):
    problems, (rf, rb) = gx.check_case(Emu(), T, V, CPU, framed)
    assert not problems, "\n".join(problems)
    assert rf <= 1.0 and rb <= 1.0


def test_checkers_pass_the_emulation_with_every_row_ignored():
    for framed in (False, True):
        problems, _ = gx.check_case(Emu(), 37, W + 8, CPU, framed, all_ignored=True)
        assert not problems, "\n".join(problems)


MUTANTS = {
    "target+1": "the target one column to the right",
    "vocab_start": "vocab_start ignored",
    "ignored": "an ignored row not zeroed",
    "drop8": "the last 8 columns dropped",
    "trunc": "truncation instead of rounding to nearest",
    "scale_T": "the scale uses T instead of n_valid",
}


@pytest.mark.parametrize("framed", [False, True], ids=["contiguous", "framed"])
@pytest.mark.parametrize("mut", sorted(MUTANTS))
def test_checkers_report_every_mutant(mut, framed):
    problems, _ = gx.check_case(Emu(mut), 37, W + 8, CPU, framed)
    assert problems, f"not reported: {MUTANTS[mut]}"
    if mut in ("trunc", "scale_T"):
        assert all(p.startswith("dlogits") for p in problems), problems
