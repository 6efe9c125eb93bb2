"""The rules of the fused AdamW that need no GPU.

* ``ops.optim_validate`` refusals, the slot map ``ops.optim_tile_map``, ``ops.optim_sched``.
* ``ops.adamw_reference``: the fp64 mirror against ``torch.optim.AdamW`` on fp64 parameters, and
  the fp32 mirror (the kernel's bits) against the fp64 mirror.
* ``ops.grad_norm_reference``.
"""
import math

import pytest
import torch

from collective_communication_mpi_amd import ops

BF16, F32, F64, I64, I32 = torch.bfloat16, torch.float32, torch.float64, torch.int64, torch.int32
CHUNK = ops.OPTIM_CHUNK


def f32(x):
    """A Python float rounded once to fp32."""
    return torch.tensor(float(x), dtype=F64).to(F32).item()


# ---------------------------------------------------------------------------
# argument rules
# ---------------------------------------------------------------------------
def _ok(n=20, offs=(0, 7, 20), dtype=BF16):
    S = len(offs) - 1
    return dict(g=torch.zeros(n, dtype=dtype), seg_off=torch.tensor(offs, dtype=I64), seg_ptr=torch.zeros(S, dtype=I64),
                seg_flags=torch.zeros(S, dtype=I32), p32=None if dtype == F32 else torch.zeros(n), m=torch.zeros(n),
                v=torch.zeros(n), partials=torch.zeros(n // CHUNK + S), sums=torch.zeros(2, 3, dtype=F64), bucket=1,
                clip=torch.zeros(2), sched=torch.zeros(4))


def test_constants():
    assert CHUNK == 2048 and ops.OPTIM_DECAY == 1 and ops.OPTIM_SHARDED == 2
    assert ops.optim_slots(4104, 3) == 5


def test_validate_accepts():
    assert ops.optim_validate(**_ok()) == (20, 2)
    assert ops.optim_validate(**_ok(dtype=F32)) == (20, 2)
    assert ops.optim_validate(**_ok(1, (0, 1))) == (1, 1)
    a = _ok()
    a["sums"] = torch.zeros(3, 4, dtype=F64)[0::2]  # rows apart: a row stride of its own
    assert ops.optim_validate(**a) == (20, 2)
    assert ops.optim_validate(a["g"], a["seg_off"]) == (20, 2)


@pytest.mark.parametrize("name,exc,change", [
    ("fp16 bucket", TypeError, lambda a: a.update(g=a["g"].half())),
    ("int32 seg_off", TypeError, lambda a: a.update(seg_off=a["seg_off"].int())),
    ("int32 seg_ptr", TypeError, lambda a: a.update(seg_ptr=a["seg_ptr"].int())),
    ("int64 seg_flags", TypeError, lambda a: a.update(seg_flags=a["seg_flags"].long())),
    ("bf16 m", TypeError, lambda a: a.update(m=a["m"].bfloat16())),
    ("fp64 p32", TypeError, lambda a: a.update(p32=a["p32"].double())),
    ("fp32 sums", TypeError, lambda a: a.update(sums=a["sums"].float())),
    ("fp64 clip", TypeError, lambda a: a.update(clip=a["clip"].double())),
    ("fp64 sched", TypeError, lambda a: a.update(sched=a["sched"].double())),
    ("fp64 partials", TypeError, lambda a: a.update(partials=a["partials"].double())),
    ("a list for the bucket", TypeError, lambda a: a.update(g=[0.0] * 20)),
    ("2-D bucket", ValueError, lambda a: a.update(g=torch.zeros(4, 5, dtype=BF16))),
    ("strided bucket", ValueError, lambda a: a.update(g=torch.zeros(40, dtype=BF16)[::2])),
    ("misaligned bucket", ValueError, lambda a: a.update(g=torch.zeros(28, dtype=BF16)[4:24])),
    ("seg_off not from 0", ValueError, lambda a: a.update(seg_off=torch.tensor([1, 7, 20]))),
    ("seg_off not to n", ValueError, lambda a: a.update(seg_off=torch.tensor([0, 7, 19]))),
    ("an empty segment", ValueError, lambda a: a.update(seg_off=torch.tensor([0, 7, 7, 20]), seg_ptr=None, seg_flags=None)),
    ("a decreasing seg_off", ValueError, lambda a: a.update(seg_off=torch.tensor([0, 21, 20]))),
    ("seg_off of one entry", ValueError, lambda a: a.update(seg_off=torch.tensor([0]))),
    ("seg_ptr of another length", ValueError, lambda a: a.update(seg_ptr=torch.zeros(3, dtype=I64))),
    ("seg_flags of another length", ValueError, lambda a: a.update(seg_flags=torch.zeros(1, dtype=I32))),
    ("short m", ValueError, lambda a: a.update(m=torch.zeros(19))),
    ("long v", ValueError, lambda a: a.update(v=torch.zeros(21))),
    ("misaligned v", ValueError, lambda a: a.update(v=torch.zeros(24)[1:21])),
    ("short partials", ValueError, lambda a: a.update(partials=torch.zeros(1))),
    ("sums of 3 rows", ValueError, lambda a: a.update(sums=torch.zeros(3, 3, dtype=F64))),
    ("sums with a column stride", ValueError, lambda a: a.update(sums=torch.zeros(2, 6, dtype=F64)[:, ::2])),
    ("bucket past the sums", ValueError, lambda a: a.update(bucket=3)),
    ("negative bucket", ValueError, lambda a: a.update(bucket=-1)),
    ("clip of 3", ValueError, lambda a: a.update(clip=torch.zeros(3))),
    ("sched of 3", ValueError, lambda a: a.update(sched=torch.zeros(3))),
    ("beta of 1", ValueError, lambda a: a.update(betas=(0.9, 1.0))),
    ("negative beta", ValueError, lambda a: a.update(betas=(-0.1, 0.9))),
    ("negative eps", ValueError, lambda a: a.update(eps=-1e-8)),
    ("infinite eps", ValueError, lambda a: a.update(eps=float("inf"))),
    ("max_grid too large", ValueError, lambda a: a.update(max_grid=4097)),
    ("max_grid a float", ValueError, lambda a: a.update(max_grid=2.0)),
])
def test_validate_refuses(name, exc, change):
    a = _ok()
    change(a)
    with pytest.raises(exc, match="optim"):
        ops.optim_validate(**a)


def test_validate_refuses_p32_for_an_fp32_bucket():
    a = _ok(dtype=F32)
    a["p32"] = torch.zeros(20)
    with pytest.raises(ValueError, match="its own master"):
        ops.optim_validate(**a)


def test_raw_ops_refuse_before_they_reach_the_extension():
    a = _ok()
    with pytest.raises(ValueError, match="optim"):
        ops.optim_sqsum(a["g"], a["seg_off"], a["seg_flags"], None, a["sums"])
    with pytest.raises(ValueError, match="p32"):
        ops.optim_adamw_update(a["g"], a["seg_off"], a["seg_ptr"], a["seg_flags"], None, a["m"], a["v"], a["sched"])
    for bad in (0.0, -1.0, float("inf"), float("nan"), 1e-60, True):
        with pytest.raises(ValueError, match="max_norm"):
            ops.optim_clip(a["sums"], bad, a["clip"])
    with pytest.raises(TypeError, match="optim"):
        ops.optim_clip(a["sums"].float(), 1.0, a["clip"])


# ---------------------------------------------------------------------------
# the slot map
# ---------------------------------------------------------------------------
LAYOUTS = {
    "mixed": [1, 7, 8, 2048, 2049, 4104],
    "single": [4104],
    "spare": [2049, 1, 7, 2048],
}


def _offsets(sizes):
    off = [0]
    for s in sizes:
        off.append(off[-1] + s)
    return off


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("chunk", (CHUNK, 8, 1))
def test_tile_map_covers_every_element_once(layout, chunk):
    off = _offsets(LAYOUTS[layout])
    n, S = off[-1], len(off) - 1
    slots = ops.optim_tile_map(torch.tensor(off), chunk)
    assert len(slots) == n // chunk + S
    seen = torch.zeros(n, dtype=torch.int32)
    last = (-1, -1)
    for e in slots:
        if e is None:
            continue
        seg, b, end = e
        assert off[seg] <= b < end <= off[seg + 1] and end - b <= chunk
        assert (b - off[seg]) % chunk == 0, "slots start at the segment's first element"
        assert (seg, b) > last, "slots are in bucket order"
        last = (seg, b)
        seen[b:end] += 1
    assert (seen == 1).all()


def test_tile_map_spare_slots_and_one_segment():
    off = _offsets(LAYOUTS["spare"])  # 4105 elements: 2 + 4 slots
    slots = ops.optim_tile_map(off)
    assert slots == [(0, 0, 2048), (0, 2048, 2049), (1, 2049, 2050), (2, 2050, 2057), (3, 2057, 4105), None]
    assert ops.optim_tile_map([0, 4104]) == [(0, 0, 2048), (0, 2048, 4096), (0, 4096, 4104)]
    assert ops.optim_tile_map([0, 1]) == [(0, 0, 1)]
    assert ops.optim_tile_map([0, 2048]) == [(0, 0, 2048), None]
    for bad in ([0], [1, 5], [0, 5, 5], [0, 5, 4]):
        with pytest.raises(ValueError, match="optim_tile_map"):
            ops.optim_tile_map(bad)
    with pytest.raises(ValueError, match="slot"):
        ops.optim_tile_map([0, 4104], slots=[3])


def test_tile_map_of_a_table_of_2_to_the_33_elements():
    emb = 128256 * 4096 + 3  # an embedding-sized segment, then offsets past 2^32 that are no multiple of 8
    off = [0, emb, (1 << 32) + 5, (1 << 33) - 2048, 1 << 33]
    n, S = off[-1], 4
    total = n // CHUNK + S
    first = [off[i] // CHUNK + i for i in range(S)]
    probe = sorted({s + d for s in first for d in (-2, -1, 0, 1, 2) if 0 <= s + d < total} | {0, total - 1})
    got = dict(zip(probe, ops.optim_tile_map(off, CHUNK, slots=probe)))
    for i in range(S):
        assert got[first[i]] == (i, off[i], min(off[i] + CHUNK, off[i + 1]))
        if i:
            # the slot in front of a segment's first holds the end of the segment before it, or is spare
            prev = got[first[i] - 1]
            tiles = -(-(off[i] - off[i - 1]) // CHUNK)
            if first[i - 1] + tiles == first[i]:
                assert prev is not None and prev[0] == i - 1 and prev[2] == off[i]
            else:
                assert prev is None
    assert got[first[1] + 1] == (1, emb + CHUNK, emb + 2 * CHUNK)
    assert got[total - 1] is None  # the last segment is one whole chunk: its second slot is spare
    assert got[total - 2] == (3, (1 << 33) - 2048, 1 << 33)
    # every element of the three boundaries is covered exactly once by the slots around it
    for i in (1, 2, 3):
        cover = [e for e in (got[first[i] - 2], got[first[i] - 1], got[first[i]]) if e is not None]
        assert sum(1 for (_, b, e) in cover if b <= off[i] - 1 < e) == 1
        assert sum(1 for (_, b, e) in cover if b <= off[i] < e) == 1


# ---------------------------------------------------------------------------
# the schedule
# ---------------------------------------------------------------------------
def test_sched_is_fp64_rounded_once():
    s = ops.optim_sched(3e-4, (0.9, 0.95), 0.1, 7)
    assert s.dtype == F32 and tuple(s.shape) == (4,) and s.device.type == "cpu"
    want = [3e-4, 1.0 - 0.9 ** 7, 1.0 - 0.95 ** 7, 1.0 - 3e-4 * 0.1]
    assert s.tolist() == [f32(x) for x in want]
    assert ops.optim_sched(1e-3, (0.9, 0.999), 0.0, 1).tolist() == [f32(1e-3), f32(1.0 - 0.9), f32(1.0 - 0.999), 1.0]
    assert ops.optim_sched(1e-3, (0.9, 0.999), 0.0, 10 ** 6).tolist()[1:3] == [1.0, 1.0]
    for bad in (dict(t=0), dict(lr=-1.0), dict(weight_decay=float("inf")), dict(betas=(0.9, 1.0))):
        kw = dict(lr=1e-3, betas=(0.9, 0.999), weight_decay=0.0, t=1)
        kw.update(bad)
        with pytest.raises(ValueError, match="optim"):
            ops.optim_sched(**kw)


# ---------------------------------------------------------------------------
# the mirrors
# ---------------------------------------------------------------------------
N = 4096
B1, B2, EPS = f32(0.9), f32(0.999), f32(1e-8)  # exact in fp32: both mirrors and torch see the same constants
LR, WD = 1e-3, 0.1


def _grads(gen, dtype=F64):
    """Magnitudes from 1e-6 to 1, random signs."""
    mag = torch.pow(10.0, -6.0 * torch.rand(N, generator=gen, dtype=F64))
    sign = torch.where(torch.rand(N, generator=gen) < 0.5, -1.0, 1.0).double()
    return (mag * sign).to(dtype)


def _sched64(t):
    return torch.tensor([LR, 1.0 - B1 ** t, 1.0 - B2 ** t, 1.0 - LR * WD], dtype=F64)


def test_fp64_mirror_against_torch_adamw():
    gen = torch.Generator().manual_seed(11)
    p0 = torch.randn(N, generator=gen, dtype=F64)
    q = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([q], lr=LR, betas=(B1, B2), eps=EPS, weight_decay=WD)
    p, m, v = p0.clone(), torch.zeros(N, dtype=F64), torch.zeros(N, dtype=F64)
    worst = 0.0
    for t in range(1, 11):
        g = _grads(gen)
        coef = f32(0.05 + 0.95 * torch.rand((), generator=gen).item())
        q.grad = g * coef
        opt.step()
        p, m, v = ops.adamw_reference(g, p, m, v, _sched64(t), coef, (B1, B2), EPS, True, dtype=F64)
        ratio = ((p - q.detach()).abs() / (1e-12 * (q.detach().abs() + LR))).max().item()
        worst = max(worst, ratio)
    print(f"[optim rules] fp64 mirror against torch.optim.AdamW: {worst:.4f} of the bound")
    assert worst <= 1.0
    # without decay: the parameter is not scaled
    p2, _, _ = ops.adamw_reference(g, p0, m, v, _sched64(10), None, (B1, B2), EPS, False, dtype=F64)
    p3, _, _ = ops.adamw_reference(g, p0, m, v, _sched64(10), None, (B1, B2), EPS, True, dtype=F64)
    mask = torch.arange(N) % 2 == 0
    p4, _, _ = ops.adamw_reference(g, p0, m, v, _sched64(10), None, (B1, B2), EPS, mask, dtype=F64)
    assert not torch.equal(p2, p3) and torch.equal(p4, torch.where(mask, p3, p2))


def _normal_or_zero(x):
    return bool(((x == 0) | (x.abs() >= 2.0 ** -100)).all())


def test_fp32_mirror_against_the_fp64_mirror():
    worst = 0.0
    for seed in range(5):
        gen = torch.Generator().manual_seed(100 + seed)
        p = torch.randn(N, generator=gen)
        m, v = torch.zeros(N), torch.zeros(N)
        for t in range(1, 11):
            g = _grads(gen, BF16 if seed % 2 else F32)
            coef = torch.tensor(0.05 + 0.95 * torch.rand((), generator=gen).item(), dtype=F32)
            sched = ops.optim_sched(LR, (B1, B2), WD, t)
            e_p, e_m, e_v = ops.adamw_reference(g, p, m, v, sched, coef, (B1, B2), EPS, True, dtype=F64)
            n_p, n_m, n_v = ops.adamw_reference(g, p, m, v, sched, coef, (B1, B2), EPS, True, dtype=F32)
            assert n_p.dtype == F32 and e_p.dtype == F64
            assert _normal_or_zero(n_m) and _normal_or_zero(n_v), "an intermediate that flushing could change"
            decay = sched[3].double()
            bound = 2.0 ** -22 * e_p.abs() + 2.0 ** -19 * (e_p - p.double() * decay).abs()
            worst = max(worst, ((n_p.double() - e_p).abs() / bound).max().item())
            p, m, v = n_p, n_m, n_v
    print(f"[optim rules] fp32 mirror against the fp64 mirror: {worst:.4f} of the bound")
    assert worst <= 1.0


def test_grad_norm_reference():
    a, b = torch.tensor([3.0, 0.0], dtype=BF16), torch.tensor([[4.0]], dtype=F32)
    assert ops.grad_norm_reference([a, b]) == (5.0, 0.0, 25.0)
    assert ops.grad_norm_reference([a, b], [True, False]) == (5.0, 9.0, 16.0)
    big = torch.full((1 << 20,), 1e-3, dtype=F32)
    norm, _, _ = ops.grad_norm_reference([big])
    assert math.isclose(norm, float(big[0].double()) * 1024.0, rel_tol=1e-12)
