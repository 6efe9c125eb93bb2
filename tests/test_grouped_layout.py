"""Grouped expert GEMM, the parts that need no GPU: the host mirror of the kernel's tile
walk (``grouped_tile_map``: tiles start at each expert's first row, so none spans two
experts, and their number never exceeds the count-free grid) and the argument rules
(``grouped_validate``) that raise before any launch."""
import numpy as np
import pytest
import torch

from collective_communication_mpi_amd.ops import grouped_tile_map, grouped_validate

# the count vectors of tests/test_gpu_grouped_gemm.py with their cap
FIXED = [
    ([130], 130),
    ([0, 1, 127, 129], 300),
    ([128, 0, 0, 256, 3], 387),
    ([1 if g % 7 else 0 for g in range(256)], 256),
    ([100, 100, 100], 250),       # overflow: the third expert truncated to 50 rows
    ([0, 0, 0], 64),
    ([5, -3, 7], 64),             # a negative count is an empty expert
]


def random_cases(n=300):
    rng = np.random.default_rng(20240607)
    for _ in range(n):
        G = int(rng.integers(1, 257))
        counts = rng.integers(0, 401, size=G)
        if rng.random() < 0.3:
            counts[rng.random(G) < 0.5] = 0
        total = int(counts.sum())
        mode = rng.integers(0, 4)
        if mode == 0:
            cap = max(1, total - int(rng.integers(1, 300)))      # below the total
        elif mode == 1:
            cap = max(1, total)
        elif mode == 2:
            cap = total + int(rng.integers(1, 130))
        else:
            cap = 2 * total + 1000                                 # well above
        yield counts.tolist(), cap


def check_map(counts, cap, bm=128):
    tiles = grouped_tile_map(counts, cap, bm)
    c = [max(int(v), 0) for v in counts]
    covered = min(sum(c), cap)
    starts = np.minimum(np.cumsum([0] + c), cap)                   # expert g owns [starts[g], starts[g + 1])
    at = 0
    for g, r0, rows in tiles:
        assert 1 <= rows <= bm
        assert r0 == at, "tiles are contiguous and in order: every row exactly once"
        assert starts[g] <= r0 and r0 + rows <= starts[g + 1], "a tile spans two experts"
        assert (r0 - starts[g]) % bm == 0, "tiles start at the expert's first row"
        at = r0 + rows
    assert at == covered
    assert len(tiles) <= -(-cap // bm) + len(counts)
    assert len(tiles) == sum(-(-(int(starts[g + 1]) - int(starts[g])) // bm) for g in range(len(c)))


def test_tile_map_fixed_cases():
    for counts, cap in FIXED:
        check_map(counts, cap)
    assert grouped_tile_map([0, 1, 127, 129], 300) == [(1, 0, 1), (2, 1, 127), (3, 128, 128), (3, 256, 1)]
    assert grouped_tile_map([100, 100, 100], 250) == [(0, 0, 100), (1, 100, 100), (2, 200, 50)]
    assert grouped_tile_map([300, 5], 200) == [(0, 0, 128), (0, 128, 72)]
    assert grouped_tile_map(torch.tensor([3, 2]), 10, bm=2) == [(0, 0, 2), (0, 2, 1), (1, 3, 2)]


def test_tile_map_random_cases():
    for counts, cap in random_cases():
        check_map(counts, cap)
    for counts, cap in random_cases(40):
        check_map(counts, cap, bm=32)


def args(cap=16, K=64, N=32, G=4, dtype=torch.bfloat16, cdtype=torch.int64):
    return torch.zeros(cap, K, dtype=dtype), torch.zeros(G, N, K, dtype=dtype), torch.zeros(G, dtype=cdtype)


def test_validate_accepts_the_contract():
    x, w, c = args()
    assert grouped_validate(x, w, c) == (16, 4, 32, 64)
    x, w, c = args(cap=300, K=72, N=136, G=256, cdtype=torch.int32)
    assert grouped_validate(x, w, c, out=torch.zeros(300, 136), bias=torch.zeros(256, 136)) == (300, 256, 136, 72)
    # a row-strided x and the [G, K, N] view of one transposed [K, G * N] copy (the dX operand)
    big = torch.zeros(16, 128, dtype=torch.bfloat16)
    wt = torch.zeros(32, 4 * 64, dtype=torch.bfloat16).view(32, 4, 64).permute(1, 0, 2)
    assert grouped_validate(big[:, :64], torch.zeros(4, 32, 64, dtype=torch.bfloat16), c[:4].long()) == (16, 4, 32, 64)
    assert grouped_validate(torch.zeros(16, 64, dtype=torch.bfloat16), wt, torch.zeros(4, dtype=torch.int64)) == (16, 4, 32, 64)


def test_validate_rejects():
    x, w, c = args()
    with pytest.raises(TypeError, match="bf16"):
        grouped_validate(x.float(), w, c)                             # a non-bf16 operand
    with pytest.raises(TypeError, match="bf16"):
        grouped_validate(x, w.half(), c)
    xk, wk, ck = args(K=60)
    with pytest.raises(ValueError, match="multiples of 8"):
        grouped_validate(xk, wk, ck)                                  # K % 8
    xn, wn, cn = args(N=20)
    with pytest.raises(ValueError, match="multiples of 8"):
        grouped_validate(xn, wn, cn)                                  # N % 8
    with pytest.raises(ValueError, match="experts"):
        grouped_validate(x, torch.zeros(0, 32, 64, dtype=torch.bfloat16), torch.zeros(0, dtype=torch.int64))
    x257, w257, c257 = args(G=257)
    with pytest.raises(ValueError, match="experts"):
        grouped_validate(x257, w257, c257)
    with pytest.raises(TypeError, match="int32 or int64"):
        grouped_validate(x, w, c.float())                             # float counts
    with pytest.raises(ValueError, match="counts"):
        grouped_validate(x, w, torch.zeros(5, dtype=torch.int64))     # wrong length
    with pytest.raises(ValueError, match="counts"):
        grouped_validate(x, w, torch.zeros(8, dtype=torch.int64)[::2])
    wide = torch.zeros(16, 128, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="inner stride"):
        grouped_validate(wide[:, ::2], w, c)                          # a non-unit inner stride
    with pytest.raises(ValueError, match="inner stride"):
        grouped_validate(x, torch.zeros(4, 64, 32, dtype=torch.bfloat16).permute(0, 2, 1), c)
    with pytest.raises(ValueError, match="shape mismatch"):
        grouped_validate(x, torch.zeros(4, 32, 72, dtype=torch.bfloat16), c)
    with pytest.raises(ValueError, match="16"):
        grouped_validate(torch.zeros(16, 68, dtype=torch.bfloat16)[:, :64], w, c)   # 136-B row stride
    with pytest.raises(TypeError, match="bf16 or fp32"):
        grouped_validate(x, w, c, out=torch.zeros(16, 32, dtype=torch.float16))
    with pytest.raises(ValueError, match="output"):
        grouped_validate(x, w, c, out=torch.zeros(15, 32))
    with pytest.raises(ValueError, match="bias"):
        grouped_validate(x, w, c, bias=torch.zeros(32))
