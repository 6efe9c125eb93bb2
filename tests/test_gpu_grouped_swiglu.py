"""SwiGLU gate in the grouped gate|up GEMM's epilogue (``grouped_gemm_nt_swiglu``) against
the two kernels it replaces, bit for bit, and ``GroupedExpertsMLP`` with the fused forward
and the K-major-B dX against its earlier three-step form and against torch autograd.

Tolerances against torch autograd are composed as tests/workers/moe_train_worker.py composes
them, from rtol 2e-2 / atol 8e-2 per bf16 GEMM a value passed through and rtol 2e-3 / atol
2e-3 sqrt(rows) for a weight gradient:
  forward       gate|up, down                          rtol 4e-2    atol 1.6e-1
  x.grad        gate|up forward, down dX, gate|up dX   rtol 6e-2    atol 2.4e-1
  down.grad     gate|up forward + the weight gradient  rtol 2.2e-2  atol 8e-2 + 2e-3 sqrt(rows)
  gate_up.grad  gate|up forward, down dX + the w. g.   rtol 4.2e-2  atol 1.6e-1 + 2e-3 sqrt(rows)
New against old form: bitwise where the same kernels see the same inputs (the forward, the
weight gradient of ``down``), the bf16 tolerance rtol 2e-2 / atol 8e-2 elsewhere."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = -512.0


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _random_counts():
    c = np.random.default_rng(4242).integers(1, 200, size=8)
    c[2], c[5] = 0, 300
    return [int(v) for v in c]


#        name      counts            spare  K
CASES = {
    "mixed": ([0, 1, 127, 129], 43, 64),
    "random": (_random_counts(), 17, 520),
}


def _cnt(counts, dtype=torch.int64):
    return torch.tensor(counts, dtype=dtype, device="cuda")


def _bounds(counts, cap):
    e = np.minimum(np.cumsum([0] + [max(int(c), 0) for c in counts]), cap)
    return [(int(e[g]), int(e[g + 1])) for g in range(len(counts))]


@pytest.mark.parametrize("with_bias", [False, True], ids=["plain", "bias_alpha"])
@pytest.mark.parametrize("N", [136, 264])
@pytest.mark.parametrize("name", list(CASES))
def test_fused_gate_is_the_two_kernels_bit_for_bit(name, N, with_bias):
    from collective_communication_mpi_amd.ops import grouped_gemm_nt, grouped_gemm_nt_swiglu, swiglu_pairs

    counts, spare, K = CASES[name]
    G, total = len(counts), sum(counts)
    cap = total + spare
    g = torch.Generator(device="cuda").manual_seed(700 + N + K)
    x = torch.randn(cap, K, device="cuda", generator=g).bfloat16()
    w = (torch.randn(G, N, K, device="cuda", generator=g) / K ** 0.5).bfloat16()
    kw = dict(bias=torch.randn(G, N, device="cuda", generator=g), alpha=0.5) if with_bias else {}
    cnt = _cnt(counts)
    h_ref = grouped_gemm_nt(x, w, cnt, out=torch.zeros(cap, N, dtype=torch.bfloat16, device="cuda"), **kw)
    glu_ref = swiglu_pairs(h_ref)
    h = torch.full((cap, N), SENTINEL, dtype=torch.bfloat16, device="cuda")
    glu = torch.full((cap, N // 2), SENTINEL, dtype=torch.bfloat16, device="cuda")
    got = grouped_gemm_nt_swiglu(x, w, cnt, h=h, glu=glu, **kw)
    assert got[0] is h and got[1] is glu
    assert torch.equal(h[:total], h_ref[:total]), "h differs from grouped_gemm_nt"
    assert torch.equal(glu[:total], glu_ref[:total]), "glu differs from swiglu_pairs(h)"
    assert torch.equal(h[total:], torch.full_like(h[total:], SENTINEL)), "rows of h past the total were written"
    assert torch.equal(glu[total:], torch.full_like(glu[total:], SENTINEL)), "rows of glu past the total were written"
    h2, glu2 = grouped_gemm_nt_swiglu(x, w, cnt, **kw)       # allocated by the op
    assert h2.shape == (cap, N) and glu2.shape == (cap, N // 2) and glu2.dtype == torch.bfloat16
    assert torch.equal(h2[:total], h_ref[:total]) and torch.equal(glu2[:total], glu_ref[:total])


def _mlp_run(monkeypatch, swiglu, dx):
    """(y, x.grad, gate_up.grad, down.grad) of one GroupedExpertsMLP step on fixed data."""
    from collective_communication_mpi_amd.parallel import GroupedExpertsMLP

    for name, val in (("CCMPI_GROUPED_SWIGLU", swiglu), ("CCMPI_GROUPED_DX", dx)):
        if val is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, val)
    G, DM, DFF, counts, spare = 4, 72, 136, [0, 1, 127, 129], 43
    total = sum(counts)
    cap = total + spare
    g = torch.Generator(device="cuda").manual_seed(4136)
    mlp = GroupedExpertsMLP(G, DM, DFF, device="cuda", dtype=torch.float32)
    with torch.no_grad():   # fp32 master weights that bf16 holds exactly
        mlp.gate_up.copy_((torch.randn(G, 2 * DFF, DM, device="cuda", generator=g) / DM ** 0.5).bfloat16())
        mlp.down.copy_((torch.randn(G, DM, DFF, device="cuda", generator=g) / DFF ** 0.5).bfloat16())
    x = torch.randn(cap, DM, device="cuda", generator=g).bfloat16().requires_grad_()
    dy = torch.randn(cap, DM, device="cuda", generator=g).bfloat16()
    y = mlp(x, _cnt(counts))
    y.backward(dy)
    res = (y.detach()[:total], x.grad[:total], mlp.gate_up.grad, mlp.down.grad)
    # torch autograd on the per-expert loop, fp32
    xr = x.detach().float().requires_grad_()
    gu = mlp.gate_up.detach().clone().requires_grad_()
    dn = mlp.down.detach().clone().requires_grad_()
    parts = []
    for e, (a, b) in enumerate(_bounds(counts, cap)):
        hh = xr[a:b] @ gu[e].T
        parts.append((torch.nn.functional.silu(hh[:, 0::2]) * hh[:, 1::2]) @ dn[e].T)
    yr = torch.cat(parts)
    yr.backward(dy[:total].float())
    ref = (yr.detach(), xr.grad[:total], gu.grad, dn.grad)
    return res, ref, max(counts)


def test_grouped_experts_mlp_new_against_old_and_autograd(monkeypatch):
    new, ref, rows = _mlp_run(monkeypatch, None, None)
    old, _, _ = _mlp_run(monkeypatch, "unfused", "transpose")
    dw_atol = 2e-3 * rows ** 0.5
    tols = [dict(rtol=4e-2, atol=1.6e-1), dict(rtol=6e-2, atol=2.4e-1),
            dict(rtol=4.2e-2, atol=1.6e-1 + dw_atol), dict(rtol=2.2e-2, atol=8e-2 + dw_atol)]
    names = ["forward", "x.grad", "gate_up.grad", "down.grad"]
    for run, tag in ((new, "new"), (old, "old")):
        for got, want, tol, name in zip(run, ref, tols, names):
            err = (got.float() - want).abs()
            print(f"{tag} {name}: worst error / tolerance {(err / (tol['atol'] + tol['rtol'] * want.abs())).max().item():.3f}")
            torch.testing.assert_close(got.float(), want, **tol, msg=lambda m: f"{tag} {name}: {m}")
    assert torch.equal(new[0], old[0]), "the fused forward differs from the three-step form"
    assert torch.equal(new[3], old[3]), "down's weight gradient differs"
    for i in (1, 2):
        torch.testing.assert_close(new[i].float(), old[i].float(), rtol=2e-2, atol=8e-2, msg=lambda m: f"{names[i]}: {m}")
    assert new[1].dtype == torch.bfloat16 and new[2].dtype == torch.float32
