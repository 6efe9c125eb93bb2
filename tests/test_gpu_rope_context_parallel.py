"""Rotary position embedding under context parallelism on 2 and 3 ranks sharing the GPU
(tests/workers/rope_cp_worker.py): each rank's ``rope_apply(pos0 = r S_loc)`` bitwise against its rows
of the full call, and the tiny ``rope=True`` flash model with ``cp`` against the single-process
``rope=True`` model on the full sequence."""
import pytest

from _launch import py, run_ranks
from collective_communication_mpi_amd.ops import rope_apply  # noqa: F401

pytestmark = pytest.mark.gpu

ENV = {"CCMPI_DEVICE_TIMEOUT_S": "20"}


@pytest.mark.parametrize("n", [2, 3])
def test_rope_context_parallel(n):
    r = run_ranks(n, py("tests/workers/rope_cp_worker.py"), timeout=180, env=ENV)
    assert "rope context parallel OK" in r.stdout
    assert "worst error / tolerance" in r.stdout
    assert "worst gradient cosine" in r.stdout
    print(r.stdout)
