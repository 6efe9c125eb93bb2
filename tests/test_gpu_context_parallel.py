"""Context-parallel attention on 2 and 3 ranks sharing the GPU
(tests/workers/context_parallel_worker.py): out, lse and dq bitwise against the local chunk call on
the full k, v; dk and dv against the fp64 sum of all ranks' bf16 partials and against the fp64
reference of the full sequence; the autograd form against the raw form; the tiny flash model with
``cp`` against the single-process model on the full sequence."""
import pytest

from _launch import py, run_ranks
from collective_communication_mpi_amd.parallel import context_parallel_attention  # noqa: F401

pytestmark = pytest.mark.gpu

ENV = {"CCMPI_DEVICE_TIMEOUT_S": "20"}


@pytest.mark.parametrize("n", [2, 3])
def test_context_parallel(n):
    r = run_ranks(n, py("tests/workers/context_parallel_worker.py"), timeout=180, env=ENV)
    assert "context parallel OK" in r.stdout
    assert "worst error / tolerance" in r.stdout
    assert "worst gradient cosine" in r.stdout
    print(r.stdout)
