"""Vocab-parallel cross-entropy on 2 and 3 ranks sharing the GPU
(tests/workers/vocab_parallel_xent_worker.py): loss, lse and n_valid bitwise equal on all ranks and
within the single-GPU tolerance of the fp64 reference on the full vocabulary, every rank's dlogits
against its slice of the reference, the autograd form against the raw form; at 2 ranks the head
end to end and the tiny model with ``loss="fused"`` against the one-rank ``loss="torch"`` model."""
import pytest

from _launch import py, run_ranks
from collective_communication_mpi_amd.parallel import vocab_parallel_cross_entropy  # noqa: F401

pytestmark = pytest.mark.gpu

ENV = {"CCMPI_DEVICE_TIMEOUT_S": "20"}


@pytest.mark.parametrize("n", [2, 3])
def test_vocab_parallel_cross_entropy(n):
    r = run_ranks(n, py("tests/workers/vocab_parallel_xent_worker.py"), timeout=180, env=ENV)
    assert "vocab parallel xent OK" in r.stdout
    assert "worst error / tolerance" in r.stdout
    if n == 2:
        assert "worst gradient cosine" in r.stdout
    print(r.stdout)
