"""``parallel.AdamW`` across ranks (tests/workers/optim_worker.py): the TP-aware norm, the same
clip coefficient on every rank, the update against the fp32 mirror, and an fp32 reference."""
import pytest

from _launch import py, run_ranks

pytestmark = pytest.mark.gpu

ENV = {"CCMPI_DEVICE_TIMEOUT_S": "20"}


@pytest.mark.parametrize("n,tp", [(2, 2), (2, 1), (4, 2)], ids=("tp2", "dp2", "dp2xtp2"))
def test_adamw_across_ranks(n, tp):
    r = run_ranks(n, py("tests/workers/optim_worker.py", "--tp", str(tp)), timeout=300, env=ENV)
    assert f"optim OK world={n} tp={tp}" in r.stdout, r.stdout
    print(r.stdout.strip().splitlines()[-1])
