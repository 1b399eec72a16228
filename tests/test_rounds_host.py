"""The streaming kernels of DeltaHost at forced round counts, on the CPU work-group emulator: the same kernel and host
source the HIP library is built from, each operator against its own oracle (tests/rounds_checks.py)."""
import pytest

from tests import rounds_checks as rc
from tests.harness import emul  # noqa: F401


@pytest.mark.parametrize("name,c", rc.CASE_COUNTS, ids=lambda v: str(v))
def test_case(emul, name, c):
    rc.check_case(emul, name, c)


def test_table_is_complete():
    rc.check_table_is_complete()


def test_hook(emul):
    rc.check_hook(emul)


def test_unaligned_views(emul):
    rc.check_views(emul)


def test_after_an_error(emul):
    rc.check_after_an_error(emul)


def test_empty(emul):
    rc.check_empty(emul)
