"""NVFP4 on the CPU work-group emulator: the kernels of csrc/sm_nv4.hpp and their host path, the same source the HIP
library is built from, against the plain restatement and the format's error bound (tests/nv4_checks.py)."""
import pytest

from tests import nv4_checks as nc
from tests.harness import DTYPES, emul  # noqa: F401


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("rows", nc.ROWS)
def test_shapes(emul, rows, dtype):
    nc.check_shapes(emul, rows, dtype)


def test_views(emul):
    nc.check_views(emul)


def test_forced_rounds(emul):
    nc.check_rounds(emul)


@pytest.mark.parametrize("corner", nc.CORNERS, ids=lambda f: f.__name__[len("corner_"):])
def test_corner(emul, corner):
    corner(emul, "cpu")


def test_commands_and_merge(tmp_path, emul):
    nc.check_commands_and_merge(tmp_path, emul, "cpu")
