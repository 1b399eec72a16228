"""MXFP4 on the CPU work-group emulator: the kernels of csrc/sm_mx4.hpp and their host path, the same source the HIP
library is built from, against the exact restatement and the format's error bound (tests/mx4_checks.py)."""
import pytest

from tests import mx4_checks as mc
from tests.harness import DTYPES, emul  # noqa: F401


def test_conversions_exhaustively(emul):
    mc.check_conversions(emul)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("rows", mc.ROWS)
def test_shapes(emul, rows, dtype):
    mc.check_shapes(emul, rows, dtype)


def test_views(emul):
    mc.check_views(emul)


@pytest.mark.parametrize("corner", mc.CORNERS, ids=lambda f: f.__name__[len("corner_"):])
def test_corner(emul, corner):
    corner(emul, "cpu")


def test_error_bound_in_fp64(emul):
    mc.check_error_bound(emul)


def test_commands_and_merge(tmp_path, emul):
    mc.check_commands_and_merge(tmp_path, emul, "cpu")


def test_odd_columns_are_copied(tmp_path, emul):
    mc.check_odd_columns(tmp_path, emul, "cpu")
