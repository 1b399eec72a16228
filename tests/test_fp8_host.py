"""Block-scaled FP8 on the CPU work-group emulator: the kernels of csrc/sm_fp8.hpp and their host path, the same source
the HIP library is built from, against torch on the CPU bit for bit and against the format's error bound in fp64
(tests/fp8_checks.py)."""
import pytest

from tests import fp8_checks as fc
from tests.harness import DTYPES, emul  # noqa: F401


def test_conversions_exhaustively(emul):
    fc.check_conversions(emul)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("rows", fc.ROWS)
def test_grid(emul, rows, dtype):
    fc.check_grid(emul, rows, dtype)


def test_views(emul):
    fc.check_views(emul)


@pytest.mark.parametrize("corner", fc.CORNERS, ids=lambda f: f.__name__[len("corner_"):])
def test_corner(emul, corner):
    corner(emul, "cpu")


def test_error_bound_in_fp64(emul):
    fc.check_error_bound(emul)


def test_commands_and_merge(tmp_path, emul):
    fc.check_commands_and_merge(tmp_path, emul, "cpu")
