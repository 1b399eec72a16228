"""GPTQ-layout INT4 on the CPU work-group emulator: the kernels of csrc/sm_gptq.hpp and their host path, the same source
the HIP library is built from, against the plain restatement and the format's error bound (tests/gptq_checks.py)."""
import pytest

from tests import gptq_checks as gc
from tests.harness import DTYPES, emul  # noqa: F401


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("g", gc.GROUPS)
def test_shapes(emul, g, dtype):
    gc.check_shapes(emul, g, dtype)


def test_views(emul):
    gc.check_views(emul)


def test_forced_rounds(emul):
    gc.check_rounds(emul)


@pytest.mark.parametrize("corner", gc.CORNERS, ids=lambda f: f.__name__[len("corner_"):])
def test_corner(emul, corner):
    corner(emul, "cpu")


def test_commands_and_merge(tmp_path, emul):
    gc.check_commands_and_merge(tmp_path, emul, "cpu")
