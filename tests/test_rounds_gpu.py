"""The streaming kernels of DeltaHost at forced round counts, on the MI355X: the table of tests/rounds_checks.py at the
same shapes, and MXFP4 and FP8 at two model-like shapes against the emulator library under the same count."""
import pytest

from tests import rounds_checks as rc
from tests.harness import eng  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,c", rc.CASE_COUNTS, ids=lambda v: str(v))
def test_case(eng, name, c):
    rc.check_case(eng, name, c, device=eng.device)


def test_hook(eng):
    rc.check_hook(eng, device=eng.device)


def test_unaligned_views(eng):
    rc.check_views(eng, device=eng.device)


def test_after_an_error(eng):
    rc.check_after_an_error(eng, device=eng.device)


def test_empty(eng):
    rc.check_empty(eng, device=eng.device)


@pytest.mark.parametrize("c", rc.DEVICE_COUNTS)
@pytest.mark.parametrize("shape", rc.DEVICE_SHAPES, ids=lambda v: "x".join(map(str, v)))
def test_device_against_emulator(eng, shape, c):
    rc.check_device_against_emulator(eng, shape, c)
