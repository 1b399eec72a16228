"""GPTQ-layout INT4 on the MI355X: the kernels of csrc/sm_gptq.hpp against the plain restatement and the format's error
bound (tests/gptq_checks.py), and three model-like shapes against the emulator library."""
import pytest
import torch

from tests import gptq_checks as gc
from tests.harness import DTYPES, eng, raw  # noqa: F401

pytestmark = pytest.mark.gpu

# more work-groups than compute units; the long rows of an MLP; partial tiles at the middle group size
DEVICE_SHAPES = [(2048, 4096, 128), (16, 28672, 128), (136, 4544, 64)]


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("g", gc.GROUPS)
def test_shapes(eng, g, dtype):
    gc.check_shapes(eng, g, dtype, device=eng.device)


def test_views(eng):
    gc.check_views(eng, device=eng.device)


def test_forced_rounds(eng):
    gc.check_rounds(eng, device=eng.device)


@pytest.mark.parametrize("corner", gc.CORNERS, ids=lambda f: f.__name__[len("corner_"):])
def test_corner(eng, corner):
    corner(eng, eng.device)


@pytest.mark.parametrize("shape", DEVICE_SHAPES, ids=lambda v: "x".join(map(str, v)))
def test_device_against_emulator(eng, shape):
    from tests.emul.loader import emul_engine
    rows, cols, g = shape
    x = gc.weights((rows, cols), g, seed=sum(shape) % 97, device=eng.device)
    *four, rep = eng.gptq_quant(x, g)
    *efour, erep = emul_engine().gptq_quant(x.cpu(), g)
    assert all(torch.equal(raw(e), raw(d.cpu())) for e, d in zip(efour, four)) and erep == rep
    assert torch.equal(raw(emul_engine().gptq_dequant(*efour, torch.bfloat16)), raw(eng.gptq_dequant(*four, torch.bfloat16).cpu()))
