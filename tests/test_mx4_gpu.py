"""MXFP4 on the MI355X: the kernels of csrc/sm_mx4.hpp against the exact restatement and the format's error bound
(tests/mx4_checks.py), and three model-like shapes against the emulator library."""
import pytest
import torch

from tests import mx4_checks as mc
from tests.harness import DTYPES, eng, raw  # noqa: F401

pytestmark = pytest.mark.gpu

# more work-groups than compute units; a last work-group that is partial; the long rows of an MLP
DEVICE_SHAPES = [(2048, 4096), (300, 4544), (16, 28672)]


def test_conversions_exhaustively(eng):
    mc.check_conversions(eng)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("rows", mc.ROWS)
def test_shapes(eng, rows, dtype):
    mc.check_shapes(eng, rows, dtype, device=eng.device)


def test_views(eng):
    mc.check_views(eng, device=eng.device)


@pytest.mark.parametrize("corner", mc.CORNERS, ids=lambda f: f.__name__[len("corner_"):])
def test_corner(eng, corner):
    corner(eng, eng.device)


def test_error_bound_in_fp64(eng):
    mc.check_error_bound(eng, device=eng.device)


@pytest.mark.parametrize("shape", DEVICE_SHAPES, ids=lambda v: "x".join(map(str, v)))
def test_device_against_emulator(eng, shape):
    from tests.emul.loader import emul_engine
    x = mc.weights(shape, seed=sum(shape) % 97, device=eng.device)
    codes, sc, rep = eng.mx4_quant(x)
    ecodes, esc, erep = emul_engine().mx4_quant(x.cpu())
    assert torch.equal(ecodes, codes.cpu()) and torch.equal(esc, sc.cpu()) and erep == rep
    assert torch.equal(raw(emul_engine().mx4_dequant(ecodes, esc, torch.bfloat16)), raw(eng.mx4_dequant(codes, sc, torch.bfloat16)))


def test_commands_and_merge_on_the_device(tmp_path, eng):
    mc.check_commands_and_merge(tmp_path, eng, "cuda")


def test_odd_columns_are_copied_on_the_device(tmp_path, eng):
    mc.check_odd_columns(tmp_path, eng, "cuda")
