"""NVFP4 on the MI355X: the kernels of csrc/sm_nv4.hpp against the plain restatement and the format's error bound
(tests/nv4_checks.py), and two model-like shapes against the emulator library."""
import pytest
import torch

from tests import nv4_checks as nc
from tests.harness import DTYPES, eng, raw  # noqa: F401

pytestmark = pytest.mark.gpu

# more work-groups than compute units; the long rows of an MLP
DEVICE_SHAPES = [(2048, 4096), (16, 28672)]


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("rows", nc.ROWS)
def test_shapes(eng, rows, dtype):
    nc.check_shapes(eng, rows, dtype, device=eng.device)


def test_views(eng):
    nc.check_views(eng, device=eng.device)


def test_forced_rounds(eng):
    nc.check_rounds(eng, device=eng.device)


@pytest.mark.parametrize("corner", nc.CORNERS, ids=lambda f: f.__name__[len("corner_"):])
def test_corner(eng, corner):
    corner(eng, eng.device)


@pytest.mark.parametrize("shape", DEVICE_SHAPES, ids=lambda v: "x".join(map(str, v)))
def test_device_against_emulator(eng, shape):
    from tests.emul.loader import emul_engine
    x = nc.weights(shape, seed=sum(shape) % 97, device=eng.device)
    codes, sc, g, rep = eng.nv4_quant(x)
    ecodes, esc, eg, erep = emul_engine().nv4_quant(x.cpu())
    assert torch.equal(ecodes, codes.cpu()) and torch.equal(esc.view(torch.uint8), sc.cpu().view(torch.uint8)) and torch.equal(raw(eg), raw(g)) and erep == rep
    assert torch.equal(raw(emul_engine().nv4_dequant(ecodes, esc, eg, torch.bfloat16)), raw(eng.nv4_dequant(codes, sc, g, torch.bfloat16)))


def test_commands_and_merge_on_the_device(tmp_path, eng):
    nc.check_commands_and_merge(tmp_path, eng, "cuda")
