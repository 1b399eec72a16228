"""Block-scaled FP8 on the MI355X: the kernels of csrc/sm_fp8.hpp against torch on the CPU bit for bit and against the
format's error bound in fp64 (tests/fp8_checks.py) - the grid and the corners of the emulator tier, and three
model-like shapes, two of them against the emulator library as well."""
import pytest
import torch

from tests import fp8_checks as fc
from tests.harness import DTYPES, eng, raw  # noqa: F401

pytestmark = pytest.mark.gpu

# 2048 x 4096: whole blocks only, more blocks than compute units; 300 x 4544: partial blocks on both edges beside whole
# ones; 16 x 28672: one partial block row, 224 block columns.  The first two also run on the emulator.
DEVICE_SHAPES = [((2048, 4096), True), ((300, 4544), True), ((16, 28672), False)]


def test_conversions_exhaustively(eng):
    fc.check_conversions(eng, device=eng.device)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("rows", fc.ROWS)
def test_grid(eng, rows, dtype):
    fc.check_grid(eng, rows, dtype, device=eng.device)


def test_views(eng):
    fc.check_views(eng, device=eng.device)


@pytest.mark.parametrize("corner", fc.CORNERS, ids=lambda f: f.__name__[len("corner_"):])
def test_corner(eng, corner):
    corner(eng, eng.device)


def test_error_bound_in_fp64(eng):
    fc.check_error_bound(eng, device=eng.device)


@pytest.mark.parametrize("shape,on_emulator", DEVICE_SHAPES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else None)
def test_device_shape(eng, shape, on_emulator):
    x = fc.weights(shape, seed=sum(shape) % 97, device=eng.device)
    codes, sc, rep = fc.check(eng, x, f"{shape}", out_dtypes=(torch.bfloat16,))
    if on_emulator:
        from tests.emul.loader import emul_engine
        em = emul_engine()
        ecodes, esc, erep = em.fp8_quant(x.cpu())
        assert torch.equal(ecodes.view(torch.uint8), codes.cpu().view(torch.uint8)) and torch.equal(raw(esc), raw(sc)) and erep == rep
        assert torch.equal(raw(em.fp8_dequant(ecodes, esc, torch.bfloat16)), raw(eng.fp8_dequant(codes, sc, torch.bfloat16)))


def test_commands_and_merge_on_the_device(tmp_path, eng):
    fc.check_commands_and_merge(tmp_path, eng, "cuda")
