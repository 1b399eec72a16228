"""The delta pack on the MI355X: the kernels of csrc/sm_dpack.hpp against tests/dpack_oracle.py bit for bit and against
torch fp64 (tests/dpack_checks.py) - the grid and the corners of the emulator tier, three model-like shapes, two of them
against the emulator library as well."""
import pytest
import torch

from tests import dpack_checks as dc
from tests.harness import DTYPES, eng, raw  # noqa: F401

pytestmark = pytest.mark.gpu

# 300 x 4544: rows that are no multiple of the lanes' wrap; 16 x 28672: 14 octets per lane; the first two also run on
# the emulator (its row pass takes a second per 10^7 elements)
DEVICE_SHAPES = [((2048, 4096), True), ((300, 4544), True), ((16, 28672), False)]


@pytest.mark.parametrize("cols", dc.COLS)
def test_cols(eng, cols):
    dc.check_cols(eng, cols, device=eng.device)


@pytest.mark.parametrize("rows", dc.ROWS)
def test_rows(eng, rows):
    dc.check_rows(eng, rows, device=eng.device)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_dtypes(eng, dtype):
    dc.check_dtypes(eng, dtype, device=eng.device)


@pytest.mark.parametrize("check", dc.CORNERS, ids=lambda f: f.__name__[len("check_"):])
def test_corner(eng, check):
    check(eng, device=eng.device)


@pytest.mark.parametrize("shape,on_emulator", DEVICE_SHAPES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else None)
def test_device_shape(eng, shape, on_emulator):
    ft, base = dc.pair(shape, seed=sum(shape) % 97, device=eng.device)
    for bits, density, scale in ((1, 1.0, "row"), (2, 0.2, "row"), (2, 0.2, "tensor")):
        sign, mask, sc, rep, out = dc.check(eng, ft, base, bits, density, scale, f"{shape} bits={bits} {scale}")
        if on_emulator and bits == 2:
            from tests.emul.loader import emul_engine
            em = emul_engine()
            esign, emask, esc, erep = em.delta_pack(ft.cpu(), base.cpu(), bits=bits, density=density, scale=scale)
            assert torch.equal(esign, sign.cpu()) and torch.equal(emask, mask.cpu()) and torch.equal(raw(esc), raw(sc)) and erep == rep
            assert torch.equal(raw(em.delta_apply(base.cpu(), esign, emask, esc)), raw(out))


def test_command_and_merge_on_the_device(tmp_path, eng):
    dc.check_command(tmp_path, eng, "cuda")


def test_one_bit_pack_with_modules_on_the_device(tmp_path, eng):
    dc.check_command_forms(tmp_path, eng, "cuda")
