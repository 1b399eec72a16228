"""The bf16x3 product of Iso-C on the MI355X: `iso_gemm3_nt` / `iso_gemm3_nn` of csrc/sm_iso3.hpp on
v_mfma_f32_32x32x16_bf16 (tests/iso_split_checks.py).  Exact integers decide the operand layout of the instruction and that
all six terms are there; the rest is held to the header's bound against fp64, never to the emulator's bits."""
import pytest
import torch

from tests import iso_split_checks as sc
from tests.harness import eng  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", sc.CASES)
def test_product(eng, case):
    sc.CASES[case](eng)


@pytest.mark.parametrize("shape", ((96, 160), (160, 96), (384, 2048)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_merge_against_svd(eng, shape):
    """the fp32 figures come from the emulator; at 384 x 2048, where its chains take more than a few seconds, from the
    device's fp32 path, which tests/test_iso_gpu.py holds to the emulator bit for bit"""
    from tests.emul.loader import emul_engine
    sc.check_merge(eng, eng if shape[1] > 1000 else emul_engine(), shape)
    torch.cuda.empty_cache()
