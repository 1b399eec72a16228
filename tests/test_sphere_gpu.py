"""operators karcher / multislerp on the MI355X: the kernels of csrc/sm_sphere.hpp and csrc/sm_geo.hpp against
tests/sphere_oracle.py, bit for bit (tests/sphere_checks.py) - the parameter grid, the three functions on the host and the
device, the properties and the corners of the emulator tier, one model shape per code path, and the CLI on the device."""
import pytest
import torch

from tests import lora_fixtures as lf
from tests import sphere_checks as sc
from tests.harness import ALPHAS, DTYPES, KS, assert_outputs, eng, make_inputs, run_cli  # noqa: F401

pytestmark = pytest.mark.gpu

# (shape, k, mode, rowwise): 4096^2 at K = 3 whole and row-wise (the register instantiation of sphere_coef), 11008 rows at
# K = 2, and k = 16 row-wise (ten tiles of pairs, the LDS instantiation at its smallest work-group)
SHAPE_CASES = [((4096, 4096), 3, "karcher", False), ((4096, 4096), 3, "multislerp", True), ((11008, 4096), 2, "multislerp", True),
               ((4096, 4096), 16, "karcher", True)]


@pytest.mark.parametrize("mode,rowwise", sc.VARIANTS, ids=sc.VARIANT_IDS)
@pytest.mark.parametrize("bo_dtype", DTYPES, ids=str)
@pytest.mark.parametrize("in_dtype", DTYPES, ids=str)
def test_dtypes(eng, in_dtype, bo_dtype, mode, rowwise):
    sc.check_dtypes(eng, in_dtype, bo_dtype, mode, rowwise, device=eng.device)


@pytest.mark.parametrize("mode,rowwise", sc.VARIANTS, ids=sc.VARIANT_IDS)
@pytest.mark.parametrize("k", KS)
def test_k(eng, k, mode, rowwise):
    sc.check_k(eng, k, mode, rowwise, device=eng.device)


def test_functions(eng):
    sc.check_functions(eng, device=eng.device)


@pytest.mark.parametrize("check", sc.PROPERTIES + sc.CORNERS, ids=lambda f: f.__name__[len("check_"):])
def test_property_or_corner(eng, check):
    check(eng, device=eng.device)


@pytest.mark.parametrize("shape,k,mode,rowwise", SHAPE_CASES,
                         ids=["x".join(map(str, c[0])) + f"-k{c[1]}-{c[2]}{'-rowwise' if c[3] else ''}" for c in SHAPE_CASES])
def test_model_shape(eng, shape, k, mode, rowwise):
    fts, bases, bo = make_inputs(shape, k, seed=sum(shape) % 97 + k, device=eng.device)
    sc.check(eng, fts, bases, ALPHAS[:k], bo, mode, rowwise, label=f"{shape} k={k} {mode}")
    del fts, bases, bo
    torch.cuda.empty_cache()


@pytest.mark.parametrize("k", [2, 5, 16])
@pytest.mark.parametrize("mode,rowwise", sc.VARIANTS, ids=sc.VARIANT_IDS)
def test_profile_names_and_launches(eng, mode, rowwise, k):
    sc.check_profile(eng, mode, rowwise, k, shape=(1024, 1024), device=eng.device)


@pytest.mark.parametrize("operator,row_wise", [("karcher", None), ("karcher", 1), ("multislerp", None), ("multislerp", 1)],
                         ids=["karcher", "karcher_row_wise", "multislerp", "multislerp_row_wise"])
def test_cli_on_the_device(tmp_path, eng, operator, row_wise):
    base, factors, full = lf.setup_k3(tmp_path, eng)
    opts = sc.options(operator, row_wise)
    res = run_cli(sc.write_config(tmp_path, "org/lora", "merged", opts, device="cuda"))
    assert res.exit_code == 0, res.output
    assert_outputs(tmp_path / "merged", sc.expected_outputs(base, full, opts))
    readme = (tmp_path / "merged" / "README.md").read_text()
    for word in sc.README_WORDS[operator]:
        assert word in readme, (word, readme)
