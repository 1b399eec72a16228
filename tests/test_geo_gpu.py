"""operators model_stock / nuslerp / slerp on the MI355X: the kernels of csrc/sm_geo.hpp against tests/geo_oracle.py, bit
for bit (tests/geo_checks.py) - the parameter grid, the properties and the corners of the emulator tier, the model shapes
of tests/test_ties_gpu.py (each once, the operators alternating: the CPU oracle takes seconds to tens of seconds there),
and the CLI on the device."""
import pytest
import torch

from tests import geo_checks as gc
from tests import lora_fixtures as lf
from tests.harness import ALPHAS, DTYPES, KS, assert_outputs, eng, make_inputs, run_cli  # noqa: F401
from tests.test_ties_gpu import MODEL_SHAPES

pytestmark = pytest.mark.gpu

# the operator variant of each model shape, in turn; nuslerp / slerp take two of the finetunes
SHAPE_CASES = [(shape, k, *gc.VARIANTS[i % len(gc.VARIANTS)]) for i, (shape, k) in enumerate(MODEL_SHAPES)]


@pytest.mark.parametrize("mode,rowwise", gc.VARIANTS, ids=gc.VARIANT_IDS)
@pytest.mark.parametrize("bo_dtype", DTYPES, ids=str)
@pytest.mark.parametrize("in_dtype", DTYPES, ids=str)
def test_dtypes(eng, in_dtype, bo_dtype, mode, rowwise):
    gc.check_dtypes(eng, in_dtype, bo_dtype, mode, rowwise, device=eng.device)


@pytest.mark.parametrize("rowwise", [False, True], ids=["whole", "rowwise"])
@pytest.mark.parametrize("k", KS)
def test_model_stock_k(eng, k, rowwise):
    gc.check_k(eng, k, rowwise, device=eng.device)


@pytest.mark.parametrize("check", gc.PROPERTIES + gc.CORNERS, ids=lambda f: f.__name__[len("check_"):])
def test_property_or_corner(eng, check):
    check(eng, device=eng.device)


@pytest.mark.parametrize("shape,k,mode,rowwise", SHAPE_CASES,
                         ids=["x".join(map(str, c[0])) + f"-k{c[1]}-{c[2]}{'-rowwise' if c[3] else ''}" for c in SHAPE_CASES])
def test_model_shape(eng, shape, k, mode, rowwise):
    k = gc.variant_k(mode, k)
    fts, bases, bo = make_inputs(shape, k, seed=sum(shape) % 97, device=eng.device)
    gc.check(eng, fts, bases, ALPHAS[:k], bo, mode, rowwise, label=f"{shape} k={k} {mode}")
    del fts, bases, bo
    torch.cuda.empty_cache()


def test_model_shape_with_own_bases(eng):
    fts, bases, bo = make_inputs((4096, 4096), 3, torch.bfloat16, torch.float32, seed=3, own_bases=True, device=eng.device)
    gc.check(eng, fts, bases, [0.5, -0.3, 0.4], bo, "model_stock", label="4096^2, own bases, fp32 output")
    gc.check(eng, fts, bases, [0.5, -0.3, 0.4], bo, "model_stock", True, label="4096^2, own bases, fp32 output, row-wise")


@pytest.mark.parametrize("k", [2, 5, 16])
@pytest.mark.parametrize("mode,rowwise", gc.VARIANTS, ids=gc.VARIANT_IDS)
def test_profile_names_and_launches(eng, mode, rowwise, k):
    gc.check_profile(eng, mode, rowwise, gc.variant_k(mode, k), shape=(1024, 1024), device=eng.device)


@pytest.mark.parametrize("inplace", [False, True], ids=["single_process", "inplace"])
@pytest.mark.parametrize("operator,filter_wise", [("model_stock", None), ("model_stock", 1), ("nuslerp", None), ("slerp", None)],
                         ids=["model_stock", "model_stock_filter_wise", "nuslerp", "slerp"])
def test_cli_on_the_device(tmp_path, eng, monkeypatch, operator, filter_wise, inplace):
    if inplace:
        monkeypatch.setenv("SHARDMERGE_INPLACE", "1")
    base, factors, full = lf.setup_k3(tmp_path, eng)
    opts = gc.options(operator, filter_wise)
    res = run_cli(gc.write_config(tmp_path, "org/lora", "merged", opts, device="cuda"))
    assert res.exit_code == 0, res.output
    assert_outputs(tmp_path / "merged", gc.expected_outputs(base, full, opts))
    readme = (tmp_path / "merged" / "README.md").read_text()
    for word in gc.README_WORDS[operator]:
        assert word in readme, (word, readme)
