"""operator: sce on the MI355X: the kernels of csrc/sm_sce.hpp against tests/sce_oracle.py, bit for bit
(tests/sce_checks.py) - the parameter grid, the sizes, the properties and the corners of the emulator tier, model shapes
(each once: the CPU oracle takes seconds there; no 128256-row shape, so that every test stays within seconds), and the CLI
on the device."""
import pytest
import torch

from tests import lora_fixtures as lf
from tests import sce_checks as sc
from tests.harness import ALPHAS, DTYPES, KS, assert_outputs, eng, make_inputs, run_cli  # noqa: F401

pytestmark = pytest.mark.gpu

MODEL_SHAPES = [((4096, 4096), 3), ((4544, 4544), 3), ((11008, 4096), 2), ((1, 4096), 3)]


@pytest.mark.parametrize("bo_dtype", DTYPES, ids=str)
@pytest.mark.parametrize("in_dtype", DTYPES, ids=str)
def test_dtypes(eng, in_dtype, bo_dtype):
    sc.check_dtypes(eng, in_dtype, bo_dtype, device=eng.device)


@pytest.mark.parametrize("topk", sc.TOPKS)
@pytest.mark.parametrize("k", KS)
def test_k_and_select_topk(eng, k, topk):
    sc.check_k_topk(eng, k, topk, device=eng.device)


@pytest.mark.parametrize("n", sc.SIZES)
def test_sizes(eng, n):
    sc.check_sizes(eng, n, device=eng.device)


@pytest.mark.parametrize("check", sc.PROPERTIES + sc.CORNERS, ids=lambda f: f.__name__[len("check_"):])
def test_property_or_corner(eng, check):
    check(eng, device=eng.device)


@pytest.mark.parametrize("shape,k", MODEL_SHAPES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"k{v}")
def test_model_shape(eng, shape, k):
    fts, bases, bo = make_inputs(shape, k, seed=sum(shape) % 97, device=eng.device)
    rep, _ = sc.check(eng, fts, bases, ALPHAS[:k], bo, select_topk=0.1, lam=0.7, label=f"{shape} k={k}")
    assert rep.selected >= rep.k_keep > 0
    del fts, bases, bo
    torch.cuda.empty_cache()


def test_model_shape_with_own_bases(eng):
    fts, bases, bo = make_inputs((4096, 4096), 3, torch.bfloat16, torch.float32, seed=3, own_bases=True, device=eng.device)
    sc.check(eng, fts, bases, [0.5, 0.0, 0.4], bo, select_topk=0.05, label="4096^2, own bases, fp32 output")


@pytest.mark.parametrize("topk", [0.1, 1.0])
@pytest.mark.parametrize("k", [1, 2, 5, 16])
def test_profile_names_and_launches(eng, k, topk):
    sc.check_profile(eng, k, topk, shape=(1024, 1024), device=eng.device)


@pytest.mark.parametrize("inplace", [False, True], ids=["single_process", "inplace"])
def test_cli_on_the_device(tmp_path, eng, monkeypatch, inplace):
    if inplace:
        monkeypatch.setenv("SHARDMERGE_INPLACE", "1")
    base, factors, full = lf.setup_k3(tmp_path, eng)
    res = run_cli(sc.write_config(tmp_path, "org/lora", "merged", device="cuda"))
    assert res.exit_code == 0, res.output
    assert_outputs(tmp_path / "merged", sc.expected_outputs(base, full))
    readme = (tmp_path / "merged" / "README.md").read_text()
    for word in sc.README_WORDS:
        assert word in readme, (word, readme)
