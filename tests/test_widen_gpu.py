"""operator: widen on the MI355X: the kernels of csrc/sm_widen.hpp against tests/widen_oracle.py, bit for bit
(tests/widen_checks.py) - the parameter grid and the corners of the emulator tier, the column sums against math.fsum, the
paper's form in fp64, model-shaped cases (the smallest with many work-groups, several segments and the 128-register
variant of widen_combine; nothing larger than 2048 x 4096), two of them also against the emulator, and the CLI on the
device."""
import pytest
import torch

from tests import lora_fixtures as lf
from tests import widen_checks as wc
from tests.harness import ALPHAS, DTYPES, assert_outputs, eng, make_inputs, run_cli  # noqa: F401

pytestmark = pytest.mark.gpu

MODEL_SHAPES = [((1024, 4096), 3), ((300, 4544), 3), ((1030, 257), 5), ((1, 4096), 3)]
IDS = ["x".join(map(str, s)) + f"-k{k}" for s, k in MODEL_SHAPES]


@pytest.mark.parametrize("R", wc.ROWS)
def test_rows(eng, R):
    wc.check_rows(eng, R, device=eng.device)


@pytest.mark.parametrize("C", wc.COLS)
def test_cols(eng, C):
    wc.check_cols(eng, C, device=eng.device)


@pytest.mark.parametrize("own", [False, True], ids=["shared_base", "own_bases"])
@pytest.mark.parametrize("k", wc.KS)
def test_k(eng, k, own):
    wc.check_k(eng, k, own, device=eng.device)


@pytest.mark.parametrize("bo_dtype", DTYPES, ids=str)
@pytest.mark.parametrize("in_dtype", DTYPES, ids=str)
def test_dtypes(eng, in_dtype, bo_dtype):
    wc.check_dtypes(eng, in_dtype, bo_dtype, device=eng.device)


@pytest.mark.parametrize("lam", wc.LAMBDAS)
@pytest.mark.parametrize("calibration", wc.CALIBRATIONS)
@pytest.mark.parametrize("ratio", wc.RATIOS)
def test_options(eng, ratio, calibration, lam):
    wc.check_options(eng, ratio, calibration, lam, device=eng.device)


@pytest.mark.parametrize("check", wc.CORNERS, ids=lambda f: f.__name__[len("check_"):])
def test_corner(eng, check):
    check(eng, device=eng.device)


@pytest.mark.parametrize("shape,k", MODEL_SHAPES, ids=IDS)
def test_model_shape(eng, shape, k):
    fts, bases, bo = make_inputs(shape, k, seed=sum(shape) % 97, device=eng.device)
    rep, _, _, _ = wc.check(eng, fts, bases, ALPHAS[:k], bo, calibration=0.5, lam=0.7, label=f"{shape} k={k}")
    assert all(0 < c < rep.cols for row in rep.calibrated for c in row[:1 if rep.vector_mode else 2])
    del fts, bases, bo
    torch.cuda.empty_cache()


def test_model_shape_k16_with_own_bases(eng):
    """the 128-register variant of widen_combine over many work-groups and four segments"""
    fts, bases, bo = make_inputs((2048, 4096), 16, torch.bfloat16, torch.float32, seed=3, own_bases=True, device=eng.device)
    alphas = [a if i % 3 else -a for i, a in enumerate(ALPHAS)]
    wc.check(eng, fts, bases, alphas, bo, calibration=0.5, label="2048 x 4096 k=16, own bases, fp32 output")
    del fts, bases, bo
    torch.cuda.empty_cache()


@pytest.mark.parametrize("shape,k", MODEL_SHAPES[:2], ids=IDS[:2])
def test_device_equals_the_emulator(eng, shape, k):
    from tests.emul.loader import emul_engine
    wc.check_equals_emulator(eng, emul_engine(), shape, k, eng.device)


@pytest.mark.parametrize("shape,k,expected", wc.PROFILES, ids=wc.PROFILE_IDS)
def test_profile_names(eng, shape, k, expected):
    wc.check_profile(eng, shape, k, expected, device=eng.device)


def test_c_abi_rejects_bad_arguments(eng):
    wc.check_c_abi(eng, device=eng.device)


def test_column_sums_against_fsum(eng):
    wc.check_sums_against_fsum(eng, device=eng.device)


@pytest.mark.parametrize("shape,k", wc.PAPER_CASES, ids=["x".join(map(str, s)) + f"-k{k}" for s, k in wc.PAPER_CASES])
def test_paper_form_in_fp64(eng, shape, k):
    wc.check_paper_form(eng, shape, k, device=eng.device)


@pytest.mark.parametrize("inplace", [False, True], ids=["single_process", "inplace"])
def test_cli_on_the_device(tmp_path, eng, monkeypatch, inplace):
    if inplace:
        monkeypatch.setenv("SHARDMERGE_INPLACE", "1")
    base, factors, full = lf.setup_k3(tmp_path, eng)
    res = run_cli(wc.write_config(tmp_path, "org/lora", "merged", wc.OPTIONS, device="cuda"))
    assert res.exit_code == 0, res.output
    assert_outputs(tmp_path / "merged", wc.expected_outputs(eng, base, full, wc.OPTIONS))
    assert "WIDEN" in (tmp_path / "merged" / "README.md").read_text()
