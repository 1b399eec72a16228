"""operator: pcb on the MI355X: the kernels of csrc/sm_pcb.hpp (and the selection kernels of the task-vector statistics)
against tests/pcb_oracle.py, bit for bit (tests/pcb_checks.py) - the parameter grid and the corners of the emulator
tier, sm_tanh through the probe kernel, the paper's form in fp64, model-shaped cases (the smallest at which the device
path differs from the emulator's: many work-groups, several octets per thread; nothing larger, the numpy oracle sorts and
takes seconds), and the CLI on the device."""
import pytest
import torch

from tests import lora_fixtures as lf
from tests import pcb_checks as pc
from tests.harness import ALPHAS, DTYPES, assert_outputs, eng, make_inputs, run_cli  # noqa: F401

pytestmark = pytest.mark.gpu

MODEL_SHAPES = [((1024, 4096), 3), ((300, 4544), 3), ((128, 11008), 5), ((1, 4096), 3)]


@pytest.mark.parametrize("bo_dtype", DTYPES, ids=str)
@pytest.mark.parametrize("in_dtype", DTYPES, ids=str)
def test_dtypes(eng, in_dtype, bo_dtype):
    pc.check_dtypes(eng, in_dtype, bo_dtype, device=eng.device)


@pytest.mark.parametrize("own", [False, True], ids=["shared_base", "own_bases"])
@pytest.mark.parametrize("k", pc.KS)
def test_k(eng, k, own):
    pc.check_k(eng, k, own, device=eng.device)


@pytest.mark.parametrize("lam", pc.LAMBDAS)
@pytest.mark.parametrize("clip", pc.CLIPS)
@pytest.mark.parametrize("ratio", pc.RATIOS)
def test_options(eng, ratio, clip, lam):
    pc.check_options(eng, ratio, clip, lam, device=eng.device)


@pytest.mark.parametrize("n", pc.SIZES)
def test_sizes(eng, n):
    pc.check_size(eng, n, device=eng.device)


@pytest.mark.parametrize("check", pc.CORNERS, ids=lambda f: f.__name__[len("check_"):])
def test_corner(eng, check):
    check(eng, device=eng.device)


@pytest.mark.parametrize("shape,k", MODEL_SHAPES, ids=["x".join(map(str, s)) + f"-k{k}" for s, k in MODEL_SHAPES])
def test_model_shape(eng, shape, k):
    fts, bases, bo = make_inputs(shape, k, seed=sum(shape) % 97, device=eng.device)
    rep, _, _, _ = pc.check(eng, fts, bases, ALPHAS[:k], bo, lam=0.7, label=f"{shape} k={k}")
    assert 0 < rep.covered < rep.n
    del fts, bases, bo
    torch.cuda.empty_cache()


def test_model_shape_k16_with_own_bases(eng):
    """the 128-register variants over many work-groups: four pcb_hist launches per level, several octets per thread"""
    fts, bases, bo = make_inputs((2048, 4096), 16, torch.bfloat16, torch.float32, seed=3, own_bases=True, device=eng.device)
    alphas = [a if i % 3 else -a for i, a in enumerate(ALPHAS)]
    rep, _, _, _ = pc.check(eng, fts, bases, alphas, bo, label="2048 x 4096 k=16, own bases, fp32 output")
    assert 0 < rep.covered < rep.n
    del fts, bases, bo
    torch.cuda.empty_cache()


@pytest.mark.parametrize("k,expected", pc.PROFILES, ids=pc.PROFILE_IDS)
def test_profile_names(eng, k, expected):
    pc.check_profile(eng, k, expected, shape=(1024, 1024), device=eng.device)


def test_c_abi_rejects_bad_arguments(eng):
    pc.check_c_abi(eng, device=eng.device)


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "kernel"])
def test_sm_tanh(eng, on_device):
    pc.check_tanh(eng, on_device)


@pytest.mark.parametrize("k", [2, 3, 5])
@pytest.mark.parametrize("n", [2 ** 16, 2 ** 20])
def test_paper_form_in_fp64(eng, n, k):
    pc.check_paper_form(eng, n, k, device=eng.device)


@pytest.mark.parametrize("inplace", [False, True], ids=["single_process", "inplace"])
def test_cli_on_the_device(tmp_path, eng, monkeypatch, inplace):
    if inplace:
        monkeypatch.setenv("SHARDMERGE_INPLACE", "1")
    base, factors, full = lf.setup_k3(tmp_path, eng)
    res = run_cli(pc.write_config(tmp_path, "org/lora", "merged", pc.OPTIONS, device="cuda"))
    assert res.exit_code == 0, res.output
    assert_outputs(tmp_path / "merged", pc.expected_outputs(base, full, pc.OPTIONS))
    assert "PCB" in (tmp_path / "merged" / "README.md").read_text()
