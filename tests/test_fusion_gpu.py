"""operator: arcee_fusion / nearswap on the MI355X: the kernels of csrc/sm_fusion.hpp against tests/fusion_oracle.py, bit
for bit (tests/fusion_checks.py) - sm_exp and sm_log on the device, the row KLs and the whole call over the shapes of the
emulator tier plus the sizes at which the device path differs from the emulator's (257 rows of 28672, many work-groups,
several octets per thread: 2048 x 4096 and 16 x 28672), the corners, the identities, the launch counts, the C ABI and
the CLI on the device."""
import pytest
import torch

from tests import fusion_checks as fc
from tests import lora_fixtures as lf
from tests.harness import DTYPES, assert_outputs, eng, run_cli, write_config  # noqa: F401

pytestmark = pytest.mark.gpu

MODEL_SHAPES = [(2048, 4096), (16, 28672)]


def test_sm_exp_and_sm_log(eng):
    fc.check_functions(eng, device=eng.device)


@pytest.mark.parametrize("R", fc.ROWS)
@pytest.mark.parametrize("C", fc.COLS)
def test_shapes(eng, C, R):
    fc.check_shape(eng, C, R, device=eng.device)


@pytest.mark.parametrize("bo_dtype", DTYPES, ids=str)
@pytest.mark.parametrize("in_dtype", DTYPES, ids=str)
def test_dtypes(eng, in_dtype, bo_dtype):
    fc.check_dtypes(eng, in_dtype, bo_dtype, device=eng.device)


@pytest.mark.parametrize("check", fc.CORNERS, ids=lambda f: f.__name__[len("check_"):])
def test_corner(eng, check):
    check(eng, device=eng.device)


@pytest.mark.parametrize("shape", MODEL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_model_shape(eng, shape):
    ft, base, bo = fc.fusion_inputs(shape, torch.bfloat16, torch.float32, seed=sum(shape) % 97, device=eng.device)
    fc.check(eng, ft, base, bo, "arcee", label=f"arcee {shape}")
    fc.check(eng, ft, base, bo, "nearswap", t=1e-3, label=f"nearswap {shape}")
    del ft, base, bo
    torch.cuda.empty_cache()


@pytest.mark.parametrize("mode,expected", fc.PROFILES, ids=[p[0] for p in fc.PROFILES])
def test_profile_names(eng, mode, expected):
    fc.check_profile(eng, mode, expected, shape=(1024, 1024), device=eng.device)


def test_c_abi_rejects_bad_arguments(eng):
    fc.check_c_abi(eng, device=eng.device)


@pytest.mark.parametrize("operator", ["arcee_fusion", "nearswap"])
@pytest.mark.parametrize("inplace", [False, True], ids=["single_process", "inplace"])
def test_cli_on_the_device(tmp_path, eng, monkeypatch, inplace, operator):
    if inplace:
        monkeypatch.setenv("SHARDMERGE_INPLACE", "1")
    base, factors, full = lf.setup_k3(tmp_path, eng)
    opts = fc.options(operator)
    res = run_cli(write_config(tmp_path, fc.models("org/lora"), "merged", opts, device="cuda"))
    assert res.exit_code == 0, res.output
    assert_outputs(tmp_path / "merged", fc.expected_outputs(base, full, opts))
    assert ("Arcee Fusion" if operator == "arcee_fusion" else "NearSwap") in (tmp_path / "merged" / "README.md").read_text()
