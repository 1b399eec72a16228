"""operator: ties on the MI355X: the kernels of csrc/sm_ties.hpp against tests/ties_oracle.py, bit for bit
(tests/ties_checks.py) - the parameter grid and the corners of the emulator tier, model shapes (each once: the CPU
oracle takes seconds to tens of seconds there), and the CLI on the device."""
import pytest
import torch

from tests import lora_fixtures as lf
from tests import ties_checks as tc
from tests.harness import ALPHAS, DTYPES, KS, assert_outputs, eng, make_inputs, run_cli  # noqa: F401

pytestmark = pytest.mark.gpu

# (shape, K): 4544 x 4544 is refused by the spectral merge's planner without the chirp-z path, here an ordinary shape;
# 128256 x 4096 has counts beyond 2^29
MODEL_SHAPES = [((4096, 4096), 3), ((8192, 8192), 3), ((28672, 8192), 2), ((8192, 28672), 2), ((11008, 4096), 3),
                ((4544, 4544), 3), ((128256, 4096), 2), ((1, 4096), 3)]


@pytest.mark.parametrize("bo_dtype", DTYPES, ids=str)
@pytest.mark.parametrize("in_dtype", DTYPES, ids=str)
def test_dtypes(eng, in_dtype, bo_dtype):
    tc.check_dtypes(eng, in_dtype, bo_dtype, device=eng.device)


@pytest.mark.parametrize("density", tc.DENSITIES)
@pytest.mark.parametrize("k", KS)
def test_k_and_density(eng, k, density):
    tc.check_k_density(eng, k, density, device=eng.device)


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("lam", [1.0, 0.7])
def test_lambda_and_normalize(eng, lam, normalize):
    tc.check_lambda_normalize(eng, lam, normalize, device=eng.device)


@pytest.mark.parametrize("check", [tc.check_signed_alphas, tc.check_zero_delta, tc.check_opposite_deltas,
                                   tc.check_tiny_weight_sum, tc.check_ties_exceed_k, tc.check_denormals, tc.check_unaligned,
                                   tc.check_tiny_and_rank3, tc.check_nonfinite, tc.check_determinism, tc.check_arguments],
                         ids=lambda f: f.__name__[len("check_"):])
def test_corner(eng, check):
    check(eng, device=eng.device)


@pytest.mark.parametrize("shape,k", MODEL_SHAPES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"k{v}")
def test_model_shape(eng, shape, k):
    fts, bases, bo = make_inputs(shape, k, seed=sum(shape) % 97, device=eng.device)
    rep = tc.check(eng, fts, bases, ALPHAS[:k], bo, density=0.2, lam=0.7, label=f"{shape} k={k}")
    assert all(kept >= rep.k_keep for kept in rep.kept)
    del fts, bases, bo
    torch.cuda.empty_cache()


def test_model_shape_with_own_bases(eng):
    fts, bases, bo = make_inputs((4096, 4096), 3, torch.bfloat16, torch.float32, seed=3, own_bases=True, device=eng.device)
    tc.check(eng, fts, bases, [0.5, -0.3, 0.4], bo, density=0.05, normalize=False, label="4096^2, own bases, fp32 output")


def test_profile_names(eng):
    fts, bases, bo = make_inputs((1024, 1024), 2, seed=4, device=eng.device)
    eng.ctx.profile(True)
    eng.ctx.profile_reset()
    try:
        eng.ties_merge(fts, bases, ALPHAS[:2], bo)
        table = eng.ctx.profile_table()
    finally:
        eng.ctx.profile(False)
    assert {n: table[n][0] for n in table} == {"ties_hist": 3, "ties_select": 3, "ties_merge": 1}


@pytest.mark.parametrize("inplace", [False, True], ids=["single_process", "inplace"])
def test_cli_on_the_device(tmp_path, eng, monkeypatch, inplace):
    if inplace:
        monkeypatch.setenv("SHARDMERGE_INPLACE", "1")
    base, factors, full = lf.setup_k3(tmp_path, eng)
    res = run_cli(tc.write_config(tmp_path, "org/lora", "merged", device="cuda"))
    assert res.exit_code == 0, res.output
    assert_outputs(tmp_path / "merged", tc.expected_outputs(base, full))
    assert "TIES" in (tmp_path / "merged" / "README.md").read_text()
