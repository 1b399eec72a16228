"""operator: dare_ties / dare_linear on the MI355X: the kernel of csrc/sm_dare.hpp against tests/dare_oracle.py, bit for
bit (tests/dare_checks.py) - the parameter grid and the corners of the emulator tier, the two identities, the
statistics, model shapes (each once, alternating the two modes: the numpy mask takes seconds to tens of seconds there),
and the CLI on the device."""
import pytest
import torch

from tests import dare_checks as dc
from tests import lora_fixtures as lf
from tests.harness import ALPHAS, DTYPES, KS, assert_outputs, eng, make_inputs, run_cli  # noqa: F401
from tests.test_ties_gpu import MODEL_SHAPES

pytestmark = pytest.mark.gpu

MODE_IDS = ["dare_ties", "dare_linear"]


@pytest.mark.parametrize("sign_election", dc.MODES, ids=MODE_IDS)
@pytest.mark.parametrize("bo_dtype", DTYPES, ids=str)
@pytest.mark.parametrize("in_dtype", DTYPES, ids=str)
def test_dtypes(eng, in_dtype, bo_dtype, sign_election):
    dc.check_dtypes(eng, in_dtype, bo_dtype, sign_election, device=eng.device)


@pytest.mark.parametrize("sign_election", dc.MODES, ids=MODE_IDS)
@pytest.mark.parametrize("density", dc.DENSITIES)
@pytest.mark.parametrize("k", KS)
def test_k_and_density(eng, k, density, sign_election):
    dc.check_k_density(eng, k, density, sign_election, device=eng.device)


@pytest.mark.parametrize("sign_election", dc.MODES, ids=MODE_IDS)
@pytest.mark.parametrize("rescale", [True, False])
@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("lam", [1.0, 0.7])
def test_lambda_normalize_rescale(eng, lam, normalize, rescale, sign_election):
    dc.check_options(eng, lam, normalize, rescale, sign_election, device=eng.device)


CORNERS = [dc.check_signed_alphas, dc.check_zero_delta, dc.check_tiny_weight_sum, dc.check_denormals, dc.check_unaligned,
           dc.check_tiny_and_rank3, dc.check_nonfinite, dc.check_arguments, dc.check_density_one_is_ties, dc.check_nested_masks,
           dc.check_determinism, dc.check_slices, dc.check_streams_and_keys]


@pytest.mark.parametrize("check", CORNERS, ids=lambda f: f.__name__[len("check_"):])
def test_corner(eng, check):
    check(eng, device=eng.device)


@pytest.mark.parametrize("density", dc.DENSITIES)
def test_statistics(eng, density):
    dc.check_statistics(eng, density, device=eng.device)


@pytest.mark.parametrize("case", list(enumerate(MODEL_SHAPES)), ids=lambda c: "x".join(map(str, c[1][0])) + f"-k{c[1][1]}-" + MODE_IDS[c[0] % 2])
def test_model_shape(eng, case):
    i, (shape, k) = case
    fts, bases, bo = make_inputs(shape, k, seed=sum(shape) % 97, device=eng.device)
    rep = dc.check(eng, fts, bases, ALPHAS[:k], bo, density=0.2, lam=0.7, sign_election=i % 2 == 0, label=f"{shape} k={k}")
    assert rep.threshold == 13107 and all(0 < kept < bo.numel() for kept in rep.kept)
    del fts, bases, bo
    torch.cuda.empty_cache()


def test_model_shape_with_own_bases(eng):
    fts, bases, bo = make_inputs((4096, 4096), 3, torch.bfloat16, torch.float32, seed=3, own_bases=True, device=eng.device)
    dc.check(eng, fts, bases, [0.5, -0.3, 0.4], bo, density=0.05, normalize=False, sign_election=False, stream_ids=[0, 2, 5],
             label="4096^2, own bases, fp32 output")


def test_profile_names(eng):
    fts, bases, bo = make_inputs((1024, 1024), 2, seed=4, device=eng.device)
    eng.ctx.profile(True)
    eng.ctx.profile_reset()
    try:
        eng.dare_merge(fts, bases, ALPHAS[:2], bo)
        table = eng.ctx.profile_table()
    finally:
        eng.ctx.profile(False)
    assert {n: table[n][0] for n in table} == {"dare_merge": 1}


@pytest.mark.parametrize("operator", ["dare_ties", "dare_linear"])
@pytest.mark.parametrize("inplace", [False, True], ids=["single_process", "inplace"])
def test_cli_on_the_device(tmp_path, eng, monkeypatch, inplace, operator):
    if inplace:
        monkeypatch.setenv("SHARDMERGE_INPLACE", "1")
    base, factors, full = lf.setup_k3(tmp_path, eng)
    opts = dc.options(operator)
    res = run_cli(dc.write_config(tmp_path, "org/lora", "merged", opts, device="cuda"))
    assert res.exit_code == 0, res.output
    assert_outputs(tmp_path / "merged", dc.expected_outputs(base, full, opts))
    assert "DARE" in (tmp_path / "merged" / "README.md").read_text()
