"""operator: breadcrumbs / breadcrumbs_ties on the MI355X: the kernels of csrc/sm_breadcrumbs.hpp against
tests/breadcrumbs_oracle.py, bit for bit (tests/breadcrumbs_checks.py) - the parameter grid and the corners of the emulator
tier, the two identities, model shapes (each once, alternating the two modes: the CPU oracle takes seconds to tens of
seconds there), and the CLI on the device."""
import pytest
import torch

from tests import breadcrumbs_checks as bc
from tests import lora_fixtures as lf
from tests.harness import ALPHAS, DTYPES, KS, assert_outputs, eng, make_inputs, run_cli  # noqa: F401

pytestmark = pytest.mark.gpu

MODE_IDS = ["breadcrumbs_ties", "breadcrumbs"]
# the model shapes of tests/test_ties_gpu.py
MODEL_SHAPES = [((4096, 4096), 3), ((8192, 8192), 3), ((28672, 8192), 2), ((8192, 28672), 2), ((11008, 4096), 3),
                ((4544, 4544), 3), ((128256, 4096), 2), ((1, 4096), 3)]


@pytest.mark.parametrize("sign_election", bc.MODES, ids=MODE_IDS)
@pytest.mark.parametrize("bo_dtype", DTYPES, ids=str)
@pytest.mark.parametrize("in_dtype", DTYPES, ids=str)
def test_dtypes(eng, in_dtype, bo_dtype, sign_election):
    bc.check_dtypes(eng, in_dtype, bo_dtype, sign_election, device=eng.device)


@pytest.mark.parametrize("sign_election", bc.MODES, ids=MODE_IDS)
@pytest.mark.parametrize("density,gamma", bc.DENSITY_GAMMA)
@pytest.mark.parametrize("k", KS)
def test_k_density_gamma(eng, k, density, gamma, sign_election):
    bc.check_k_density_gamma(eng, k, density, gamma, sign_election, device=eng.device)


@pytest.mark.parametrize("sign_election", bc.MODES, ids=MODE_IDS)
@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("lam", [1.0, 0.7])
def test_lambda_and_normalize(eng, lam, normalize, sign_election):
    bc.check_lambda_normalize(eng, lam, normalize, sign_election, device=eng.device)


@pytest.mark.parametrize("check", bc.CORNERS, ids=lambda f: f.__name__[len("check_"):])
def test_corner(eng, check):
    check(eng, device=eng.device)


@pytest.mark.parametrize("case", list(enumerate(MODEL_SHAPES)), ids=lambda c: "x".join(map(str, c[1][0])) + f"-k{c[1][1]}-" + MODE_IDS[c[0] % 2])
def test_model_shape(eng, case):
    i, (shape, k) = case
    fts, bases, bo = make_inputs(shape, k, seed=sum(shape) % 97, device=eng.device)
    rep = bc.check(eng, fts, bases, ALPHAS[:k], bo, density=0.9, gamma=0.01, lam=0.7, sign_election=i % 2 == 0, label=f"{shape} k={k}")
    assert all(kept >= rep.k_keep for kept in rep.kept) and all(d <= rep.n_top for d in rep.dropped_top)
    del fts, bases, bo
    torch.cuda.empty_cache()


def test_model_shape_at_low_density(eng):
    fts, bases, bo = make_inputs((8192, 8192), 3, seed=7, device=eng.device)
    rep = bc.check(eng, fts, bases, ALPHAS[:3], bo, density=0.2, gamma=0.01, lam=0.7, sign_election=True, label="8192^2 k=3, 0.2 / 0.01")
    assert all(kept >= rep.k_keep for kept in rep.kept) and all(1 <= d <= rep.n_top for d in rep.dropped_top)
    del fts, bases, bo
    torch.cuda.empty_cache()


def test_model_shape_with_own_bases(eng):
    fts, bases, bo = make_inputs((4096, 4096), 3, torch.bfloat16, torch.float32, seed=3, own_bases=True, device=eng.device)
    bc.check(eng, fts, bases, [0.5, -0.3, 0.4], bo, density=0.05, gamma=0.002, normalize=False, sign_election=False,
             label="4096^2, own bases, fp32 output")
    del fts, bases, bo
    torch.cuda.empty_cache()


@pytest.mark.parametrize("k,expected", [(2, {"crumbs_hist": 3, "crumbs_select": 3, "crumbs_merge": 1}),
                                        (5, {"crumbs_hist": 6, "crumbs_select": 3, "crumbs_merge": 1})], ids=["k2", "k5"])
def test_profile_names(eng, k, expected):
    bc.check_profile(eng, k, expected, shape=(1024, 1024), device=eng.device)


@pytest.mark.parametrize("operator", ["breadcrumbs", "breadcrumbs_ties"])
@pytest.mark.parametrize("inplace", [False, True], ids=["single_process", "inplace"])
def test_cli_on_the_device(tmp_path, eng, monkeypatch, inplace, operator):
    if inplace:
        monkeypatch.setenv("SHARDMERGE_INPLACE", "1")
    base, factors, full = lf.setup_k3(tmp_path, eng)
    opts = bc.options(operator)
    res = run_cli(bc.write_config(tmp_path, "org/lora", "merged", opts, device="cuda"))
    assert res.exit_code == 0, res.output
    assert_outputs(tmp_path / "merged", bc.expected_outputs(base, full, opts))
    assert "Breadcrumbs" in (tmp_path / "merged" / "README.md").read_text()
