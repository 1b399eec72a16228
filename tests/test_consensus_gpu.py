"""operator: consensus_ta / consensus_ties on the MI355X: the kernel of csrc/sm_consensus.hpp (and the selection kernels of
TIES) against tests/consensus_oracle.py, bit for bit (tests/consensus_checks.py) - the parameter grid and the corners of
the emulator tier, the identities, model-shaped cases (the smallest at which the device path differs from the
emulator's: many work-groups, several octets per thread; none above 4096 x 4096, the CPU oracle takes seconds), and the
CLI on the device."""
import pytest
import torch

from tests import consensus_checks as cc
from tests import lora_fixtures as lf
from tests.harness import ALPHAS, DTYPES, assert_outputs, eng, make_inputs, run_cli  # noqa: F401

pytestmark = pytest.mark.gpu

# (shape, k, the flavours)
MODEL_SHAPES = [((1024, 4096), 3, cc.FLAVOURS), ((300, 4544), 3, cc.FLAVOURS), ((128, 11008), 5, cc.FLAVOURS), ((1, 4096), 3, cc.FLAVOURS),
                ((4096, 4096), 3, (True,))]     # (the selection's histograms need a tensor that spans many work-groups)


@pytest.mark.parametrize("ties", cc.FLAVOURS, ids=cc.FLAVOUR_IDS)
@pytest.mark.parametrize("bo_dtype", DTYPES, ids=str)
@pytest.mark.parametrize("in_dtype", DTYPES, ids=str)
def test_dtypes(eng, in_dtype, bo_dtype, ties):
    cc.check_dtypes(eng, in_dtype, bo_dtype, ties, device=eng.device)


@pytest.mark.parametrize("ties", cc.FLAVOURS, ids=cc.FLAVOUR_IDS)
@pytest.mark.parametrize("mask_lambda", cc.MASK_LAMBDAS)
@pytest.mark.parametrize("consensus_k", cc.CONSENSUS_KS)
@pytest.mark.parametrize("k", cc.KS)
def test_k_and_options(eng, k, consensus_k, mask_lambda, ties):
    cc.check_k_options(eng, k, consensus_k, mask_lambda, ties, device=eng.device)


@pytest.mark.parametrize("ties", cc.FLAVOURS, ids=cc.FLAVOUR_IDS)
@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("lam", [1.0, 0.7])
def test_lambda_and_normalize(eng, lam, normalize, ties):
    cc.check_lambda_normalize(eng, lam, normalize, ties, device=eng.device)


@pytest.mark.parametrize("ties", cc.FLAVOURS, ids=cc.FLAVOUR_IDS)
@pytest.mark.parametrize("n", cc.SIZES)
def test_sizes(eng, n, ties):
    cc.check_size(eng, n, ties, device=eng.device)


@pytest.mark.parametrize("check", cc.CORNERS, ids=lambda f: f.__name__[len("check_"):])
def test_corner(eng, check):
    check(eng, device=eng.device)


@pytest.mark.parametrize("shape,k,flavours", MODEL_SHAPES, ids=["x".join(map(str, s)) + f"-k{k}" for s, k, _ in MODEL_SHAPES])
def test_model_shape(eng, shape, k, flavours):
    fts, bases, bo = make_inputs(shape, k, seed=sum(shape) % 97, device=eng.device)
    for ties in flavours:
        rep, _, _ = cc.check(eng, fts, bases, ALPHAS[:k], bo, ties=ties, lam=0.7, label=f"{shape} k={k} {cc.name_of(ties)}")
        assert 0 < rep.selected < rep.n
    del fts, bases, bo
    torch.cuda.empty_cache()


@pytest.mark.parametrize("ties", cc.FLAVOURS, ids=cc.FLAVOUR_IDS)
def test_model_shape_k16_with_own_bases(eng, ties):
    """the 128-register variant over many work-groups, with the plain sum and with the TIES election"""
    fts, bases, bo = make_inputs((2048, 4096), 16, torch.bfloat16, torch.float32, seed=3, own_bases=True, device=eng.device)
    alphas = [a if i % 3 else -a for i, a in enumerate(ALPHAS)]
    cc.check(eng, fts, bases, alphas, bo, ties=ties, consensus_k=4, normalize=not ties,
             label=f"2048 x 4096 k=16, own bases, fp32 output, {cc.name_of(ties)}")
    del fts, bases, bo
    torch.cuda.empty_cache()


@pytest.mark.parametrize("ties,k,expected", cc.PROFILES, ids=cc.PROFILE_IDS)
def test_profile_names(eng, ties, k, expected):
    cc.check_profile(eng, ties, k, expected, shape=(1024, 1024), device=eng.device)


def test_c_abi_rejects_bad_arguments(eng):
    cc.check_c_abi(eng, device=eng.device)


@pytest.mark.parametrize("operator", ["consensus_ta", "consensus_ties"])
@pytest.mark.parametrize("inplace", [False, True], ids=["single_process", "inplace"])
def test_cli_on_the_device(tmp_path, eng, monkeypatch, inplace, operator):
    if inplace:
        monkeypatch.setenv("SHARDMERGE_INPLACE", "1")
    base, factors, full = lf.setup_k3(tmp_path, eng)
    opts = cc.options(operator)
    res = run_cli(cc.write_config(tmp_path, "org/lora", "merged", opts, device="cuda"))
    assert res.exit_code == 0, res.output
    assert_outputs(tmp_path / "merged", cc.expected_outputs(base, full, opts))
    assert "Consensus" in (tmp_path / "merged" / "README.md").read_text()
