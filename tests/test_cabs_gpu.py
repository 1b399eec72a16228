"""operator: cabs on the MI355X: the kernel of csrc/sm_cabs.hpp against tests/cabs_oracle.py, bit for bit
(tests/cabs_checks.py) - the row lengths, the option grid and the corners of the emulator tier, the identities, the
paper's form in torch, model-shaped cases (many work-groups, several tiles per work-group; none above 2048 x 4096, the
CPU oracle takes seconds), two of them against the emulator too, and the CLI on the device."""
import pytest
import torch

from tests import cabs_checks as cc
from tests import lora_fixtures as lf
from tests.harness import ALPHAS, DTYPES, assert_outputs, eng, make_inputs, raw, run_cli  # noqa: F401

pytestmark = pytest.mark.gpu

TAIL_COLS = 4544                                # the option grid's row length on the device: 8 full groups of 512 and 448
# (shape, k, N, M, own bases, also against the emulator)
MODEL_SHAPES = [((1024, 4096), 3, 16, 64, False, True), ((300, 4544), 3, 128, 512, False, True), ((1030, 257), 5, 16, 64, True, False)]


@pytest.mark.parametrize("C", cc.COLS)
def test_cols(eng, C):
    cc.check_cols(eng, C, device=eng.device)


@pytest.mark.parametrize("conflict_aware", [True, False], ids=["ca", "independent"])
@pytest.mark.parametrize("M", cc.GROUPS)
def test_options(eng, M, conflict_aware):
    cc.check_options(eng, M, conflict_aware, TAIL_COLS, device=eng.device)


@pytest.mark.parametrize("own", [False, True], ids=["shared_base", "own_bases"])
@pytest.mark.parametrize("k", cc.KS)
def test_k(eng, k, own):
    cc.check_k(eng, k, own, device=eng.device)


@pytest.mark.parametrize("bo_dtype", DTYPES, ids=str)
@pytest.mark.parametrize("in_dtype", DTYPES, ids=str)
def test_dtypes(eng, in_dtype, bo_dtype):
    cc.check_dtypes(eng, in_dtype, bo_dtype, device=eng.device)


@pytest.mark.parametrize("check", cc.CORNERS, ids=lambda f: f.__name__[len("check_"):])
def test_corner(eng, check):
    check(eng, device=eng.device)


def test_tied_bf16_at_the_measured_shape(eng):
    """(512, 1024), k = 2, 64:256 in bf16: about four groups in ten keep more than their quota"""
    cc.check_tied(eng, (512, 1024), device=eng.device)


@pytest.mark.parametrize("shape,k,N,M,own,emulated", MODEL_SHAPES, ids=["x".join(map(str, c[0])) + f"-k{c[1]}" for c in MODEL_SHAPES])
def test_model_shape(eng, shape, k, N, M, own, emulated):
    fts, bases, bo = make_inputs(shape, k, seed=sum(shape) % 97, own_bases=own, device=eng.device)
    rep, out, delta = cc.check(eng, fts, bases, ALPHAS[:k], bo, N, M, lam=0.7, label=f"{shape} k={k} {N}:{M}")
    assert 0 < rep.covered < rep.n
    if emulated:
        from tests.emul.loader import emul_engine
        cpu = lambda ts: [t.cpu() for t in ts]
        e_out, e_rep, e_delta = emul_engine().cabs_merge(cpu(fts), cpu(bases), ALPHAS[:k], bo.cpu(), n_keep=N, group=M, lam=0.7,
                                                         want_delta=True, want_mask=True)
        assert torch.equal(raw(out), raw(e_out)) and torch.equal(raw(delta), raw(e_delta)) and torch.equal(rep.mask.cpu(), e_rep.mask)
        e_rep.mask = rep.mask = None
        assert rep == e_rep
    del fts, bases, bo
    torch.cuda.empty_cache()


def test_model_shape_k16_with_own_bases(eng):
    """the 128-register variant over many work-groups: the later finetunes find the groups used up"""
    fts, bases, bo = make_inputs((2048, 4096), 16, torch.bfloat16, torch.float32, seed=3, own_bases=True, device=eng.device)
    alphas = [a if i % 3 else -a for i, a in enumerate(ALPHAS)]
    rep, _, _ = cc.check(eng, fts, bases, alphas, bo, 16, 256, label="2048 x 4096 k=16, own bases, fp32 output")
    assert rep.short_groups[0] == 0 and rep.kept[15] > 0
    del fts, bases, bo
    torch.cuda.empty_cache()


@pytest.mark.parametrize("shape,k,N,M", cc.PAPER_CASES, ids=["x".join(map(str, c[0])) + f"-k{c[1]}-{c[2]}of{c[3]}" for c in cc.PAPER_CASES])
def test_paper_form_in_torch(eng, shape, k, N, M):
    """Measured on the CPU with this construction: 0 of 4096, 0 of 8100 and 1 of 196608 groups have a cut value that is not
    unique; the cap is 0.1 %."""
    cc.check_paper_form(eng, shape, k, N, M, device=eng.device)


@pytest.mark.parametrize("k,expected", cc.PROFILES, ids=[f"k{k}" for k, _ in cc.PROFILES])
def test_profile_names(eng, k, expected):
    cc.check_profile(eng, k, expected, device=eng.device)


def test_c_abi_rejects_bad_arguments(eng):
    cc.check_c_abi(eng, device=eng.device)


@pytest.mark.parametrize("inplace", [False, True], ids=["single_process", "inplace"])
def test_cli_on_the_device(tmp_path, eng, monkeypatch, inplace):
    if inplace:
        monkeypatch.setenv("SHARDMERGE_INPLACE", "1")
    base, factors, full = lf.setup_k3(tmp_path, eng)
    res = run_cli(cc.write_config(tmp_path, "org/lora", "merged", cc.OPTIONS, device="cuda"))
    assert res.exit_code == 0, res.output
    assert_outputs(tmp_path / "merged", cc.expected_outputs(base, full, cc.OPTIONS))
    readme = (tmp_path / "merged" / "README.md").read_text()
    assert "CABS" in readme and "8:32" in readme and "entry order: org/ft1 > org/ft2 > org/lora" in readme
