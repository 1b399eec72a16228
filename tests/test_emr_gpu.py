"""EMR-Merging on the MI355X: the kernels of csrc/sm_emr.hpp against tests/emr_oracle.py bit for bit, the identities and the
paper's form in torch fp64 (tests/emr_checks.py) - the grid and the corners of the emulator tier, three model-like shapes,
two of them against the emulator library as well - and the merge, the command and the pack once on the device."""
import pytest
import torch

from tests import emr_checks as ec
from tests.harness import DTYPES, KS, eng, make_inputs, raw  # noqa: F401

pytestmark = pytest.mark.gpu

# 300 x 4544: rows that are no multiple of the lanes' wrap; 16 x 28672: 14 octets per lane; the first and the third also
# run on the emulator
DEVICE_SHAPES = [((2048, 4096), 3, True), ((2048, 4096), 16, False), ((300, 4544), 2, True), ((16, 28672), 2, False)]


@pytest.mark.parametrize("lam", ec.LAMBDAS)
@pytest.mark.parametrize("own", [False, True], ids=["shared", "own"])
@pytest.mark.parametrize("k", KS)
def test_k_bases_and_lambda(eng, k, own, lam):
    ec.check_k(eng, k, own, lam, device=eng.device)


@pytest.mark.parametrize("n", ec.SIZES)
def test_sizes(eng, n):
    ec.check_size(eng, n, device=eng.device)


@pytest.mark.parametrize("bo_dtype", DTYPES, ids=str)
@pytest.mark.parametrize("in_dtype", DTYPES, ids=str)
def test_dtypes(eng, in_dtype, bo_dtype):
    ec.check_dtypes(eng, in_dtype, bo_dtype, device=eng.device)


@pytest.mark.parametrize("check", ec.MERGE_CORNERS, ids=lambda f: f.__name__[len("check_"):])
def test_merge_corner(eng, check):
    check(eng, device=eng.device)


@pytest.mark.parametrize("cols", ec.COLS)
def test_mask_cols(eng, cols):
    ec.check_cols(eng, cols, device=eng.device)


@pytest.mark.parametrize("rows", ec.ROWS)
def test_mask_rows(eng, rows):
    ec.check_rows(eng, rows, device=eng.device)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_mask_dtypes(eng, dtype):
    ec.check_mask_dtypes(eng, dtype, device=eng.device)


@pytest.mark.parametrize("check", ec.MASK_CORNERS, ids=lambda f: f.__name__[len("check_"):])
def test_mask_corner(eng, check):
    check(eng, device=eng.device)


def test_profile_names_and_launches(eng):
    ec.check_profile(eng, device=eng.device)


def test_c_abi_rejects_bad_arguments(eng):
    ec.check_c_abi(eng, device=eng.device)


@pytest.mark.parametrize("k", [2, 3, 5])
def test_the_papers_form_in_fp64(eng, k):
    ec.check_paper_form(eng, k, device=eng.device)


@pytest.mark.parametrize("shape,k,on_emulator", DEVICE_SHAPES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_device_shape(eng, shape, k, on_emulator):
    fts, bases, bo = make_inputs(shape, k, seed=sum(shape) % 97 + k, device=eng.device)
    rep, out, delta, _ = ec.check(eng, fts, bases, bo, label=f"{shape} k={k}")
    mask, scale, mrep, applied = ec.check_mask(eng, fts[k - 1], bo, out, label=f"{shape} k={k} mask")
    assert mrep.c == rep.agree[k - 1]
    if on_emulator:
        from tests.emul.loader import emul_engine
        em = emul_engine()
        cpu = lambda ts: [t.cpu() for t in ts]
        eout, erep, edelta = em.emr_merge(cpu(fts), cpu(bases), bo.cpu(), want_delta=True)
        assert torch.equal(raw(eout), raw(out)) and torch.equal(raw(edelta), raw(delta)) and erep == rep
        emask, escale, emrep = em.emr_mask(fts[k - 1].cpu(), bo.cpu(), eout)
        assert torch.equal(emask, mask.cpu()) and torch.equal(raw(escale), raw(scale)) and emrep == mrep
        assert torch.equal(raw(em.emr_apply(bo.cpu(), eout, emask, escale)), raw(applied))


def test_merge_task_and_pack_on_the_device(tmp_path, eng):
    ec.check_end_to_end(tmp_path, eng, "cuda")
