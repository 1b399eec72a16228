"""operator: iso_c on the MI355X: `iso_gemm` of csrc/sm_iso.hpp on v_mfma_f32_32x32x2_f32 and the small kernels against
tests/iso_oracle.py bit for bit (tests/iso_checks.py) - the probe's grid, the layout check on integers, the whole function,
two model-shaped cases (384 x 2048: three tiles along m and n, 64 k-blocks; 300 x 4544: unaligned edges) against the
emulator library that build() produces - there the numpy chain takes more than a few seconds - then what defines Iso-C
against torch fp64, the properties, the C ABI, the launch counts and the CLI on the device."""
import pytest
import torch

from tests import iso_checks as ic
from tests import iso_oracle as io
from tests.harness import eng  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("K", ic.GEMM_K)
def test_gemm_shapes(eng, K):
    for M, N in ic.GEMM_MN:
        for form in (io.NT, io.NN):
            ic.check_gemm(eng, form, M, N, K)


@pytest.mark.parametrize("ep", (io.POLY, io.AXPY, io.CUBIC))
@pytest.mark.parametrize("form", (io.NT, io.NN))
def test_gemm_epilogues(eng, form, ep):
    for M, N, K in ((17, 15, 5), (129, 257, 33), (128, 128, 32)):
        ic.check_gemm(eng, form, M, N, K, ep)


@pytest.mark.parametrize("form", (io.NT, io.NN))
def test_gemm_views_and_special_values(eng, form):
    ic.check_gemm(eng, form, 129, 130, 33, io.CUBIC, offset=1)
    ic.check_gemm(eng, form, 130, 129, 35, io.POLY, offset=1, pad=3)
    ic.check_gemm(eng, form, 33, 130, 64, io.AXPY, pad=4)
    ic.check_gemm(eng, form, 65, 47, 37, io.PLAIN, special=True)
    ic.check_gemm(eng, form, 17, 33, 9, io.POLY, offset=1, special=True)
    for poke in (float("nan"), float("inf"), float("-inf")):
        ic.check_gemm(eng, form, 33, 17, 35, io.AXPY, poke=poke)


@pytest.mark.parametrize("s,K", ic.GEMM_SYM)
def test_gemm_symmetric_mode(eng, s, K):
    ic.check_gemm_sym(eng, s, K, gram=True)
    ic.check_gemm_sym(eng, s, K, gram=False)


def test_gemm_layout_on_integers(eng):
    for form in (io.NT, io.NN):
        for M, N, K in ((17, 33, 5), (130, 257, 33), (257, 130, 64)):
            ic.check_gemm_integers(eng, form, M, N, K)


@pytest.mark.parametrize("shape", ic.MERGE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_merge_equals_the_oracle(eng, shape):
    rep = ic.check_merge(eng, shape, 2)
    assert rep.converged and rep.transposed == (shape[0] > shape[1])


@pytest.mark.parametrize("k,own", ic.MERGE_KS, ids=ic.MERGE_K_IDS)
@pytest.mark.parametrize("shape", ((17, 33), (33, 17)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_merge_k_and_bases(eng, shape, k, own):
    ic.check_merge(eng, shape, k, own)


@pytest.mark.parametrize("bo_dtype", ic.DTYPES, ids=str)
@pytest.mark.parametrize("in_dtype", ic.DTYPES, ids=str)
def test_merge_dtype_pairs(eng, in_dtype, bo_dtype):
    ic.check_merge(eng, (33, 17), 2, in_dtype=in_dtype, bo_dtype=bo_dtype)


def test_merge_corner_cases(eng):
    ic.check_merge(eng, (130, 257), 3, True)
    ic.check_rank3(eng)
    for shape in ((17, 33), (130, 40)):
        rep = ic.check_merge(eng, shape, 2, variant="zero")
        assert rep.zero and rep.e == []
    ic.check_nonfinite(eng)
    rep = ic.check_merge(eng, (33, 17), 3, max_iter=0)
    assert rep.iterations == 0 and len(rep.e) == 1 and not rep.converged
    rep = ic.check_merge(eng, (130, 257), 2, max_iter=2)
    assert rep.steps == "qq" and not rep.converged
    ic.check_merge(eng, (17, 33), 3, variant="signs")
    ic.check_merge(eng, (33, 17), 5, True, variant="signs")


@pytest.mark.parametrize("rows,cols,max_iter", [(384, 2048, 4), (300, 4544, 3)], ids=["384x2048", "300x4544"])
def test_model_shape_against_the_emulator(eng, rows, cols, max_iter):
    from tests.emul.loader import emul_engine
    fts, bases, base_out = ic.merge_inputs((rows, cols), 2, seed=1)
    kw = dict(lam=0.7, max_iter=max_iter, want_delta=True)
    on = lambda t: t.to(eng.device)
    out, rep, delta = eng.iso_merge([on(t) for t in fts], [on(bases[0])] * 2, [1.0, 0.7], on(base_out), **kw)
    out2, rep2, delta2 = emul_engine().iso_merge(fts, [bases[0]] * 2, [1.0, 0.7], base_out, **kw)
    print(f"{rows}x{cols}: steps {rep.steps}, e {rep.e}")
    assert torch.equal(ic.raw(out), ic.raw(out2)) and torch.equal(ic.raw(delta), ic.raw(delta2))
    assert rep == rep2 and rep.iterations == max_iter
    torch.cuda.empty_cache()


@pytest.mark.parametrize("shape,k", ic.SVD_CASES, ids=lambda v: str(v))
def test_merged_delta_is_the_isotropic_one(eng, shape, k):
    """see tests/test_iso_host.py: the tolerances are 4 x what the numpy restatement deviates by, measured on the CPU"""
    ic.check_against_svd(eng, shape, k)


def test_properties(eng):
    ic.check_transpose(eng)
    ic.check_doubled_alphas(eng)
    ic.check_swapped_entries(eng)
    ic.check_partial_permutation(eng)


@pytest.mark.parametrize("shape", [(2048, 2048), (1024, 4096)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_large_matrices_converge(eng, shape):
    """converged, and the residual recomputed in torch fp64 from delta_out / sigma_bar is within iso_tol + 4 x the gap
    |e_fp64 - e_engine| that the numpy restatement shows on the CPU at 256 x 1024 (iso_checks.E_GAP)"""
    ic.check_large_residual(eng, shape)
    torch.cuda.empty_cache()


def test_profile_names_and_launches(eng):
    ic.check_profile(eng, (96, 160), 2)
    ic.check_profile(eng, (160, 96), 3, max_iter=1)
    ic.check_profile(eng, (160, 96), 2, zero=True)


def test_c_abi_rejects_bad_arguments(eng):
    ic.check_c_abi(eng)


@pytest.mark.parametrize("inplace", [False, True], ids=["single_process", "inplace"])
def test_cli_on_the_device(tmp_path, eng, monkeypatch, inplace):
    if inplace:
        monkeypatch.setenv("SHARDMERGE_INPLACE", "1")
    ic.check_cli(tmp_path, eng, device="cuda", third="org/lora")
