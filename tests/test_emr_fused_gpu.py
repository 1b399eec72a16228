"""The fused EMR pass on the MI355X: the kernels of csrc/sm_emr_fused.hpp against the composition that defines them
(tests/emr_fused_checks.py) bit for bit - the grid and the corners of the emulator tier, five model-like shapes, two of
them against the emulator library as well - and `merge --emr-packs` once on the device."""
import pytest
import torch

from tests import emr_fused_checks as fc
from tests.harness import DTYPES, eng, make_inputs, raw  # noqa: F401

pytestmark = pytest.mark.gpu

# 300 x 4544: rows that are no multiple of the lanes' wrap; 16 x 28672 with k = 5: 14 octets per lane and two groups of
# tasks; 28672 x 8: many short rows, 448 blocks of the fold; the first and the second also run on the emulator
DEVICE_SHAPES = [((2048, 4096), 3, True), ((300, 4544), 2, True), ((16, 28672), 5, False), ((28672, 8), 2, False),
                 ((2048, 4096), 16, False)]


@pytest.mark.parametrize("cols", fc.COLS)
def test_cols(eng, cols):
    fc.check_cols(eng, cols, device=eng.device)


@pytest.mark.parametrize("rows", fc.ROWS)
def test_rows(eng, rows):
    fc.check_rows(eng, rows, device=eng.device)


@pytest.mark.parametrize("rows", fc.FOLD_EDGE_ROWS)
def test_fold_block_edge(eng, rows):
    fc.check_fold_rows(eng, rows, device=eng.device)


@pytest.mark.parametrize("lam", fc.LAMBDAS)
@pytest.mark.parametrize("own", [False, True], ids=["shared", "own"])
@pytest.mark.parametrize("k", fc.KS)
def test_k_bases_and_lambda(eng, k, own, lam):
    fc.check_k(eng, k, own, lam, device=eng.device)


@pytest.mark.parametrize("bo_dtype", DTYPES, ids=str)
@pytest.mark.parametrize("in_dtype", DTYPES, ids=str)
def test_dtypes(eng, in_dtype, bo_dtype):
    fc.check_dtypes(eng, in_dtype, bo_dtype, device=eng.device)


@pytest.mark.parametrize("check", fc.CORNERS, ids=lambda f: f.__name__[len("check_"):])
def test_corner(eng, check):
    check(eng, device=eng.device)


def test_profile_names_and_launches(eng):
    fc.check_profile(eng, device=eng.device)


def test_c_abi_rejects_bad_arguments(eng):
    fc.check_c_abi(eng, device=eng.device)


def test_geo_gram_fold_gives_the_same_bits(eng):
    fc.check_fold_hook(eng, device=eng.device)


@pytest.mark.parametrize("shape,k,on_emulator", DEVICE_SHAPES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_device_shape(eng, shape, k, on_emulator):
    """against the engine's own emr_merge + emr_mask on the device (the oracle's numpy walk of these sizes takes too long
    for the suite; the small grid holds both to it), and against the emulator library where stated"""
    fts, bases, bo = make_inputs(shape, k, seed=sum(shape) % 97 + k, device=eng.device)
    out, rep, masks, scales, mreps = eng.emr_merge_masks(fts, bases, bo)
    out2, rep2 = eng.emr_merge(fts, bases, bo)
    assert torch.equal(raw(out), raw(out2)) and rep == rep2
    for i in range(k):
        m2, s2, r2 = eng.emr_mask(fts[i], bases[i], out2)
        assert torch.equal(m2, masks[i]) and torch.equal(raw(s2), raw(scales[i])) and r2 == mreps[i], i
    assert [r.c for r in mreps] == rep.agree
    if on_emulator:
        from tests.emul.loader import emul_engine
        cpu = lambda ts: [t.cpu() for t in ts]
        eout, erep, emasks, escales, emreps = emul_engine().emr_merge_masks(cpu(fts), cpu(bases), bo.cpu())
        assert torch.equal(raw(eout), raw(out)) and erep == rep and emreps == mreps
        assert all(torch.equal(a, b.cpu()) for a, b in zip(emasks, masks))
        assert all(torch.equal(raw(a), raw(b)) for a, b in zip(escales, scales))


def test_merge_writes_the_packs_on_the_device(tmp_path, eng):
    fc.check_packs_end_to_end(tmp_path, eng, "cuda")
