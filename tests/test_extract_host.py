"""extract-lora / Engine.lora_extract without a GPU: the kernels of csrc/sm_extract.hpp on the CPU work-group emulator
against tests/extract_oracle.py bit for bit (tests/extract_checks.py), the oracle's own exact fma, the layout check on
integers, the quality checks against torch.linalg.svd, the round trip through lora_apply, the C ABI and the launch
counts."""
import numpy as np
import pytest
import torch

from tests import extract_checks as xc
from tests import extract_oracle as xo
from tests.harness import emul  # noqa: F401


# ---- the oracle's own tools ------------------------------------------------------------------------------------
def test_oracle_fma_is_exact():
    """a self-check of the test infrastructure (it runs no code of the library): the oracle's fp32 fma against exact
    rational arithmetic, on the known double-rounding cases and on random operands"""
    xo.fma32_selfcheck()
    g = np.random.default_rng(0)
    a, b, c = (g.standard_normal(20000).astype(np.float32) for _ in range(3))
    c *= np.float32(1e-3)
    got = xo.fma32(a, b, c)
    # exact reference in integers: every fp32 is m * 2^e
    from fractions import Fraction
    naive = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    for i in np.nonzero(got != naive)[0][:50].tolist() + list(range(200)):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo = np.float32(float(exact))
        cand = [np.nextafter(lo, np.float32(-np.inf)), lo, np.nextafter(lo, np.float32(np.inf))]
        best = min(cand, key=lambda v: (abs(Fraction(float(v)) - exact), int(v.view(np.uint32)) & 1))
        assert got[i] == best, (i, a[i], b[i], c[i], got[i], best)


# ---- 1. the primitives -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", xc.WIDTHS)
@pytest.mark.parametrize("nrows", (1, 5, 257, 1124))
def test_fill(emul, nrows, L):
    xc.check_fill(emul, nrows, L)


@pytest.mark.parametrize("shape", xc.SHAPES + tuple((c, r) for r, c in xc.SHAPES if r != c), ids=lambda s: f"{s[0]}x{s[1]}")
def test_delta_mm_shapes(emul, shape):
    xc.check_delta_mm(emul, shape[0], shape[1], 32, torch.bfloat16)


@pytest.mark.parametrize("L", xc.WIDTHS)
def test_delta_mm_widths(emul, L):
    xc.check_delta_mm(emul, 17, 33, L, torch.bfloat16)
    xc.check_delta_mm(emul, 130, 257, L, torch.float32, seed=1)


@pytest.mark.parametrize("dtype", xc.DTYPES, ids=str)
def test_delta_mm_dtypes_views_and_special_values(emul, dtype):
    xc.check_delta_mm(emul, 130, 264, 16, dtype)                    # 16-byte loads
    xc.check_delta_mm(emul, 130, 264, 16, dtype, offset=1)          # the same, one element off: no 16-byte loads
    xc.check_delta_mm(emul, 64, xc.S + 1, 32, dtype, offset=1, special=True)


def test_delta_mm_crossed_cases(emul):
    """the widest panel across a segment edge, fp16, an unaligned view; every shape's edge at a second width and dtype"""
    xc.check_delta_mm(emul, 64, xc.S + 1, 272, torch.float16, offset=1, special=True)
    xc.check_delta_mm(emul, 2 * xc.S + 100, 48, 80, torch.float32, offset=1)
    xc.check_delta_mm(emul, 3, 5, 272, torch.float16)
    xc.check_delta_mm(emul, 1, 1, 16, torch.float32, offset=1)


def test_delta_mm_nonfinite_propagates_and_fails(emul):
    xc.check_delta_mm_nonfinite(emul)


@pytest.mark.parametrize("shape", ((130, 257), (257, 130)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_layout_on_integers(emul, shape):
    xc.check_layout_integers(emul, *shape)
    xc.check_layout_integers(emul, *shape, dtype=torch.float32)


# (several segments at every width; 1124 rows at the narrow widths, where the numpy Gram is quick)
@pytest.mark.parametrize("m,L", [(m, L) for L in xc.WIDTHS for m in (1, 3, 255, 256, 257, 600)] + [(1124, 16), (1124, 32)])
def test_gram(emul, m, L):
    xc.check_gram(emul, m, L)


@pytest.mark.parametrize("out_dtype,trans", ((torch.float32, 0), (torch.bfloat16, 0), (torch.float16, 1), (torch.float32, 1)))
@pytest.mark.parametrize("L", xc.WIDTHS)
def test_panel_mm(emul, L, out_dtype, trans):
    xc.check_panel_mm(emul, 131, L, L if not trans else 24, out_dtype, trans)


@pytest.mark.parametrize("L,rank", ((16, 16), (16, 3), (32, 32), (32, 8), (80, 80), (80, 16)))
def test_sym_eig(emul, L, rank):
    xc.check_sym_eig(emul, L, rank)


def test_sym_eig_272_against_lapack(emul):
    """the widest matrix: the numpy restatement would take minutes, LAPACK is the reference here"""
    from shardmerge_amd import _lib
    G = xc.gram_matrix(272, 100, 9)
    e = emul.xl_probe(_lib.XL_SYM_EIG, rows=1, L=272, x=torch.from_numpy(G)).numpy()
    lam, V = e[:272], e[272:].reshape(272, 272)
    ref = np.linalg.eigvalsh(G)[::-1]
    assert np.abs(lam - ref).max() <= 1e-13 * ref[0] * 272
    assert np.abs(V.T @ V - np.eye(272)).max() < 1e-12
    assert np.abs(G @ V - V * lam).max() <= 1e-12 * ref[0]


# ---- 3. the whole extraction -------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", xc.POWERS)
@pytest.mark.parametrize("rank", xc.RANKS)
@pytest.mark.parametrize("shape", xc.EXTRACT_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_extract_bit_for_bit(emul, shape, rank, q):
    for factor_dtype in (torch.bfloat16, torch.float32):
        xc.check_extract(emul, shape[0], shape[1], rank, q, factor_dtype)


def test_extract_of_a_merged_adapter_has_a_singular_gram(emul):
    """a finetune that is a merged rank-4 adapter, extracted at r = 16: every orth truncates"""
    rep = xc.check_extract(emul, 192, 320, 16, 1, torch.bfloat16, low_rank=4)
    assert rep.orth_ranks == [4, 4, 4] and rep.effective_rank == 4, rep


def test_extract_clips_the_rank_of_a_narrow_tensor(emul):
    ft, base = xc.pair(5, 40, torch.float32, 3)
    a, b, rep = emul.lora_extract(ft, base, 16, factor_dtype=torch.float32)
    assert rep.width == 16 and rep.effective_rank <= 5 and not a[rep.effective_rank:].any() and not b[:, rep.effective_rank:].any()
    D = (ft - base).double()
    assert float(torch.linalg.norm(D - b.double() @ a.double()) / torch.linalg.norm(D)) < 1e-5
    same = emul.lora_extract(ft, ft.clone(), 4)                      # a zero delta: zero factors, rank 0
    assert same[2].effective_rank == 0 and same[2].share == 0.0 and not same[0].any() and not same[1].any()


# ---- 4. quality ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rank", xc.RANKS)
@pytest.mark.parametrize("which", ("decay", "gauss", "lowrank+noise"))
def test_quality_against_the_svd_truncation(emul, which, rank):
    xc.check_quality(emul, which, rank)


@pytest.mark.parametrize("rank", (16, 32))
def test_exact_rank_16(emul, rank):
    rep, a, b, rel = xc.check_exact_rank(emul, rank)
    assert rep.effective_rank == 16
    assert not a[16:].any() and not b[:, 16:].any()
    assert rel <= 4e-6, rel


# ---- 5. the round trip -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rank", (8, 16))
def test_round_trip_through_lora_apply(emul, rank):
    xc.check_round_trip(emul, rank)


# ---- 7. the C ABI ----------------------------------------------------------------------------------------------------
def test_c_abi_rejects_bad_arguments(emul):
    xc.check_c_abi(emul)


@pytest.mark.parametrize("q", (0, 2, 4))
def test_profile_names_and_launches(emul, q):
    xc.check_profile(emul, q)


# ---- 6. the command, with the emulator as the device -------------------------------------------------------------------
def test_command_writes_an_adapter_that_merge_takes(tmp_path, emul):
    xc.check_command(tmp_path, emul, "cpu")


def test_command_skips_a_changed_norm_and_clips_the_rank(tmp_path, emul):
    xc.check_command_variants(tmp_path, emul, "cpu")


def test_command_rejects_before_the_directory_exists(tmp_path, emul, monkeypatch):
    xc.check_command_rejections(tmp_path, emul, "cpu", monkeypatch)
