"""Engine.lora_extract on the MI355X: the kernels of csrc/sm_extract.hpp - the delta product on v_mfma_f32_16x16x4_f32
above all - against tests/extract_oracle.py bit for bit (tests/extract_checks.py): the primitives on the emulator tier's
grid, the layout check on integers, the whole extraction, and two model-shaped cases (1024 x 4096, 300 x 4544: many
work-groups, several reduction segments) against the emulator library that build() produces - there the numpy chain
takes more than a few seconds - then quality, the round trip, the C ABI and the launch counts."""
import pytest
import torch

from tests import extract_checks as xc
from tests.harness import eng  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("L", xc.WIDTHS)
def test_fill(eng, L):
    for nrows in (1, 5, 257, 1124):
        xc.check_fill(eng, nrows, L)


@pytest.mark.parametrize("shape", xc.SHAPES + tuple((c, r) for r, c in xc.SHAPES if r != c), ids=lambda s: f"{s[0]}x{s[1]}")
def test_delta_mm_shapes(eng, shape):
    xc.check_delta_mm(eng, shape[0], shape[1], 32, torch.bfloat16)


@pytest.mark.parametrize("L", xc.WIDTHS)
def test_delta_mm_widths(eng, L):
    xc.check_delta_mm(eng, 17, 33, L, torch.bfloat16)
    xc.check_delta_mm(eng, 130, 257, L, torch.float32, seed=1)


@pytest.mark.parametrize("dtype", xc.DTYPES, ids=str)
def test_delta_mm_dtypes_views_and_special_values(eng, dtype):
    xc.check_delta_mm(eng, 130, 264, 16, dtype)
    xc.check_delta_mm(eng, 130, 264, 16, dtype, offset=1)
    xc.check_delta_mm(eng, 64, xc.S + 1, 32, dtype, offset=1, special=True)


def test_delta_mm_crossed_cases(eng):
    xc.check_delta_mm(eng, 64, xc.S + 1, 272, torch.float16, offset=1, special=True)
    xc.check_delta_mm(eng, 2 * xc.S + 100, 48, 80, torch.float32, offset=1)
    xc.check_delta_mm(eng, 3, 5, 272, torch.float16)
    xc.check_delta_mm(eng, 1, 1, 16, torch.float32, offset=1)


def test_delta_mm_nonfinite_propagates_and_fails(eng):
    xc.check_delta_mm_nonfinite(eng)


@pytest.mark.parametrize("shape", ((130, 257), (257, 130)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_layout_on_integers(eng, shape):
    xc.check_layout_integers(eng, *shape)
    xc.check_layout_integers(eng, *shape, dtype=torch.float32)


@pytest.mark.parametrize("m,L", [(m, L) for L in xc.WIDTHS for m in (1, 3, 255, 256, 257, 600)] + [(1124, 16), (1124, 32)])
def test_gram(eng, m, L):
    xc.check_gram(eng, m, L)


@pytest.mark.parametrize("out_dtype,trans", ((torch.float32, 0), (torch.bfloat16, 0), (torch.float16, 1), (torch.float32, 1)))
@pytest.mark.parametrize("L", xc.WIDTHS)
def test_panel_mm(eng, L, out_dtype, trans):
    xc.check_panel_mm(eng, 131, L, L if not trans else 24, out_dtype, trans)


@pytest.mark.parametrize("L,rank", ((16, 3), (32, 32), (80, 16)))
def test_sym_eig_of_the_hip_build(eng, L, rank):
    xc.check_sym_eig(eng, L, rank)


def test_sym_eig_272_of_the_hip_build_equals_the_emulator(eng):
    """the widest matrix: the hipcc build's solver against the g++ build's, bit for bit (numpy would take minutes)"""
    from shardmerge_amd import _lib
    from tests.emul.loader import emul_engine
    G = torch.from_numpy(xc.gram_matrix(272, 100, 9))
    e = eng.xl_probe(_lib.XL_SYM_EIG, rows=1, L=272, x=G)
    e2 = emul_engine().xl_probe(_lib.XL_SYM_EIG, rows=1, L=272, x=G)
    assert torch.equal(e.view(torch.int64), e2.view(torch.int64))


@pytest.mark.parametrize("q", xc.POWERS)
@pytest.mark.parametrize("rank", xc.RANKS)
@pytest.mark.parametrize("shape", xc.EXTRACT_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_extract_bit_for_bit(eng, shape, rank, q):
    for factor_dtype in (torch.bfloat16, torch.float32):
        xc.check_extract(eng, shape[0], shape[1], rank, q, factor_dtype)


@pytest.mark.parametrize("shape", ((1024, 4096), (300, 4544)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_model_shape_against_the_emulator(eng, shape):
    from tests.emul.loader import emul_engine
    xc.check_extract_against(eng, emul_engine(), shape[0], shape[1], 16)


def test_extract_of_a_merged_adapter_has_a_singular_gram(eng):
    rep = xc.check_extract(eng, 192, 320, 16, 1, torch.bfloat16, low_rank=4)
    assert rep.orth_ranks == [4, 4, 4] and rep.effective_rank == 4, rep


@pytest.mark.parametrize("rank", xc.RANKS)
@pytest.mark.parametrize("which", ("decay", "gauss", "lowrank+noise"))
def test_quality_against_the_svd_truncation(eng, which, rank):
    xc.check_quality(eng, which, rank)


@pytest.mark.parametrize("rank", (16, 32))
def test_exact_rank_16(eng, rank):
    rep, a, b, rel = xc.check_exact_rank(eng, rank)
    assert rep.effective_rank == 16
    assert not a[16:].any() and not b[:, 16:].any()
    assert rel <= 4e-6, rel


@pytest.mark.parametrize("rank", (8, 16))
def test_round_trip_through_lora_apply(eng, rank):
    xc.check_round_trip(eng, rank)


def test_c_abi_rejects_bad_arguments(eng):
    xc.check_c_abi(eng)


@pytest.mark.parametrize("q", (0, 2))
def test_profile_names_and_launches(eng, q):
    xc.check_profile(eng, q)


def test_command_writes_an_adapter_that_merge_takes(tmp_path, eng):
    xc.check_command(tmp_path, eng, "cuda")


def test_command_skips_a_changed_norm_and_clips_the_rank(tmp_path, eng):
    xc.check_command_variants(tmp_path, eng, "cuda")


def test_command_rejects_before_the_directory_exists(tmp_path, eng, monkeypatch):
    xc.check_command_rejections(tmp_path, eng, "cuda", monkeypatch)
