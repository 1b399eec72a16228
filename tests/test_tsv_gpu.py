"""operator: tsv on the MI355X: `tsv_apply` of csrc/sm_tsv.hpp on v_mfma_f32_16x16x4_f32 and the extraction kernels it
runs on against tests/tsv_oracle.py bit for bit (tests/tsv_checks.py) - the probe's grid, the layout check on integers, the
whole function, two model-shaped cases (1024 x 4096 with R = 192, 300 x 4544: many work-groups, panels wider than one
chunk) against the emulator library that build() produces - there the numpy chain takes more than a few seconds - then
the properties that define TSV, the C ABI, the launch counts and the CLI on the device."""
import pytest
import torch

from tests import lora_fixtures as lf
from tests import tsv_checks as tc
from tests.harness import eng  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("Rp", tc.APPLY_WIDTHS)
@pytest.mark.parametrize("shape", tc.APPLY_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_apply_shapes_and_widths(eng, shape, Rp):
    for dtype in tc.DTYPES:
        tc.check_apply(eng, shape[0], shape[1], Rp, dtype)


@pytest.mark.parametrize("dtype", tc.DTYPES, ids=str)
def test_apply_views_and_special_values(eng, dtype):
    tc.check_apply(eng, 130, 257, 32, dtype, offset=1)
    tc.check_apply(eng, 17, 33, 80, dtype, offset=1, special=True)
    tc.check_apply(eng, 257, 130, 16, dtype, special=True, lam=-1.5)


def test_apply_layout_on_integers(eng):
    for rows, cols, Rp in ((17, 33, 16), (130, 257, 48), (257, 130, 256)):
        tc.check_apply_integers(eng, rows, cols, Rp)
    tc.check_apply_empty_panel(eng)


@pytest.mark.parametrize("k,own", tc.MERGE_KS, ids=tc.MERGE_K_IDS)
@pytest.mark.parametrize("shape", tc.MERGE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_merge_equals_the_oracle(eng, shape, k, own):
    rep = tc.check_merge(eng, shape[0], shape[1], k, 16, 2, own)
    assert rep.R == 16 * k


@pytest.mark.parametrize("q", (0, 1))
@pytest.mark.parametrize("shape", tc.MERGE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_merge_rank_8(eng, shape, q):
    tc.check_merge(eng, shape[0], shape[1], 3, 8, q)


@pytest.mark.parametrize("base_out_dtype", (torch.float16, torch.float32), ids=str)
def test_merge_base_out_dtypes(eng, base_out_dtype):
    tc.check_merge(eng, 192, 320, 2, 8, 1, base_out_dtype=base_out_dtype)


def test_merge_corner_cases(eng):
    rep = tc.check_merge(eng, 192, 320, 3, 16, 1, variant="zero_alpha")
    assert rep.rho == [16, 0, 16] and rep.R == 32
    rep = tc.check_merge(eng, 192, 320, 3, 16, 1, variant="identical")
    assert rep.R == 48 and rep.kept_U == rep.kept_W == 32
    rep = tc.check_merge(eng, 320, 192, 2, 16, 1, variant="equal_base")
    assert rep.rho == [16, 0] and rep.Rp == 16
    tc.check_nonfinite(eng)
    tc.check_rank3(eng)


@pytest.mark.parametrize("rows,cols,k,r", [(1024, 4096, 3, 64), (300, 4544, 2, 64)], ids=["1024x4096-k3-r64", "300x4544-k2-r64"])
def test_model_shape_against_the_emulator(eng, rows, cols, k, r):
    from tests.emul.loader import emul_engine
    tc.check_merge_against(eng, emul_engine(), rows, cols, k, r)
    torch.cuda.empty_cache()


@pytest.mark.parametrize("k", (2, 3, 5))
def test_singular_values_are_the_weighted_sigmas(eng, k):
    """see tests/test_tsv_host.py: the tolerances are 4 x what the numpy restatement deviates by, measured on the CPU"""
    tc.check_singular_values(eng, k)


def test_duplicates_and_disjoint_supports(eng):
    tc.check_duplicates(eng)
    tc.check_disjoint_supports(eng)


@pytest.mark.parametrize("rank", tc.xc.RANKS)
@pytest.mark.parametrize("which", ("decay", "gauss", "lowrank+noise"))
def test_k1_is_the_truncation(eng, which, rank):
    tc.check_truncation(eng, which, rank)


@pytest.mark.parametrize("k,q", [(1, 0), (3, 2)])
def test_profile_names_and_launches(eng, k, q):
    tc.check_profile(eng, k, q)


def test_c_abi_rejects_bad_arguments(eng):
    tc.check_c_abi(eng)


@pytest.mark.parametrize("inplace", [False, True], ids=["single_process", "inplace"])
def test_cli_on_the_device(tmp_path, eng, monkeypatch, inplace):
    if inplace:
        monkeypatch.setenv("SHARDMERGE_INPLACE", "1")
    tc.check_cli(tmp_path, eng, device="cuda", third="org/lora")
