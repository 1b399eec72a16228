"""The fused EMR pass and `merge --emr-packs` without a GPU: the kernels of csrc/sm_emr_fused.hpp on the CPU work-group
emulator against the composition that defines them (tests/emr_fused_checks.py: the oracle's and the engine's own
emr_merge + emr_mask, bit for bit), the identities, the launches, the C ABI, and the packs a merge writes against the
packs `emr-task` writes afterwards, with the emulator as the device."""
import pytest

from tests import emr_fused_checks as fc
from tests.harness import DTYPES, emul  # noqa: F401


@pytest.mark.parametrize("cols", fc.COLS)
def test_cols(emul, cols):
    fc.check_cols(emul, cols)


@pytest.mark.parametrize("rows", fc.ROWS)
def test_rows(emul, rows):
    fc.check_rows(emul, rows)


@pytest.mark.parametrize("rows", fc.FOLD_EDGE_ROWS)
def test_fold_block_edge(emul, rows):
    fc.check_fold_rows(emul, rows)


@pytest.mark.parametrize("lam", fc.LAMBDAS)
@pytest.mark.parametrize("own", [False, True], ids=["shared", "own"])
@pytest.mark.parametrize("k", fc.KS)
def test_k_bases_and_lambda(emul, k, own, lam):
    fc.check_k(emul, k, own, lam)


@pytest.mark.parametrize("bo_dtype", DTYPES, ids=str)
@pytest.mark.parametrize("in_dtype", DTYPES, ids=str)
def test_dtypes(emul, in_dtype, bo_dtype):
    fc.check_dtypes(emul, in_dtype, bo_dtype)


@pytest.mark.parametrize("check", fc.CORNERS, ids=lambda f: f.__name__[len("check_"):])
def test_corner(emul, check):
    check(emul)


def test_profile_names_and_launches(emul):
    fc.check_profile(emul)


def test_c_abi_rejects_bad_arguments(emul):
    fc.check_c_abi(emul)


def test_geo_gram_fold_gives_the_same_bits(emul):
    fc.check_fold_hook(emul)


# ---- the merge writes the packs ---------------------------------------------------------------------------------------------
def test_merge_writes_what_emr_task_writes(tmp_path, emul):
    fc.check_packs_end_to_end(tmp_path, emul, "cpu")


def test_packs_scale_per_tensor_and_full(tmp_path, emul):
    fc.check_pack_forms(tmp_path, emul, "cpu")


def test_pack_rejections(tmp_path, emul, monkeypatch):
    fc.check_pack_rejections(tmp_path, emul, "cpu", monkeypatch)


def test_every_tensor_is_read_once(tmp_path, emul, monkeypatch):
    fc.check_reads(tmp_path, emul, monkeypatch)
