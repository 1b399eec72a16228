"""The device-side eigensolver on the CPU emulator, which runs the kernel source of csrc/sm_eig.hpp thread by thread
(tests/eig_checks.py)."""
import pytest

from tests import eig_checks as ec
from tests.harness import emul  # noqa: F401


@pytest.mark.parametrize("n,kind", [c for c in ec.CASES if c[0] < 272 or c[1] == "flat"], ids=lambda x: str(x))
def test_bit_for_bit_against_the_restatement(emul, n, kind):
    ec.check_bits(emul, n, kind)


def test_a_batch_of_three(emul):
    ec.check_batch(emul)


@pytest.mark.parametrize("kind", ec.KINDS)
@pytest.mark.parametrize("n", ec.ACCURACY_SIZES)
def test_accuracy_within_four_times_the_host_solver(emul, n, kind):
    ec.check_accuracy(emul, n, kind)


def test_arguments(emul):
    ec.check_arguments(emul)


@pytest.mark.parametrize("rows,cols", [(128, 512)], ids=lambda v: str(v))
def test_tsv_singular_values_with_the_device_solver(emul, rows, cols):
    ec.check_tsv_singular_values(emul, rows, cols)


def test_tsv_duplicates_and_the_host_setting(emul):
    ec.check_tsv_duplicates(emul)
    ec.check_tsv_host_is_unchanged(emul)


def test_extract_exact_rank_with_the_device_solver(emul):
    ec.check_extract_exact_rank(emul)


def test_cli_and_config(tmp_path, emul):
    ec.check_config(tmp_path)
    ec.check_cli(tmp_path, emul)
