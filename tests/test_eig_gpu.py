"""The device-side eigensolver on the MI355X: `eig_jacobi` of csrc/sm_eig.hpp in its three residency plans
(tests/eig_checks.py)."""
import pytest

from tests import eig_checks as ec
from tests.harness import eng  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n,kind", ec.CASES, ids=lambda x: str(x))
def test_bit_for_bit_against_the_restatement(eng, n, kind):
    ec.check_bits(eng, n, kind)


def test_a_batch_of_three(eng):
    ec.check_batch(eng)


@pytest.mark.parametrize("kind", ec.KINDS)
@pytest.mark.parametrize("n", ec.ACCURACY_SIZES)
def test_accuracy_within_four_times_the_host_solver(eng, n, kind):
    ec.check_accuracy(eng, n, kind)


def test_arguments(eng):
    ec.check_arguments(eng)


@pytest.mark.parametrize("rows,cols", [(128, 512)] + [(300, 4544)], ids=lambda v: str(v))
def test_tsv_singular_values_with_the_device_solver(eng, rows, cols):
    ec.check_tsv_singular_values(eng, rows, cols)


def test_tsv_duplicates_and_the_host_setting(eng):
    ec.check_tsv_duplicates(eng)
    ec.check_tsv_host_is_unchanged(eng)


def test_extract_exact_rank_with_the_device_solver(eng):
    ec.check_extract_exact_rank(eng)


def test_cli_and_config(tmp_path, eng):
    ec.check_config(tmp_path)
    ec.check_cli(tmp_path, eng, device="cuda")


def test_tsv_bytes_equal_the_emulator(eng):
    from tests.emul.loader import emul_engine
    ec.check_tsv_against(eng, emul_engine())
