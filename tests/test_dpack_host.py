"""The delta pack on the CPU work-group emulator: the kernels of csrc/sm_dpack.hpp and their host path, the same source
the HIP library is built from, against tests/dpack_oracle.py bit for bit and against torch fp64 (tests/dpack_checks.py)."""
import pytest

from tests import dpack_checks as dc
from tests.harness import DTYPES, emul  # noqa: F401


@pytest.mark.parametrize("cols", dc.COLS)
def test_cols(emul, cols):
    dc.check_cols(emul, cols)


@pytest.mark.parametrize("rows", dc.ROWS)
def test_rows(emul, rows):
    dc.check_rows(emul, rows)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_dtypes(emul, dtype):
    dc.check_dtypes(emul, dtype)


@pytest.mark.parametrize("check", dc.CORNERS, ids=lambda f: f.__name__[len("check_"):])
def test_corner(emul, check):
    check(emul)


# ---- the format, the routing and the command, on the on-disk model of tests/lora_fixtures.py --------------------------
def test_command_writes_a_pack_that_merge_takes(tmp_path, emul):
    dc.check_command(tmp_path, emul, "cpu")


def test_one_bit_pack_with_modules_provides_the_embedding(tmp_path, emul):
    dc.check_command_forms(tmp_path, emul, "cpu")


def test_two_gloo_ranks_equal_the_oracle(tmp_path, emul):
    from tests import harness
    base, ft3, _ = dc.setup_pack(tmp_path, emul, "cpu")
    cfg = harness.write_config(tmp_path, dc.pack_models("org/pack"), "merged", dc.OPTIONS, "cpu")
    harness.run_ranks(cfg)
    assert not list((tmp_path / "merged").glob(".tmp-*"))
    harness.assert_outputs(tmp_path / "merged", dc.expected_outputs(base, dc.oracle_finetune(base, ft3, 2, 0.5, "row")))


def test_in_place_path_equals_the_oracle(tmp_path, emul, monkeypatch):
    from shardmerge_amd import distributed
    from tests import harness
    monkeypatch.setenv("SHARDMERGE_INPLACE", "1")
    monkeypatch.setattr(distributed, "ENGINE_FACTORY", lambda: emul)
    base, ft3, _ = dc.setup_pack(tmp_path, emul, "cpu")
    res = harness.run_cli(harness.write_config(tmp_path, dc.pack_models("org/pack"), "merged", dc.OPTIONS, "cpu"))
    assert res.exit_code == 0, res.output
    harness.assert_outputs(tmp_path / "merged", dc.expected_outputs(base, dc.oracle_finetune(base, ft3, 2, 0.5, "row")))


def test_config_stamp_follows_the_pack(tmp_path, emul):
    dc.check_stamp(tmp_path, emul, "cpu")


def test_reader_rejects_before_an_output_exists(tmp_path, emul):
    dc.check_reader_rejections(tmp_path, emul, "cpu")


def test_commands_reject_before_the_directory_exists(tmp_path, emul, monkeypatch):
    dc.check_command_rejections(tmp_path, emul, "cpu", monkeypatch)
