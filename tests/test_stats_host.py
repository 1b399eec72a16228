"""analyze / Engine.delta_stats without a GPU: the kernels of csrc/sm_stats.hpp (and geo_gram's) on the CPU work-group
emulator against tests/stats_oracle.py (every report field bit for bit, tests/stats_checks.py), the identities with
ties_merge and geo_merge through the same engine, the C ABI, the launch counts, and `python -m shard analyze` end to end
with the emulator as the device."""
import json

import pytest
import torch

from tests import lora_fixtures as lf
from tests import stats_checks as sc
from tests.harness import DTYPES, emul, make_inputs, ties_models  # noqa: F401


# ---- the kernels on the emulator against the oracle ---------------------------------------------------------
@pytest.mark.parametrize("n", sc.SIZES)
def test_sizes(emul, n):
    sc.check_size(emul, n)


@pytest.mark.parametrize("m", sc.MS)
@pytest.mark.parametrize("k", sc.KS)
def test_k_and_m(emul, k, m):
    sc.check_k_m(emul, k, m)


@pytest.mark.parametrize("in_dtype", DTYPES, ids=str)
def test_dtypes(emul, in_dtype):
    sc.check_dtypes(emul, in_dtype)


@pytest.mark.parametrize("check", sc.CORNERS, ids=lambda f: f.__name__[len("check_"):])
def test_corner(emul, check):
    check(emul)


@pytest.mark.parametrize("m", sc.MS)
@pytest.mark.parametrize("k", (2, 4, 5, 16))
def test_profile_names_and_launches(emul, k, m):
    sc.check_profile(emul, k, m)


def test_c_abi_rejects_bad_arguments(emul):
    sc.check_c_abi(emul)


def test_report_dataclass_holds_python_values(emul):
    fts, bases, _ = make_inputs((16, 16), 2, seed=1)
    rep = emul.delta_stats(fts, bases, [0.5, 0.5], (0.5,))
    assert type(rep.n) is int and type(rep.kept[0][0]) is int and type(rep.thresholds[0][0]) is float
    assert type(rep.gram[0][1]) is float and type(rep.energy[0][0]) is float and type(rep.cover[0][2]) is int
    assert len(rep.cover[0]) == 3 and len(rep.gram) == 2 and type(rep.conflict[0]) is int


# ---- the CLI end to end ------------------------------------------------------------------------------------------
def _tree(root):
    return sorted(str(p.relative_to(root)) for p in root.rglob("*"))


def test_cli_equals_the_oracle_tensor_by_tensor(tmp_path, emul):
    base, factors, full = lf.setup_k3(tmp_path, emul)
    cfg = sc.write_config(tmp_path, "org/lora_full", "merged", {"operator": "ties", "density": 0.3})
    res = sc.run_cli(["analyze", cfg])
    assert res.exit_code == 0, res.output
    # nothing but the report under output_dir
    assert _tree(tmp_path / "merged") == ["analysis.json"]
    expected = sc.expected_records(base, full, sc.DENS4)
    assert [len(t["entries"]) for t in expected] == [3] * 4 + [2] * 4          # the layer windows decide who covers a tensor
    doc = sc.assert_report(tmp_path / "merged" / "analysis.json", expected, sc.DENS4)
    assert any(c > 0 for c in doc["model"]["conflict"]) and all(0 < v for row in doc["model"]["kept"] for v in row)
    # the tables
    for word in ("8 block tensor(s)", "3 passthrough tensor(s)", "[0] org/ft1", "[2] org/lora_full", "cosine:", "opposed/kept",
                 "density 0.05: conflict", "report:"):
        assert word in res.output, (word, res.output)
    # one finetune given as a LoRA adapter directory: the same numbers as on its materialised checkpoint
    other = tmp_path / "elsewhere" / "a.json"
    res = sc.run_cli(["analyze", sc.write_config(tmp_path, "org/lora", "merged_adapter"), "--report", other, "--densities", "0.05,0.1,0.2,0.5"])
    assert res.exit_code == 0, res.output
    assert not (tmp_path / "merged_adapter").exists()                          # --report elsewhere: output_dir is not even created
    assert json.loads(other.read_text())["tensors"] == doc["tensors"]
    # other densities; no windows: every entry covers every block tensor
    models = [{**m, "end_layer": -1} for m in ties_models("org/lora_full")]
    res = sc.run_cli(["analyze", sc.write_config(tmp_path, "org/lora_full", "merged_all", models=models), "--densities", "1,0.5"])
    assert res.exit_code == 0, res.output
    expected = sc.expected_records(base, full, (1.0, 0.5), windows=False)
    assert [len(t["entries"]) for t in expected] == [3] * 8
    sc.assert_report(tmp_path / "merged_all" / "analysis.json", expected, (1.0, 0.5))


def test_a_merge_after_an_analysis_writes_the_same_bytes(tmp_path, emul):
    from tests.harness import run_cli as run_merge
    base, factors, full = lf.setup_k3(tmp_path, emul)
    opts = {"operator": "ties", "density": 0.3}
    assert sc.run_cli(["analyze", sc.write_config(tmp_path, "org/lora_full", "merged", opts)]).exit_code == 0
    before = (tmp_path / "merged" / "analysis.json").read_bytes()
    res = run_merge(sc.write_config(tmp_path, "org/lora_full", "merged", opts))
    assert res.exit_code == 0, res.output
    res = run_merge(sc.write_config(tmp_path, "org/lora_full", "merged_plain", opts))
    assert res.exit_code == 0, res.output
    lf.assert_same_outputs(tmp_path / "merged", tmp_path / "merged_plain")
    assert (tmp_path / "merged" / "analysis.json").read_bytes() == before
    for name in ("README.md", "model.safetensors.index.json"):
        assert (tmp_path / "merged" / name).read_bytes() == (tmp_path / "merged_plain" / name).read_bytes()
    assert sorted(set(_tree(tmp_path / "merged")) - set(_tree(tmp_path / "merged_plain"))) == ["analysis.json"]


@pytest.mark.parametrize("value,word", [("0.1,0.2,0.3,0.4,0.5", "5 densities"), ("0", "not in (0, 1]"), ("0.2,1.5", "not in (0, 1]"),
                                        ("-0.1", "not in (0, 1]"), ("nan", "not in (0, 1]"), ("0.2,x", "comma-separated"), ("", "comma-separated")])
def test_cli_rejects_bad_densities_before_anything_is_read(tmp_path, value, word):
    """no storage exists here: the option fails first"""
    cfg = sc.write_config(tmp_path, "org/lora_full", "merged")
    res = sc.run_cli(["analyze", cfg, "--densities", value])
    assert res.exit_code == 2 and word in res.output and "--densities" in res.output, res.output
    assert not (tmp_path / "merged").exists()


def test_cli_validates_merge_options_and_refuses_several_ranks(tmp_path, monkeypatch):
    cfg = sc.write_config(tmp_path, "org/lora_full", "merged", {"operator": "ties", "density": 1.5})
    res = sc.run_cli(["analyze", cfg])
    assert res.exit_code != 0 and not (tmp_path / "merged").exists()
    monkeypatch.setenv("WORLD_SIZE", "2")
    res = sc.run_cli(["analyze", sc.write_config(tmp_path, "org/lora_full", "merged")])
    assert res.exit_code != 0 and "single process" in res.output and not (tmp_path / "merged").exists()


def test_the_alias_package_has_the_command():
    from shard.__main__ import cli
    assert "analyze" in cli.commands and "merge" in cli.commands
