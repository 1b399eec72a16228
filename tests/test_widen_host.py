"""operator: widen without a GPU: the kernels of csrc/sm_widen.hpp on the CPU work-group emulator against
tests/widen_oracle.py (bit for bit, tests/widen_checks.py), the column sums against math.fsum, the function against a
torch fp64 restatement of the paper's form, the properties, the YAML options, the stamp, the column limit in
initialize(), and `python -m shard merge` / `analyze` end to end - single process, in place, and two gloo ranks - with
the emulator as the device."""
import click
import pytest
import torch
import yaml
from click.testing import CliRunner

from shardmerge_amd import distributed
from shardmerge_amd.config import OPERATORS, WIDEN_OPERATORS, MergeConfig
from tests import lora_fixtures as lf
from tests import widen_checks as wc
from tests.harness import DTYPES, assert_outputs, emul, run_cli, run_ranks, ties_models, yaml_config  # noqa: F401

KEYS = ["widen_ratio", "widen_calibration", "widen_lambda"]


# ---- the kernels on the emulator against the oracle ---------------------------------------------------------
@pytest.mark.parametrize("R", wc.ROWS)
def test_rows(emul, R):
    wc.check_rows(emul, R)


@pytest.mark.parametrize("C", wc.COLS)
def test_cols(emul, C):
    wc.check_cols(emul, C)


@pytest.mark.parametrize("own", [False, True], ids=["shared_base", "own_bases"])
@pytest.mark.parametrize("k", wc.KS)
def test_k(emul, k, own):
    wc.check_k(emul, k, own)


@pytest.mark.parametrize("bo_dtype", DTYPES, ids=str)
@pytest.mark.parametrize("in_dtype", DTYPES, ids=str)
def test_dtypes(emul, in_dtype, bo_dtype):
    wc.check_dtypes(emul, in_dtype, bo_dtype)


@pytest.mark.parametrize("lam", wc.LAMBDAS)
@pytest.mark.parametrize("calibration", wc.CALIBRATIONS)
@pytest.mark.parametrize("ratio", wc.RATIOS)
def test_options(emul, ratio, calibration, lam):
    wc.check_options(emul, ratio, calibration, lam)


@pytest.mark.parametrize("check", wc.CORNERS, ids=lambda f: f.__name__[len("check_"):])
def test_corner(emul, check):
    check(emul)


@pytest.mark.parametrize("shape,k,expected", wc.PROFILES, ids=wc.PROFILE_IDS)
def test_profile_names(emul, shape, k, expected):
    wc.check_profile(emul, shape, k, expected)


def test_c_abi_rejects_bad_arguments(emul):
    wc.check_c_abi(emul)


def test_column_sums_against_fsum(emul):
    wc.check_sums_against_fsum(emul)


@pytest.mark.parametrize("shape,k", wc.PAPER_CASES, ids=["x".join(map(str, s)) + f"-k{k}" for s, k in wc.PAPER_CASES])
def test_paper_form_in_fp64(emul, shape, k):
    """Measured on the emulator: no uncertain column, |d - d_ref| <= 3.2e-15, |w - w_ref| <= 2^-24 |w_ref|, delta_out at
    most 0.65 of its bound."""
    wc.check_paper_form(emul, shape, k)


# ---- YAML ------------------------------------------------------------------------------------------------------
def test_yaml_accepts_the_operator_and_its_keys(tmp_path):
    from shardmerge_amd.merge import operator_class
    from shardmerge_amd.merge.fast_fourier import FourierMerge
    from shardmerge_amd.merge.ties import TiesMerge
    from shardmerge_amd.merge.widen import WidenMerge
    cls = operator_class("widen")
    assert cls is WidenMerge and issubclass(cls, TiesMerge) and "widen" in OPERATORS and WIDEN_OPERATORS == ("widen",)
    cfg = MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": "widen"}))
    assert cfg.operator == "widen" and cfg.merge_options == {}
    m = cls(config=cfg, index_manager=object())
    assert (m.widen_ratio, m.widen_calibration, m.widen_lambda) == (1.0, 1.0, 1.0)
    cfg = MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": "widen", "widen_ratio": -1, "widen_calibration": 0, "widen_lambda": 0.7}))
    assert cfg.merge_options == {"widen_ratio": -1.0, "widen_calibration": 0.0, "widen_lambda": 0.7}
    m = cls(config=cfg, index_manager=object())
    readme = m.get_readme()
    for word in ("# WIDEN Merged Model", "WIDEN (", "ratio -1", "calibration 0", "lambda 0.7", "org/ft1"):
        assert word in readme, (word, readme)
    for edge in ({"widen_ratio": -1e6}, {"widen_ratio": 1e6}, {"widen_calibration": 0}, {"widen_calibration": 1e6},
                 {"widen_lambda": -1e6}, {"widen_lambda": 1e6}):
        assert MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": "widen", **edge})).merge_options == {k: float(v) for k, v in edge.items()}
    assert cls.merge_block is not TiesMerge.merge_block and cls._merge_layer is FourierMerge._merge_layer
    assert [m.tensor_passes(k) for k in (1, 2, 3)] == [5, 8, 11]


@pytest.mark.parametrize("options,text", [
    ({"widen_ratio": 1e7}, r"\[-1000000\.0, 1000000\.0\]"), ({"widen_ratio": -1e7}, r"\[-1000000\.0, 1000000\.0\]"),
    ({"widen_ratio": "1"}, r"\[-1000000\.0, 1000000\.0\]"), ({"widen_ratio": True}, r"\[-1000000\.0, 1000000\.0\]"),
    ({"widen_ratio": float("nan")}, r"\[-1000000\.0, 1000000\.0\]"),
    ({"widen_calibration": -1e-9}, r"\[0, 1000000\.0\]"), ({"widen_calibration": 1e7}, r"\[0, 1000000\.0\]"),
    ({"widen_calibration": "x"}, r"\[0, 1000000\.0\]"), ({"widen_calibration": float("inf")}, r"\[0, 1000000\.0\]"),
    ({"widen_lambda": 1e7}, r"\[-1000000\.0, 1000000\.0\]"), ({"widen_lambda": "x"}, r"\[-1000000\.0, 1000000\.0\]"),
    ({"widen_lambda": float("inf")}, r"\[-1000000\.0, 1000000\.0\]")], ids=str)
def test_yaml_rejects_out_of_range_values(tmp_path, options, text):
    (key, _), = options.items()
    with pytest.raises(click.BadParameter, match=rf"merge_options\.{key} must be a number in {text}"):
        MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": "widen", **options}))


@pytest.mark.parametrize("operator", [None] + [op for op in OPERATORS if op != "widen"])
@pytest.mark.parametrize("key", KEYS)
def test_yaml_rejects_a_widen_key_with_another_operator(tmp_path, operator, key):
    opts = {key: 0.5}
    if operator:
        opts["operator"] = operator
    shown = operator or "fourier"
    with pytest.raises(click.BadParameter, match=rf"merge_options\.{key} is accepted only with operator: widen \(operator '{shown}' would ignore it\)"):
        MergeConfig.from_yaml(yaml_config(tmp_path, opts))


@pytest.mark.parametrize("key,value", [("cutoff_pct", 0.08), ("cull_start_pct", 0.2), ("t_sum", 1.0), ("target_norm_offset", 1e-10),
                                       ("b", 0.1), ("norm_mode", "exact"), ("task_add_models", ["org/ft1"]), ("density", 0.2),
                                       ("ties_lambda", 1.0), ("ties_normalize", 1), ("dare_lambda", 1.0), ("dare_rescale", 1),
                                       ("seed", 0), ("gamma", 0.01), ("breadcrumbs_lambda", 1.0), ("stock_filter_wise", 1),
                                       ("select_topk", 0.5), ("sce_lambda", 1.0), ("epsilon", 0.1), ("della_lambda", 1.0),
                                       ("mask_lambda", 0.4), ("consensus_k", 2), ("karcher_max_iter", 10), ("karcher_tol", 1e-5),
                                       ("sphere_row_wise", 1), ("fusion_iqr", 1.5), ("nearswap_t", 0.001), ("pcb_ratio", 0.1),
                                       ("pcb_clip", 0.0001), ("pcb_lambda", 1.0), ("tsv_rank", 64), ("tsv_power_iters", 2),
                                       ("tsv_lambda", 1.0), ("bogus", 1)])
def test_yaml_rejects_an_option_widen_would_ignore(tmp_path, key, value):
    """the message names the rejected key itself and the operator that would ignore it"""
    named = r"unknown keys \['bogus'\]" if key == "bogus" else rf"merge_options\.{key}\b.*operator 'widen'"
    with pytest.raises(click.BadParameter, match=named):
        MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": "widen", key: value}))


def test_yaml_words_the_rejections_as_the_families_do(tmp_path):
    for opts, text in (({"karcher_tol": 1e-5}, r"merge_options\.karcher_tol is accepted only with operator: karcher or multislerp \(operator 'widen' would ignore it\)"),
                       ({"density": 0.2}, r"merge_options\.density is an option of operator ties; operator 'widen' would ignore it \(it trims nothing and weighs by column: widen_ratio, widen_lambda\)"),
                       ({"seed": 1}, r"merge_options\.seed is an option of operators dare_ties / dare_linear; operator 'widen' would ignore it \(it drops nothing at random\)"),
                       ({"pcb_ratio": 0.1}, r"merge_options\.pcb_ratio is accepted only with operator: pcb \(operator 'widen' would ignore it\)"),
                       ({"tsv_rank": 8}, r"merge_options\.tsv_rank is accepted only with operator: tsv \(operator 'widen' would ignore it\)"),
                       ({"cutoff_pct": 0.1}, r"merge_options\.cutoff_pct is an option of the spectral operators; operator 'widen' would ignore it"),
                       ({"norm_mode": "exact"}, r"merge_options\.norm_mode is an option of the spectral operators; operator 'widen' takes no norm")):
        with pytest.raises(click.BadParameter, match=text):
            MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": "widen", **opts}))


def test_a_zero_alpha_sum_is_no_error(tmp_path):
    doc = yaml.safe_load(yaml_config(tmp_path, {"operator": "widen"}).read_text())
    doc["finetune_merge"] = [{"model": "org/ft1", "base": "org/base", "alpha": 0.5}, {"model": "org/ft2", "base": "org/base", "alpha": -0.5}]
    (tmp_path / "cfg.yaml").write_text(yaml.safe_dump(doc))
    assert [m.alpha for m in MergeConfig.from_yaml(tmp_path / "cfg.yaml").finetune_merge] == [0.5, -0.5]


def test_config_stamp(tmp_path):
    stamp = lambda opts: distributed.config_stamp(MergeConfig.from_yaml(yaml_config(tmp_path, opts)))
    full = {"operator": "widen", "widen_ratio": 1.0, "widen_calibration": 1.0, "widen_lambda": 1.0}
    base = stamp(full)
    assert base == stamp(dict(full))
    others = [stamp({**full, "widen_ratio": 0.5}), stamp({**full, "widen_calibration": 0.9}), stamp({**full, "widen_lambda": 0.9}),
              stamp({"operator": "ties", "density": 0.2}), stamp({"operator": "pcb"}), stamp(None)]
    assert len({base, *others}) == len(others) + 1


# ---- the CLI end to end ------------------------------------------------------------------------------------------
def test_cli_equals_the_oracle_tensor_by_tensor(tmp_path, emul):
    base, factors, full = lf.setup_k3(tmp_path, emul)
    opts = wc.OPTIONS
    expected = wc.expected_outputs(emul, base, full, opts)
    assert any(not torch.equal(expected[n], base[n]) for n in expected if "layers" in n)
    res = run_cli(wc.write_config(tmp_path, "org/lora_full", "merged", opts))
    assert res.exit_code == 0, res.output
    assert_outputs(tmp_path / "merged", expected)           # (passthrough tensors included: torch.equal)
    readme = (tmp_path / "merged" / "README.md").read_text()
    for word in ("# WIDEN Merged Model", "WIDEN (", "ratio 0.5", "calibration 0.8", "lambda 0.7"):
        assert word in readme, (word, readme)
    # two runs give the same bytes
    res = run_cli(wc.write_config(tmp_path, "org/lora_full", "merged_again", opts))
    assert res.exit_code == 0, res.output
    lf.assert_same_outputs(tmp_path / "merged_again", tmp_path / "merged")
    # one finetune given as a LoRA adapter directory: the run on its materialised checkpoint
    res = run_cli(wc.write_config(tmp_path, "org/lora", "merged_adapter", opts))
    assert res.exit_code == 0, res.output
    lf.assert_same_outputs(tmp_path / "merged_adapter", tmp_path / "merged")
    # the default options
    res = run_cli(wc.write_config(tmp_path, "org/lora_full", "merged_default", {"operator": "widen"}))
    assert res.exit_code == 0, res.output
    assert_outputs(tmp_path / "merged_default", wc.expected_outputs(emul, base, full, {"operator": "widen"}))
    # analyze keeps accepting the config: the operator's options are validated and not used
    from shardmerge_amd.__main__ import cli
    res = CliRunner().invoke(cli, ["analyze", str(wc.write_config(tmp_path, "org/lora_full", "analysed", opts))])
    assert res.exit_code == 0, res.output


def test_cli_a_window_that_leaves_one_entry(tmp_path, emul):
    """layer 1 is covered by the third entry alone: the function at k = 1; ft2 has a base of its own (ft1)"""
    base, factors, full = lf.setup_k3(tmp_path, emul)
    models = ties_models("org/lora_full")
    models[0]["end_layer"] = 0
    cfg = yaml.safe_load(wc.write_config(tmp_path, "org/lora_full", "merged", wc.OPTIONS).read_text())
    cfg["finetune_merge"] = models
    path = tmp_path / "one_entry.yaml"
    path.write_text(yaml.safe_dump(cfg))
    res = run_cli(path)
    assert res.exit_code == 0, res.output
    assert_outputs(tmp_path / "merged", wc.expected_outputs(emul, base, full, wc.OPTIONS, models=models))


def test_cli_in_place_equals_the_oracle(tmp_path, emul, monkeypatch):
    """the partitioned path merges block tensors itself (distributed._merge_block_tensor): it must run WIDEN too"""
    monkeypatch.setenv("SHARDMERGE_INPLACE", "1")
    monkeypatch.setattr(distributed, "ENGINE_FACTORY", lambda: emul)
    base, factors, full = lf.setup_k3(tmp_path, emul)
    res = run_cli(wc.write_config(tmp_path, "org/lora", "merged", wc.OPTIONS))
    assert res.exit_code == 0, res.output
    assert_outputs(tmp_path / "merged", wc.expected_outputs(emul, base, full, wc.OPTIONS))
    assert "WIDEN" in (tmp_path / "merged" / "README.md").read_text()


@pytest.mark.parametrize("inplace", [False, True], ids=["single_process", "inplace"])
def test_too_many_columns_fail_in_initialize(tmp_path, emul, monkeypatch, inplace):
    """a block tensor of the output base with 65537 columns: an error that names it, before anything is written"""
    from safetensors.torch import load_file, save_file
    if inplace:
        monkeypatch.setenv("SHARDMERGE_INPLACE", "1")
        monkeypatch.setattr(distributed, "ENGINE_FACTORY", lambda: emul)
    lf.setup_k3(tmp_path, emul)
    shard = tmp_path / "storage" / "org/base" / "model-00001-of-00002.safetensors"
    tensors = load_file(str(shard))
    tensors["model.layers.0.mlp.wide.weight"] = torch.zeros((2, 65537), dtype=torch.bfloat16)
    save_file(tensors, str(shard), metadata={"format": "pt"})
    res = run_cli(wc.write_config(tmp_path, "org/lora_full", "merged", wc.OPTIONS))
    assert res.exit_code != 0
    text = res.output + repr(res.exception)
    assert "model.layers.0.mlp.wide.weight" in text and "65537 columns" in text and "at most 65536" in text, text
    assert not (tmp_path / "merged").exists()


def test_two_gloo_ranks_equal_the_oracle(tmp_path, emul):
    base, factors, full = lf.setup_k3(tmp_path, emul)
    cfg = wc.write_config(tmp_path, "org/lora", "merged", wc.OPTIONS, device="cpu")
    run_ranks(cfg)
    assert not list((tmp_path / "merged").glob(".tmp-*"))
    assert_outputs(tmp_path / "merged", wc.expected_outputs(emul, base, full, wc.OPTIONS))
