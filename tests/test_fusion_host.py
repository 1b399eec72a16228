"""operator: arcee_fusion / nearswap without a GPU: the kernels of csrc/sm_fusion.hpp on the CPU work-group emulator against
tests/fusion_oracle.py (bit for bit, tests/fusion_checks.py), the YAML options, the coverage rule, the stamp, and
`python -m shard merge` / `analyze` end to end - single process, in place, and two gloo ranks - with the emulator as the
device."""
import click
import pytest
import torch
from click.testing import CliRunner

from shardmerge_amd import distributed
from shardmerge_amd.config import MergeConfig
from tests import fusion_checks as fc
from tests import lora_fixtures as lf
from tests.harness import DTYPES, assert_outputs, emul, run_cli, run_ranks, write_config, yaml_config  # noqa: F401

OPERATORS = ("arcee_fusion", "nearswap")
OWN = {"arcee_fusion": {"fusion_iqr": 1.5}, "nearswap": {"nearswap_t": 1e-3}}


# ---- the kernels on the emulator against the oracle ---------------------------------------------------------
def test_sm_exp_and_sm_log(emul):
    fc.check_functions(emul)


@pytest.mark.parametrize("R", fc.ROWS)
@pytest.mark.parametrize("C", fc.COLS)
def test_shapes(emul, C, R):
    fc.check_shape(emul, C, R)


@pytest.mark.parametrize("bo_dtype", DTYPES, ids=str)
@pytest.mark.parametrize("in_dtype", DTYPES, ids=str)
def test_dtypes(emul, in_dtype, bo_dtype):
    fc.check_dtypes(emul, in_dtype, bo_dtype)


@pytest.mark.parametrize("check", fc.CORNERS, ids=lambda f: f.__name__[len("check_"):])
def test_corner(emul, check):
    check(emul)


def test_largest_emulator_shape(emul):
    ft, base, bo = fc.fusion_inputs((16, 28672), torch.bfloat16, torch.float32, seed=5)
    fc.check(emul, ft, base, bo, "arcee", label="16 x 28672")
    fc.check(emul, ft, base, bo, "nearswap", t=1e-3, label="16 x 28672")


@pytest.mark.parametrize("mode,expected", fc.PROFILES, ids=[p[0] for p in fc.PROFILES])
def test_profile_names_and_launches(emul, mode, expected):
    fc.check_profile(emul, mode, expected)


def test_c_abi_rejects_bad_arguments(emul):
    fc.check_c_abi(emul)


# ---- YAML ------------------------------------------------------------------------------------------------------
def test_yaml_accepts_the_operators_and_their_keys(tmp_path):
    from shardmerge_amd.merge import operator_class
    from shardmerge_amd.merge.fast_fourier import FourierMerge
    from shardmerge_amd.merge.fusion import ArceeFusionMerge, NearSwapMerge
    from shardmerge_amd.merge.ties import TiesMerge
    assert operator_class("arcee_fusion") is ArceeFusionMerge and operator_class("nearswap") is NearSwapMerge
    assert issubclass(NearSwapMerge, TiesMerge) and ArceeFusionMerge._merge_layer is FourierMerge._merge_layer
    cfg = MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": "arcee_fusion"}))
    assert cfg.operator == "arcee_fusion" and cfg.merge_options == {}
    m = ArceeFusionMerge(config=cfg, index_manager=object())
    assert m.fusion_iqr == 1.5 and m.tensor_passes(1) == 12
    assert "fusion_iqr 1.5" in m.get_readme() and "arcee_fusion" in m.get_readme() and "org/ft1" in m.get_readme()
    for value in (-1e6, 0, 1e6):
        assert MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": "arcee_fusion", "fusion_iqr": value})).merge_options == {"fusion_iqr": float(value)}
    cfg = MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": "nearswap", "nearswap_t": 0.002}))
    assert cfg.merge_options == {"nearswap_t": 0.002}
    m = NearSwapMerge(config=cfg, index_manager=object())
    assert m.nearswap_t == 0.002 and m.tensor_passes(1) == 4
    assert "nearswap_t 0.002" in m.get_readme() and "# NearSwap Merged Model" in m.get_readme() and "org/ft1" in m.get_readme()
    assert MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": "nearswap", "nearswap_t": 1e6})).merge_options == {"nearswap_t": 1e6}


@pytest.mark.parametrize("operator,options", [("arcee_fusion", {"fusion_iqr": 1.1e6}), ("arcee_fusion", {"fusion_iqr": -1.1e6}),
                                              ("arcee_fusion", {"fusion_iqr": "1.5"}), ("arcee_fusion", {"fusion_iqr": True}),
                                              ("arcee_fusion", {"fusion_iqr": float("nan")}), ("nearswap", {"nearswap_t": 0}),
                                              ("nearswap", {"nearswap_t": -1e-3}), ("nearswap", {"nearswap_t": "x"}),
                                              ("nearswap", {"nearswap_t": 1.1e6}), ("nearswap", {"nearswap_t": float("nan")}),
                                              ("nearswap", {"nearswap_t": True})], ids=str)
def test_yaml_rejects_out_of_range_values(tmp_path, operator, options):
    (key, _), = options.items()
    with pytest.raises(click.BadParameter, match=key):
        MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": operator, **options}))


def test_yaml_requires_nearswap_t(tmp_path):
    with pytest.raises(click.BadParameter, match=r"merge_options\.nearswap_t is required with operator nearswap"):
        MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": "nearswap"}))


def test_yaml_rejects_the_other_operators_key(tmp_path):
    with pytest.raises(click.BadParameter, match=r"merge_options\.nearswap_t is accepted only with operator: nearswap \(operator 'arcee_fusion'"):
        MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": "arcee_fusion", "nearswap_t": 1e-3}))
    with pytest.raises(click.BadParameter, match=r"merge_options\.fusion_iqr is accepted only with operator: arcee_fusion \(operator 'nearswap'"):
        MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": "nearswap", "nearswap_t": 1e-3, "fusion_iqr": 1.5}))


@pytest.mark.parametrize("operator", [None, "fourier", "addition", "task_addition", "fourier_legacy", "ties", "dare_ties", "dare_linear",
                                      "breadcrumbs", "breadcrumbs_ties", "model_stock", "nuslerp", "slerp", "sce", "della", "della_linear",
                                      "consensus_ta", "consensus_ties", "karcher", "multislerp"])
@pytest.mark.parametrize("key,only", [("fusion_iqr", "arcee_fusion"), ("nearswap_t", "nearswap")])
def test_yaml_rejects_a_fusion_key_with_another_operator(tmp_path, operator, key, only):
    opts = {key: 1}
    if operator:
        opts["operator"] = operator
    entries = [{"model": "org/ft1", "base": "org/base"}, {"model": "org/ft2", "base": "org/base"}]
    with pytest.raises(click.BadParameter, match=rf"merge_options\.{key} is accepted only with operator: {only} \(operator '{operator or 'fourier'}'"):
        MergeConfig.from_yaml(yaml_config(tmp_path, opts, entries))


@pytest.mark.parametrize("operator", OPERATORS)
@pytest.mark.parametrize("key,value", [("cutoff_pct", 0.08), ("cull_start_pct", 0.2), ("t_sum", 1.0), ("target_norm_offset", 1e-10),
                                       ("b", 0.1), ("norm_mode", "exact"), ("task_add_models", ["org/ft1"]), ("density", 0.2),
                                       ("ties_lambda", 1.0), ("ties_normalize", 1), ("dare_lambda", 1.0), ("dare_normalize", 1),
                                       ("dare_rescale", 1), ("seed", 0), ("gamma", 0.01), ("breadcrumbs_lambda", 1.0),
                                       ("breadcrumbs_normalize", 1), ("stock_filter_wise", 1), ("select_topk", 0.5), ("sce_lambda", 1.0),
                                       ("epsilon", 0.1), ("della_lambda", 1.0), ("della_normalize", 1), ("della_rescale", 1),
                                       ("mask_lambda", 0.4), ("consensus_k", 2), ("consensus_lambda", 1.0), ("consensus_normalize", 1),
                                       ("karcher_max_iter", 10), ("karcher_tol", 1e-5), ("sphere_row_wise", 1), ("bogus", 1)])
def test_yaml_rejects_an_option_fusion_would_ignore(tmp_path, operator, key, value):
    """the message names the rejected key itself and the operator that would ignore it"""
    named = r"unknown keys \['bogus'\]" if key == "bogus" else rf"merge_options\.{key}\b.*operator '{operator}'"
    with pytest.raises(click.BadParameter, match=named):
        MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": operator, **OWN[operator], key: value}))


@pytest.mark.parametrize("operator", OPERATORS)
@pytest.mark.parametrize("alpha", [0.5, 0, 2, -1, True, "1"])
def test_yaml_rejects_an_alpha(tmp_path, operator, alpha):
    entries = [{"model": "org/ft1", "base": "org/base", "alpha": alpha}]
    with pytest.raises(click.BadParameter, match=rf"operator {operator} takes no weight.*org/ft1"):
        MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": operator, **OWN[operator]}, entries))
    entries[0]["alpha"] = 1.0
    MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": operator, **OWN[operator]}, entries))


def test_config_stamp(tmp_path):
    stamp = lambda opts: distributed.config_stamp(MergeConfig.from_yaml(yaml_config(tmp_path, opts)))
    base = stamp({"operator": "arcee_fusion", "fusion_iqr": 1.5})
    others = [stamp({"operator": "arcee_fusion", "fusion_iqr": 1.0}), stamp({"operator": "nearswap", "nearswap_t": 1e-3}),
              stamp({"operator": "nearswap", "nearswap_t": 2e-3}), stamp({"operator": "dare_linear", "density": 1.0}), stamp(None)]
    assert base == stamp({"operator": "arcee_fusion", "fusion_iqr": 1.5}) and len({base, *others}) == len(others) + 1


# ---- the CLI end to end ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("operator", OPERATORS)
def test_two_entries_on_one_layer_are_an_error_before_anything_is_written(tmp_path, emul, operator):
    lf.setup_k3(tmp_path, emul)
    entries = [{"model": "org/ft1", "base": "org/base", "is_input": True},
               {"model": "org/ft2", "base": "org/base", "is_output": True, "start_layer": 1}]
    res = run_cli(write_config(tmp_path, entries, "merged", fc.options(operator)))
    assert res.exit_code != 0
    text = res.output + str(res.exception)
    assert "layer 1 is covered by 2 finetune_merge entries (org/ft1, org/ft2)" in text and operator in text, text
    out = tmp_path / "merged"
    assert not out.exists() or not list(out.glob("*.safetensors"))
    # ... and a layer that no entry covers
    entries[0]["end_layer"], entries[1]["start_layer"] = 0, 2
    res = run_cli(write_config(tmp_path, entries, "merged2", fc.options(operator)))
    assert res.exit_code != 0 and "layer 1 is covered by 0 finetune_merge entries" in res.output + str(res.exception)
    assert not (tmp_path / "merged2").exists() or not list((tmp_path / "merged2").glob("*.safetensors"))


@pytest.mark.parametrize("operator", OPERATORS)
def test_cli_equals_the_oracle_tensor_by_tensor(tmp_path, emul, operator):
    base, factors, full = lf.setup_k3(tmp_path, emul)
    opts = fc.options(operator)
    expected = fc.expected_outputs(base, full, opts)
    assert any(not torch.equal(expected[n], base[n]) for n in expected if "layers" in n)
    res = run_cli(write_config(tmp_path, fc.models("org/lora_full"), "merged", opts))
    assert res.exit_code == 0, res.output
    assert_outputs(tmp_path / "merged", expected)
    readme = (tmp_path / "merged" / "README.md").read_text()
    for word in (operator, "fusion_iqr 1" if operator == "arcee_fusion" else "nearswap_t 0.002", "org/ft1", "org/lora_full", "layers 1..end"):
        assert word in readme, (word, readme)
    # the second entry given as a LoRA adapter directory: the run on its materialised checkpoint
    res = run_cli(write_config(tmp_path, fc.models("org/lora"), "merged_adapter", opts))
    assert res.exit_code == 0, res.output
    lf.assert_same_outputs(tmp_path / "merged_adapter", tmp_path / "merged")
    # analyze keeps accepting the config: the operator's options are validated and not used
    from shardmerge_amd.__main__ import cli
    res = CliRunner().invoke(cli, ["analyze", str(write_config(tmp_path, fc.models("org/lora_full"), "analysed", opts))])
    assert res.exit_code == 0, res.output


@pytest.mark.parametrize("operator", OPERATORS)
def test_cli_in_place_equals_the_oracle(tmp_path, emul, monkeypatch, operator):
    """the partitioned path merges block tensors itself (distributed._merge_block_tensor): it must run the fusion too"""
    monkeypatch.setenv("SHARDMERGE_INPLACE", "1")
    monkeypatch.setattr(distributed, "ENGINE_FACTORY", lambda: emul)
    base, factors, full = lf.setup_k3(tmp_path, emul)
    opts = fc.options(operator)
    res = run_cli(write_config(tmp_path, fc.models("org/lora"), "merged", opts))
    assert res.exit_code == 0, res.output
    assert_outputs(tmp_path / "merged", fc.expected_outputs(base, full, opts))


@pytest.mark.parametrize("operator", OPERATORS)
def test_two_gloo_ranks_equal_a_single_process(tmp_path, emul, operator):
    base, factors, full = lf.setup_k3(tmp_path, emul)
    opts = fc.options(operator)
    res = run_cli(write_config(tmp_path, fc.models("org/lora"), "single", opts))
    assert res.exit_code == 0, res.output
    cfg = write_config(tmp_path, fc.models("org/lora"), "merged", opts, device="cpu")
    run_ranks(cfg)
    assert not list((tmp_path / "merged").glob(".tmp-*"))
    lf.assert_same_outputs(tmp_path / "merged", tmp_path / "single", file_bytes=False)
    assert_outputs(tmp_path / "merged", fc.expected_outputs(base, full, opts))
