"""operators karcher / multislerp without a GPU: the kernels of csrc/sm_sphere.hpp and csrc/sm_geo.hpp on the CPU work-group
emulator against tests/sphere_oracle.py (bit for bit, tests/sphere_checks.py), the three defined functions, the checks
that need no oracle, the YAML options, the stamp, and `python -m shard merge` end to end - single process, in place, and
two gloo ranks - with the emulator as the device."""
import click
import pytest
import torch

from shardmerge_amd import distributed
from shardmerge_amd.config import OPERATORS as ALL_OPERATORS
from shardmerge_amd.config import MergeConfig
from tests import lora_fixtures as lf
from tests import sphere_checks as sc
from tests.harness import ALPHAS, DTYPES, KS, assert_outputs, emul, make_inputs, run_cli, run_ranks, yaml_config  # noqa: F401

OPERATORS = ("karcher", "multislerp")
# what the CLI tests run: (operator, sphere_row_wise)
CLI_CASES = [("karcher", None), ("karcher", 1), ("multislerp", None), ("multislerp", 1)]
CLI_IDS = ["karcher", "karcher_row_wise", "multislerp", "multislerp_row_wise"]
NEW_KEYS = [("karcher_max_iter", 5), ("karcher_tol", 1e-6), ("sphere_row_wise", 1)]


# ---- the kernels on the emulator against the oracle ---------------------------------------------------------
@pytest.mark.parametrize("mode,rowwise", sc.VARIANTS, ids=sc.VARIANT_IDS)
@pytest.mark.parametrize("bo_dtype", DTYPES, ids=str)
@pytest.mark.parametrize("in_dtype", DTYPES, ids=str)
def test_dtypes(emul, in_dtype, bo_dtype, mode, rowwise):
    sc.check_dtypes(emul, in_dtype, bo_dtype, mode, rowwise)


@pytest.mark.parametrize("mode,rowwise", sc.VARIANTS, ids=sc.VARIANT_IDS)
@pytest.mark.parametrize("k", KS)
def test_k(emul, k, mode, rowwise):
    sc.check_k(emul, k, mode, rowwise)


def test_functions(emul):
    sc.check_functions(emul)


@pytest.mark.parametrize("check", sc.PROPERTIES, ids=lambda f: f.__name__[len("check_"):])
def test_property(emul, check):
    check(emul)


@pytest.mark.parametrize("check", sc.CORNERS, ids=lambda f: f.__name__[len("check_"):])
def test_corner(emul, check):
    check(emul)


@pytest.mark.parametrize("k", [2, 5, 16])
@pytest.mark.parametrize("mode,rowwise", sc.VARIANTS, ids=sc.VARIANT_IDS)
def test_profile_names_and_launches(emul, mode, rowwise, k):
    """ONE launch of each kernel per call, whatever k and the iteration count"""
    sc.check_profile(emul, mode, rowwise, k)


def test_c_abi_rejects_bad_arguments(emul):
    sc.check_c_abi(emul)


def test_existing_entry_points_keep_their_limits(emul):
    """the new operators have their own entry point: geo_merge still knows three modes and pairs only"""
    fts, bases, bo = make_inputs((8, 8), 3, seed=1)
    for mode in ("karcher", "multislerp"):
        with pytest.raises(ValueError, match="mode"):
            emul.geo_merge(fts, bases, ALPHAS[:3], bo, mode=mode)
    with pytest.raises(ValueError, match="at most 2"):
        emul.geo_merge(fts, bases, ALPHAS[:3], bo, mode="slerp")


# ---- YAML ------------------------------------------------------------------------------------------------------
TRIPLE = [{"model": "org/ft1", "base": "org/base"}, {"model": "org/ft2", "base": "org/base"},
          {"model": "org/ft3", "base": "org/base"}]


@pytest.mark.parametrize("operator", OPERATORS)
def test_yaml_accepts_the_operators_and_their_defaults(tmp_path, operator):
    from shardmerge_amd.merge import operator_class
    from shardmerge_amd.merge.fast_fourier import FourierMerge
    from shardmerge_amd.merge.spherical import KarcherMerge, MultiSlerpMerge
    from shardmerge_amd.merge.ties import TiesMerge
    cls = operator_class(operator)
    assert cls is {"karcher": KarcherMerge, "multislerp": MultiSlerpMerge}[operator] and issubclass(cls, TiesMerge)
    cfg = MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": operator}, TRIPLE))
    assert cfg.operator == operator and cfg.merge_options == {}
    m = cls(config=cfg, index_manager=object())
    assert m.mode == operator and not m.sphere_row_wise and int(m.karcher_max_iter) == 10 and m.karcher_tol == 1e-5
    readme = m.get_readme()
    for word in (f"{operator}:", "org/ft1", "org/ft3", "max_iter 10", "tol 1e-05", "per tensor", "weights [0.333333, 0.333333, 0.333333]"):
        assert word in readme, (word, readme)
    assert cls.merge_block is not TiesMerge.merge_block and cls._merge_layer is FourierMerge._merge_layer
    assert [m.tensor_passes(k) for k in (2, 3)] == ([5, 7] if operator == "karcher" else [7, 9])
    assert m.block_cost_ms((128, 64), 3) == TiesMerge.block_cost_ms(m, (128, 64), 3)
    # any number of entries >= 1
    for n in (1, 2, 16):
        models = [{"model": f"org/ft{i}", "base": "org/base"} for i in range(n)]
        assert MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": operator}, models)).operator == operator


@pytest.mark.parametrize("operator", OPERATORS)
def test_yaml_keys(tmp_path, operator):
    from shardmerge_amd.merge import operator_class
    cfg = MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": operator, "karcher_max_iter": 25, "karcher_tol": 0, "sphere_row_wise": 1}, TRIPLE))
    assert cfg.merge_options == {"karcher_max_iter": 25, "karcher_tol": 0.0, "sphere_row_wise": 1.0}
    assert isinstance(cfg.merge_options["karcher_max_iter"], int)
    m = operator_class(operator)(config=cfg, index_manager=object())
    assert int(m.karcher_max_iter) == 25 and m.karcher_tol == 0.0 and bool(m.sphere_row_wise)
    for word in ("per row", "max_iter 25", "tol 0"):
        assert word in m.get_readme()
    for bad in (0, 101, 2.5, "ten", True):
        with pytest.raises(click.BadParameter, match=r"karcher_max_iter must be an integer in 1\.\.100"):
            MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": operator, "karcher_max_iter": bad}, TRIPLE))
    for bad in (-1e-9, 1, 1.5, "small", True):
        with pytest.raises(click.BadParameter, match=r"karcher_tol must be a number in \[0, 1\)"):
            MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": operator, "karcher_tol": bad}, TRIPLE))
    for bad in (2, 0.5, -1, "yes", True):
        with pytest.raises(click.BadParameter, match="sphere_row_wise must be 0 or 1"):
            MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": operator, "sphere_row_wise": bad}, TRIPLE))


@pytest.mark.parametrize("key,value", NEW_KEYS)
@pytest.mark.parametrize("operator", [None] + [op for op in ALL_OPERATORS if op not in OPERATORS])
def test_yaml_rejects_the_new_keys_with_every_other_operator(tmp_path, operator, key, value):
    opts = {key: value}
    if operator:
        opts["operator"] = operator
    models = [{"model": "org/ft1", "base": "org/base"}, {"model": "org/ft2", "base": "org/base"}]
    with pytest.raises(click.BadParameter, match=rf"merge_options\.{key} is accepted only with operator: karcher or multislerp \("):
        MergeConfig.from_yaml(yaml_config(tmp_path, opts, models))


@pytest.mark.parametrize("operator", OPERATORS)
@pytest.mark.parametrize("key,value", [("cutoff_pct", 0.08), ("cull_start_pct", 0.2), ("t_sum", 1.0), ("target_norm_offset", 1e-10),
                                       ("b", 0.1), ("norm_mode", "exact"), ("task_add_models", ["org/ft1"]), ("density", 0.5),
                                       ("ties_lambda", 1.0), ("ties_normalize", 1), ("dare_lambda", 1.0), ("dare_normalize", 1),
                                       ("dare_rescale", 1), ("seed", 0), ("gamma", 0.01), ("breadcrumbs_lambda", 1.0),
                                       ("breadcrumbs_normalize", 1), ("stock_filter_wise", 1), ("select_topk", 0.5), ("sce_lambda", 1.0),
                                       ("epsilon", 0.1), ("della_lambda", 1.0), ("della_normalize", 1), ("della_rescale", 1),
                                       ("mask_lambda", 0.4), ("consensus_k", 2), ("consensus_lambda", 1.0), ("consensus_normalize", 1),
                                       ("bogus", 1)])
def test_yaml_rejects_an_option_the_operators_would_ignore(tmp_path, operator, key, value):
    with pytest.raises(click.BadParameter, match=key) as e:
        MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": operator, key: value}, TRIPLE))
    assert f"merge_options.{key}" in str(e.value) or key == "bogus"
    assert f"operator {operator!r} would ignore it" in str(e.value) or f"operator {operator!r} takes no norm" in str(e.value) or key == "bogus"


@pytest.mark.parametrize("operator", OPERATORS)
def test_yaml_alpha_rule(tmp_path, operator):
    entry = lambda i, a=1.0: {"model": f"org/ft{i}", "base": "org/base", "alpha": a}
    for alphas in ((-0.5, 1.0), (0.5, -0.1, 1.0), (0.0, 0.0), (0.0,), (float("nan"), 1.0), (float("inf"), 1.0), (True, 1.0)):
        with pytest.raises(click.BadParameter, match=f"operator {operator} needs finetune_merge alphas >= 0 with a sum > 0"):
            MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": operator}, [entry(i, a) for i, a in enumerate(alphas)]))
    assert MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": operator}, [entry(1, 1.0), entry(2, 0.0), entry(3, 2)])).operator == operator


def test_config_stamp(tmp_path):
    stamp = lambda opts: distributed.config_stamp(MergeConfig.from_yaml(yaml_config(tmp_path, opts, [{"model": "org/ft1", "base": "org/base"},
                                                                                              {"model": "org/ft2", "base": "org/base"}])))
    base = stamp({"operator": "karcher"})
    assert base == stamp({"operator": "karcher"})
    others = [stamp({"operator": "multislerp"}), stamp({"operator": "karcher", "karcher_max_iter": 11}),
              stamp({"operator": "karcher", "karcher_tol": 1e-6}), stamp({"operator": "karcher", "sphere_row_wise": 1}),
              stamp({"operator": "multislerp", "sphere_row_wise": 1}), stamp({"operator": "slerp"}), stamp({"operator": "nuslerp"}),
              stamp({"operator": "model_stock"}), stamp(None)]
    assert len({base, *others}) == len(others) + 1


# ---- the CLI end to end ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("operator,row_wise", CLI_CASES, ids=CLI_IDS)
def test_cli_equals_the_oracle_tensor_by_tensor(tmp_path, emul, operator, row_wise):
    base, factors, full = lf.setup_k3(tmp_path, emul)
    opts = sc.options(operator, row_wise)
    expected = sc.expected_outputs(base, full, opts)
    assert any(not torch.equal(expected[n], base[n]) for n in expected if "layers" in n)
    res = run_cli(sc.write_config(tmp_path, "org/lora_full", "merged", opts))
    assert res.exit_code == 0, res.output
    assert_outputs(tmp_path / "merged", expected)
    readme = (tmp_path / "merged" / "README.md").read_text()
    for word in sc.README_WORDS[operator] + (("per row",) if row_wise else ("per tensor",)):
        assert word in readme, (word, readme)
    # one finetune given as a LoRA adapter directory: the run on its materialised checkpoint
    res = run_cli(sc.write_config(tmp_path, "org/lora", "merged_adapter", opts))
    assert res.exit_code == 0, res.output
    lf.assert_same_outputs(tmp_path / "merged_adapter", tmp_path / "merged")
    # the other granularity and the other operator are other models
    for other_opts in (sc.options(operator, 0 if row_wise else 1), sc.options(OPERATORS[1 - OPERATORS.index(operator)], row_wise)):
        other = sc.expected_outputs(base, full, other_opts)
        assert any(not torch.equal(other[n], expected[n]) for n in expected if "layers" in n), other_opts


@pytest.mark.parametrize("operator,row_wise", CLI_CASES, ids=CLI_IDS)
def test_cli_in_place_equals_the_oracle(tmp_path, emul, monkeypatch, operator, row_wise):
    """the partitioned path merges block tensors itself (distributed._merge_block_tensor): it must run these operators too"""
    monkeypatch.setenv("SHARDMERGE_INPLACE", "1")
    monkeypatch.setattr(distributed, "ENGINE_FACTORY", lambda: emul)
    base, factors, full = lf.setup_k3(tmp_path, emul)
    opts = sc.options(operator, row_wise, karcher_max_iter=20)
    res = run_cli(sc.write_config(tmp_path, "org/lora", "merged", opts))
    assert res.exit_code == 0, res.output
    assert_outputs(tmp_path / "merged", sc.expected_outputs(base, full, opts))
    readme = (tmp_path / "merged" / "README.md").read_text()
    assert sc.README_WORDS[operator][0] in readme and "max_iter 20" in readme


@pytest.mark.parametrize("operator,row_wise", CLI_CASES, ids=CLI_IDS)
def test_two_gloo_ranks_equal_the_oracle(tmp_path, emul, operator, row_wise):
    base, factors, full = lf.setup_k3(tmp_path, emul)
    opts = sc.options(operator, row_wise)
    cfg = sc.write_config(tmp_path, "org/lora", "merged", opts, device="cpu")
    run_ranks(cfg)
    assert not list((tmp_path / "merged").glob(".tmp-*"))
    assert_outputs(tmp_path / "merged", sc.expected_outputs(base, full, opts))
