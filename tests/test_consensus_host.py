"""operator: consensus_ta / consensus_ties without a GPU: the kernel of csrc/sm_consensus.hpp (and, for consensus_ties, the
selection kernels of TIES) on the CPU work-group emulator against tests/consensus_oracle.py (bit for bit,
tests/consensus_checks.py), the YAML options, the stamp, and `python -m shard merge` end to end - single process, in
place, and two gloo ranks - with the emulator as the device."""
import click
import pytest
import torch

from shardmerge_amd import distributed
from shardmerge_amd.config import MergeConfig
from tests import consensus_checks as cc
from tests import lora_fixtures as lf
from tests.harness import (ALPHAS, DTYPES, assert_outputs, emul, make_inputs, run_cli, run_ranks,  # noqa: F401
                           yaml_config)

OPERATORS = ("consensus_ta", "consensus_ties")


# ---- the kernels on the emulator against the oracle ---------------------------------------------------------
@pytest.mark.parametrize("ties", cc.FLAVOURS, ids=cc.FLAVOUR_IDS)
@pytest.mark.parametrize("bo_dtype", DTYPES, ids=str)
@pytest.mark.parametrize("in_dtype", DTYPES, ids=str)
def test_dtypes(emul, in_dtype, bo_dtype, ties):
    cc.check_dtypes(emul, in_dtype, bo_dtype, ties)


@pytest.mark.parametrize("ties", cc.FLAVOURS, ids=cc.FLAVOUR_IDS)
@pytest.mark.parametrize("mask_lambda", cc.MASK_LAMBDAS)
@pytest.mark.parametrize("consensus_k", cc.CONSENSUS_KS)
@pytest.mark.parametrize("k", cc.KS)
def test_k_and_options(emul, k, consensus_k, mask_lambda, ties):
    cc.check_k_options(emul, k, consensus_k, mask_lambda, ties)


@pytest.mark.parametrize("ties", cc.FLAVOURS, ids=cc.FLAVOUR_IDS)
@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("lam", [1.0, 0.7])
def test_lambda_and_normalize(emul, lam, normalize, ties):
    cc.check_lambda_normalize(emul, lam, normalize, ties)


@pytest.mark.parametrize("ties", cc.FLAVOURS, ids=cc.FLAVOUR_IDS)
@pytest.mark.parametrize("n", cc.SIZES)
def test_sizes(emul, n, ties):
    cc.check_size(emul, n, ties)


@pytest.mark.parametrize("check", cc.CORNERS, ids=lambda f: f.__name__[len("check_"):])
def test_corner(emul, check):
    check(emul)


def test_largest_emulator_shape(emul):
    fts, bases, bo = make_inputs((512, 1024), 3, seed=5, own_bases=True)
    for ties in cc.FLAVOURS:
        cc.check(emul, fts, bases, ALPHAS[:3], bo, ties=ties, lam=0.7, label="512 x 1024")


@pytest.mark.parametrize("ties,k,expected", cc.PROFILES, ids=cc.PROFILE_IDS)
def test_profile_names_and_launches(emul, ties, k, expected):
    cc.check_profile(emul, ties, k, expected)


def test_c_abi_rejects_bad_arguments(emul):
    cc.check_c_abi(emul)


# ---- YAML ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("operator", OPERATORS)
def test_yaml_accepts_the_operators_and_their_keys(tmp_path, operator):
    from shardmerge_amd.merge import operator_class
    from shardmerge_amd.merge.consensus import ConsensusTaMerge, ConsensusTiesMerge
    from shardmerge_amd.merge.fast_fourier import FourierMerge
    from shardmerge_amd.merge.ties import TiesMerge
    ties = operator == "consensus_ties"
    cls = operator_class(operator)
    assert cls is (ConsensusTiesMerge if ties else ConsensusTaMerge) and issubclass(cls, TiesMerge)
    assert cls.ties is ties
    cfg = MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": operator}))
    assert cfg.operator == operator and cfg.merge_options == {}
    m = cls(config=cfg, index_manager=object())
    assert (m.mask_lambda, m.consensus_k, m.consensus_lambda, bool(m.consensus_normalize), m.density) == (0.4, 2, 1.0, True, 0.2)
    opts = {"operator": operator, "mask_lambda": 1, "consensus_k": 3, "consensus_lambda": 0.7, "consensus_normalize": 0}
    want = {"mask_lambda": 1.0, "consensus_k": 3, "consensus_lambda": 0.7, "consensus_normalize": 0.0}
    if ties:
        opts["density"], want["density"] = 1, 1.0
    cfg = MergeConfig.from_yaml(yaml_config(tmp_path, opts))
    assert cfg.merge_options == want and type(cfg.merge_options["consensus_k"]) is int
    m = cls(config=cfg, index_manager=object())
    assert (m.mask_lambda, int(m.consensus_k), m.consensus_lambda, bool(m.consensus_normalize)) == (1.0, 3, 0.7, False)
    readme = m.get_readme()
    for word in ("# Consensus Merged Model", operator + ":", "mask_lambda 1", "consensus_k 3", "lambda 0.7", "plain sum", "org/ft1",
                 "density 1" if ties else "task arithmetic"):
        assert word in readme, (word, readme)
    readme = cls(config=MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": operator})), index_manager=object()).get_readme()
    assert ("agreeing weights" if ties else "sum of the weights") in readme and ("density" in readme) is ties, readme
    for edge in ({"mask_lambda": 0}, {"mask_lambda": 1e6}, {"consensus_k": 1}, {"consensus_k": 16}):
        assert MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": operator, **edge})).merge_options == \
            {k: (v if k == "consensus_k" else float(v)) for k, v in edge.items()}
    # the one method both paths call is what differs; the routing is FourierMerge's
    assert cls.merge_block is not TiesMerge.merge_block and cls._merge_layer is FourierMerge._merge_layer
    assert m.tensor_passes(3) == (17 if ties else 5)


@pytest.mark.parametrize("operator", OPERATORS)
@pytest.mark.parametrize("options", [{"mask_lambda": -0.1}, {"mask_lambda": 1.1e6}, {"mask_lambda": "0.4"}, {"mask_lambda": True},
                                     {"mask_lambda": float("nan")},
                                     {"consensus_k": 0}, {"consensus_k": 17}, {"consensus_k": 2.0}, {"consensus_k": 2.5}, {"consensus_k": "2"},
                                     {"consensus_k": True}, {"consensus_k": -1},
                                     {"consensus_lambda": 1e7}, {"consensus_lambda": -1e7}, {"consensus_lambda": "x"},
                                     {"consensus_normalize": 2}, {"consensus_normalize": 0.5}, {"consensus_normalize": -1},
                                     {"consensus_normalize": "yes"}], ids=str)
def test_yaml_rejects_out_of_range_values(tmp_path, operator, options):
    (key, _), = options.items()
    with pytest.raises(click.BadParameter, match=key):
        MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": operator, **options}))


@pytest.mark.parametrize("value", [0, -0.1, 1.0001, "0.2", True])
def test_yaml_rejects_an_out_of_range_density(tmp_path, value):
    with pytest.raises(click.BadParameter, match="density"):
        MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": "consensus_ties", "density": value}))


def test_yaml_rejects_density_with_consensus_ta(tmp_path):
    with pytest.raises(click.BadParameter, match=r"merge_options\.density is accepted only with operator: consensus_ties"):
        MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": "consensus_ta", "density": 0.2}))


@pytest.mark.parametrize("operator", [None, "fourier", "addition", "task_addition", "fourier_legacy", "ties", "dare_ties", "dare_linear",
                                      "breadcrumbs", "breadcrumbs_ties", "model_stock", "nuslerp", "slerp", "sce", "della", "della_linear"])
@pytest.mark.parametrize("key", ["mask_lambda", "consensus_k", "consensus_lambda", "consensus_normalize"])
def test_yaml_rejects_a_consensus_key_with_another_operator(tmp_path, operator, key):
    opts = {key: 1}
    if operator:
        opts["operator"] = operator
    with pytest.raises(click.BadParameter, match=rf"merge_options\.{key} is accepted only with operator: consensus_ta or consensus_ties"):
        MergeConfig.from_yaml(yaml_config(tmp_path, opts))


@pytest.mark.parametrize("operator", OPERATORS)
@pytest.mark.parametrize("key,value", [("cutoff_pct", 0.08), ("cull_start_pct", 0.2), ("t_sum", 1.0), ("target_norm_offset", 1e-10),
                                       ("b", 0.1), ("norm_mode", "exact"), ("task_add_models", ["org/ft1"]), ("ties_lambda", 1.0),
                                       ("ties_normalize", 1), ("dare_lambda", 1.0), ("dare_normalize", 1), ("dare_rescale", 1),
                                       ("seed", 0), ("gamma", 0.01), ("breadcrumbs_lambda", 1.0), ("breadcrumbs_normalize", 1),
                                       ("stock_filter_wise", 1), ("select_topk", 0.5), ("sce_lambda", 1.0), ("epsilon", 0.1),
                                       ("della_lambda", 1.0), ("della_normalize", 1), ("della_rescale", 1), ("bogus", 1)])
def test_yaml_rejects_an_option_consensus_would_ignore(tmp_path, operator, key, value):
    """the message names the rejected key itself and the operator that would ignore it"""
    named = r"unknown keys \['bogus'\]" if key == "bogus" else rf"merge_options\.{key}\b.*operator '{operator}'"
    with pytest.raises(click.BadParameter, match=named):
        MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": operator, key: value}))


def test_config_stamp(tmp_path):
    stamp = lambda opts: distributed.config_stamp(MergeConfig.from_yaml(yaml_config(tmp_path, opts)))
    full = {"operator": "consensus_ties", "density": 0.2, "mask_lambda": 0.4, "consensus_k": 2, "consensus_lambda": 1.0,
            "consensus_normalize": 1}
    base = stamp(full)
    assert base == stamp(dict(full))
    ta = {k: v for k, v in full.items() if k != "density"}
    others = [stamp({**ta, "operator": "consensus_ta"}), stamp({**full, "density": 0.3}), stamp({**full, "mask_lambda": 0.5}),
              stamp({**full, "consensus_k": 3}), stamp({**full, "consensus_lambda": 0.9}), stamp({**full, "consensus_normalize": 0}),
              stamp({"operator": "ties", "density": 0.2}), stamp({"operator": "dare_linear", "density": 0.2}), stamp(None)]
    assert len({base, *others}) == len(others) + 1


# ---- the CLI end to end ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("operator", OPERATORS)
def test_cli_equals_the_oracle_tensor_by_tensor(tmp_path, emul, operator):
    base, factors, full = lf.setup_k3(tmp_path, emul)
    opts = cc.options(operator)
    expected = cc.expected_outputs(base, full, opts)
    assert any(not torch.equal(expected[n], base[n]) for n in expected if "layers" in n)
    res = run_cli(cc.write_config(tmp_path, "org/lora_full", "merged", opts))
    assert res.exit_code == 0, res.output
    assert_outputs(tmp_path / "merged", expected)
    readme = (tmp_path / "merged" / "README.md").read_text()
    for word in ("# Consensus Merged Model", operator + ":", "mask_lambda 0.6", "consensus_k 2", "lambda 0.7"):
        assert word in readme, (word, readme)
    # one finetune given as a LoRA adapter directory: the run on its materialised checkpoint
    res = run_cli(cc.write_config(tmp_path, "org/lora", "merged_adapter", opts))
    assert res.exit_code == 0, res.output
    lf.assert_same_outputs(tmp_path / "merged_adapter", tmp_path / "merged")
    # the default options
    res = run_cli(cc.write_config(tmp_path, "org/lora_full", "merged_default", {"operator": operator}))
    assert res.exit_code == 0, res.output
    assert_outputs(tmp_path / "merged_default", cc.expected_outputs(base, full, {"operator": operator}))
    # the consensus shows in the output: consensus_k 1 is another model
    res = run_cli(cc.write_config(tmp_path, "org/lora_full", "merged_k1", {**opts, "consensus_k": 1}))
    assert res.exit_code == 0, res.output
    other = lf.read_outputs(tmp_path / "merged_k1")
    assert any(not torch.equal(other[n], expected[n]) for n in expected if "layers" in n)
    assert_outputs(tmp_path / "merged_k1", cc.expected_outputs(base, full, {**opts, "consensus_k": 1}))


@pytest.mark.parametrize("operator", OPERATORS)
def test_cli_in_place_equals_the_oracle(tmp_path, emul, monkeypatch, operator):
    """the partitioned path merges block tensors itself (distributed._merge_block_tensor): it must run Consensus too"""
    monkeypatch.setenv("SHARDMERGE_INPLACE", "1")
    monkeypatch.setattr(distributed, "ENGINE_FACTORY", lambda: emul)
    base, factors, full = lf.setup_k3(tmp_path, emul)
    opts = cc.options(operator)
    res = run_cli(cc.write_config(tmp_path, "org/lora", "merged", opts))
    assert res.exit_code == 0, res.output
    assert_outputs(tmp_path / "merged", cc.expected_outputs(base, full, opts))
    assert "Consensus" in (tmp_path / "merged" / "README.md").read_text()


@pytest.mark.parametrize("operator", OPERATORS)
def test_two_gloo_ranks_equal_the_oracle(tmp_path, emul, operator):
    base, factors, full = lf.setup_k3(tmp_path, emul)
    opts = cc.options(operator)
    cfg = cc.write_config(tmp_path, "org/lora", "merged", opts, device="cpu")
    run_ranks(cfg)
    assert not list((tmp_path / "merged").glob(".tmp-*"))
    assert_outputs(tmp_path / "merged", cc.expected_outputs(base, full, opts))
