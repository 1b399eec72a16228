"""operator: cabs without a GPU: the kernel of csrc/sm_cabs.hpp on the CPU work-group emulator against tests/cabs_oracle.py
(bit for bit, tests/cabs_checks.py), the paper's form in torch, the YAML options, the stamp, and `python -m shard merge` /
`analyze` end to end - single process, in place, and two gloo ranks - with the emulator as the device."""
import click
import pytest
import torch
import yaml
from click.testing import CliRunner

from shardmerge_amd import distributed
from shardmerge_amd.config import CABS_OPERATORS, OPERATORS, MergeConfig
from tests import cabs_checks as cc
from tests import lora_fixtures as lf
from tests.harness import DTYPES, assert_outputs, emul, run_cli, run_ranks, ties_models, yaml_config  # noqa: F401

KEYS = ["cabs_n", "cabs_m", "cabs_conflict_aware", "cabs_lambda"]
TAIL_COLS = 600                                 # the option grid's row length on the emulator: a tail group at every M


# ---- the kernel on the emulator against the oracle ----------------------------------------------------------
@pytest.mark.parametrize("C", cc.COLS)
def test_cols(emul, C):
    cc.check_cols(emul, C)


@pytest.mark.parametrize("conflict_aware", [True, False], ids=["ca", "independent"])
@pytest.mark.parametrize("M", cc.GROUPS)
def test_options(emul, M, conflict_aware):
    cc.check_options(emul, M, conflict_aware, TAIL_COLS)


@pytest.mark.parametrize("own", [False, True], ids=["shared_base", "own_bases"])
@pytest.mark.parametrize("k", cc.KS)
def test_k(emul, k, own):
    cc.check_k(emul, k, own)


@pytest.mark.parametrize("bo_dtype", DTYPES, ids=str)
@pytest.mark.parametrize("in_dtype", DTYPES, ids=str)
def test_dtypes(emul, in_dtype, bo_dtype):
    cc.check_dtypes(emul, in_dtype, bo_dtype)


@pytest.mark.parametrize("check", cc.CORNERS, ids=lambda f: f.__name__[len("check_"):])
def test_corner(emul, check):
    check(emul)


def test_largest_emulator_shape(emul):
    """2^16 + 5 elements in rows of no multiple of 8: every team of 32 lanes, several tiles per work-group"""
    fts, bases, bo = cc.make_inputs((1, 2 ** 16 + 5), 3, seed=5, own_bases=True)
    cc.check(emul, fts, bases, cc.ALPHAS[:3], bo, 64, 256, lam=0.7, label="1 x 65541")


def test_paper_form_in_torch(emul):
    """the GPU tier runs the three cases of the issue; here a slice of them that the emulator takes in seconds"""
    cc.check_paper_form(emul, (64, 1024), 2, 64, 256)
    cc.check_paper_form(emul, (12, 4544), 3, 128, 512)


@pytest.mark.parametrize("k,expected", cc.PROFILES, ids=[f"k{k}" for k, _ in cc.PROFILES])
def test_profile_names(emul, k, expected):
    cc.check_profile(emul, k, expected)


def test_c_abi_rejects_bad_arguments(emul):
    cc.check_c_abi(emul)


# ---- YAML ------------------------------------------------------------------------------------------------------
def test_yaml_accepts_the_operator_and_its_keys(tmp_path):
    from shardmerge_amd.merge import operator_class
    from shardmerge_amd.merge.cabs import CabsMerge
    from shardmerge_amd.merge.fast_fourier import FourierMerge
    from shardmerge_amd.merge.ties import TiesMerge
    cls = operator_class("cabs")
    assert cls is CabsMerge and issubclass(cls, TiesMerge) and "cabs" in OPERATORS and CABS_OPERATORS == ("cabs",)
    cfg = MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": "cabs"}))
    assert cfg.operator == "cabs" and cfg.merge_options == {}
    m = cls(config=cfg, index_manager=object())
    assert (m.cabs_n, m.cabs_m, bool(m.cabs_conflict_aware), m.cabs_lambda) == (64, 256, True, 1.0)
    cfg = MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": "cabs", "cabs_n": 2, "cabs_m": 4, "cabs_conflict_aware": 0, "cabs_lambda": 0.7}))
    assert cfg.merge_options == {"cabs_n": 2, "cabs_m": 4, "cabs_conflict_aware": 0.0, "cabs_lambda": 0.7}
    assert type(cfg.merge_options["cabs_n"]) is int and type(cfg.merge_options["cabs_m"]) is int
    m = cls(config=cfg, index_manager=object())
    readme = m.get_readme()
    for word in ("# CABS Merged Model", "CABS (", "2:4", "conflict-aware off", "lambda 0.7", "entry order: org/ft1", "org/ft1 (vs org/base"):
        assert word in readme, (word, readme)
    models = [{"model": "org/ft2", "base": "org/base"}, {"model": "org/ft1", "base": "org/base"}]
    readme = cls(config=MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": "cabs"}, models)), index_manager=object()).get_readme()
    for word in ("64:256", "conflict-aware: ", "order is part of the result", "entry order: org/ft2 > org/ft1"):
        assert word in readme, (word, readme)
    for edge in ({"cabs_n": 1}, {"cabs_n": 256}, {"cabs_m": 64}, {"cabs_m": 512}, {"cabs_n": 512, "cabs_m": 512}, {"cabs_n": 4, "cabs_m": 4},
                 {"cabs_lambda": -1e6}, {"cabs_lambda": 1e6}):
        assert MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": "cabs", **edge})).merge_options == \
            {k: (v if k in ("cabs_n", "cabs_m") else float(v)) for k, v in edge.items()}
    assert cls.merge_block is not TiesMerge.merge_block and cls._merge_layer is FourierMerge._merge_layer
    assert [m.tensor_passes(k) for k in (1, 2, 3)] == [3, 4, 5]


@pytest.mark.parametrize("options,key", [
    ({"cabs_m": 0}, "cabs_m"), ({"cabs_m": 2}, "cabs_m"), ({"cabs_m": 48}, "cabs_m"), ({"cabs_m": 1024}, "cabs_m"), ({"cabs_m": 64.0}, "cabs_m"),
    ({"cabs_m": "64"}, "cabs_m"), ({"cabs_m": True}, "cabs_m"), ({"cabs_m": -64}, "cabs_m"), ({"cabs_m": 100, "cabs_n": 10}, "cabs_m"),
    ({"cabs_n": 0}, "cabs_n"), ({"cabs_n": 257}, "cabs_n"), ({"cabs_n": 64.0}, "cabs_n"), ({"cabs_n": "1"}, "cabs_n"), ({"cabs_n": True}, "cabs_n"),
    ({"cabs_n": -1}, "cabs_n"), ({"cabs_n": 9, "cabs_m": 8}, "cabs_n"), ({"cabs_m": 32}, "cabs_n"), ({"cabs_n": 513, "cabs_m": 512}, "cabs_n"),
    ({"cabs_conflict_aware": 2}, "cabs_conflict_aware"), ({"cabs_conflict_aware": 0.5}, "cabs_conflict_aware"),
    ({"cabs_conflict_aware": "yes"}, "cabs_conflict_aware"), ({"cabs_conflict_aware": -1}, "cabs_conflict_aware"),
    ({"cabs_lambda": 1e7}, "cabs_lambda"), ({"cabs_lambda": "x"}, "cabs_lambda"), ({"cabs_lambda": float("inf")}, "cabs_lambda"),
    ({"cabs_lambda": float("nan")}, "cabs_lambda")], ids=str)
def test_yaml_rejects_out_of_range_values(tmp_path, options, key):
    """when the config is loaded, naming the key ({"cabs_m": 32}: the default cabs_n = 64 no longer fits)"""
    with pytest.raises(click.BadParameter, match=rf"merge_options\.{key}\b"):
        MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": "cabs", **options}))


@pytest.mark.parametrize("operator", [None] + [op for op in OPERATORS if op != "cabs"])
@pytest.mark.parametrize("key", KEYS)
def test_yaml_rejects_a_cabs_key_with_another_operator(tmp_path, operator, key):
    opts = {key: 1}
    if operator:
        opts["operator"] = operator
    shown = operator or "fourier"
    with pytest.raises(click.BadParameter, match=rf"merge_options\.{key} is accepted only with operator: cabs \(operator '{shown}' would ignore it\)"):
        MergeConfig.from_yaml(yaml_config(tmp_path, opts))


@pytest.mark.parametrize("key,value", [("cutoff_pct", 0.08), ("cull_start_pct", 0.2), ("t_sum", 1.0), ("target_norm_offset", 1e-10),
                                       ("b", 0.1), ("norm_mode", "exact"), ("task_add_models", ["org/ft1"]), ("density", 0.2),
                                       ("ties_lambda", 1.0), ("ties_normalize", 1), ("dare_lambda", 1.0), ("dare_rescale", 1),
                                       ("seed", 0), ("gamma", 0.01), ("breadcrumbs_lambda", 1.0), ("stock_filter_wise", 1),
                                       ("select_topk", 0.5), ("sce_lambda", 1.0), ("epsilon", 0.1), ("della_lambda", 1.0),
                                       ("mask_lambda", 0.4), ("consensus_k", 2), ("karcher_max_iter", 10), ("karcher_tol", 1e-5),
                                       ("sphere_row_wise", 1), ("fusion_iqr", 1.5), ("nearswap_t", 0.001), ("pcb_ratio", 0.1),
                                       ("pcb_clip", 0.0001), ("pcb_lambda", 1.0), ("tsv_rank", 64), ("tsv_power_iters", 2),
                                       ("tsv_lambda", 1.0), ("widen_ratio", 1.0), ("widen_calibration", 1.0), ("widen_lambda", 1.0),
                                       ("bogus", 1)])
def test_yaml_rejects_an_option_cabs_would_ignore(tmp_path, key, value):
    """the message names the rejected key itself and the operator that would ignore it"""
    named = r"unknown keys \['bogus'\]" if key == "bogus" else rf"merge_options\.{key}\b.*operator 'cabs'"
    with pytest.raises(click.BadParameter, match=named):
        MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": "cabs", key: value}))


def test_a_zero_alpha_sum_is_no_error(tmp_path):
    doc = yaml.safe_load(yaml_config(tmp_path, {"operator": "cabs"}).read_text())
    doc["finetune_merge"] = [{"model": "org/ft1", "base": "org/base", "alpha": 0.5}, {"model": "org/ft2", "base": "org/base", "alpha": -0.5}]
    (tmp_path / "cfg.yaml").write_text(yaml.safe_dump(doc))
    assert [m.alpha for m in MergeConfig.from_yaml(tmp_path / "cfg.yaml").finetune_merge] == [0.5, -0.5]


def test_config_stamp(tmp_path):
    stamp = lambda opts: distributed.config_stamp(MergeConfig.from_yaml(yaml_config(tmp_path, opts)))
    full = {"operator": "cabs", "cabs_n": 64, "cabs_m": 256, "cabs_conflict_aware": 1, "cabs_lambda": 1.0}
    base = stamp(full)
    assert base == stamp(dict(full))
    others = [stamp({**full, "cabs_n": 32}), stamp({**full, "cabs_m": 512}), stamp({**full, "cabs_conflict_aware": 0}),
              stamp({**full, "cabs_lambda": 0.9}), stamp({"operator": "ties", "density": 0.25}), stamp({"operator": "widen"}), stamp(None)]
    assert len({base, *others}) == len(others) + 1


# ---- the CLI end to end ------------------------------------------------------------------------------------------
def test_cli_equals_the_oracle_tensor_by_tensor(tmp_path, emul):
    base, factors, full = lf.setup_k3(tmp_path, emul)
    opts = cc.OPTIONS
    expected = cc.expected_outputs(base, full, opts)
    assert any(not torch.equal(expected[n], base[n]) for n in expected if "layers" in n)
    res = run_cli(cc.write_config(tmp_path, "org/lora_full", "merged", opts))
    assert res.exit_code == 0, res.output
    assert_outputs(tmp_path / "merged", expected)           # (passthrough tensors included: torch.equal)
    readme = (tmp_path / "merged" / "README.md").read_text()
    for word in ("# CABS Merged Model", "CABS (", "8:32", "conflict-aware: ", "lambda 0.7", "entry order: org/ft1 > org/ft2 > org/lora_full"):
        assert word in readme, (word, readme)
    # one finetune given as a LoRA adapter directory: the run on its materialised checkpoint
    res = run_cli(cc.write_config(tmp_path, "org/lora", "merged_adapter", opts))
    assert res.exit_code == 0, res.output
    lf.assert_same_outputs(tmp_path / "merged_adapter", tmp_path / "merged")
    # the default options
    res = run_cli(cc.write_config(tmp_path, "org/lora_full", "merged_default", {"operator": "cabs"}))
    assert res.exit_code == 0, res.output
    assert_outputs(tmp_path / "merged_default", cc.expected_outputs(base, full, {"operator": "cabs"}))
    # the order of the entries is part of the result: the same entries the other way round give another model
    models = ties_models("org/lora_full")[::-1]
    cfg = yaml.safe_load(cc.write_config(tmp_path, "org/lora_full", "merged_reversed", opts).read_text())
    cfg["finetune_merge"] = models
    path = tmp_path / "reversed.yaml"
    path.write_text(yaml.safe_dump(cfg))
    res = run_cli(path)
    assert res.exit_code == 0, res.output
    other = lf.read_outputs(tmp_path / "merged_reversed")
    assert any(not torch.equal(other[n], expected[n]) for n in expected if "layers.0" in n)
    assert_outputs(tmp_path / "merged_reversed", cc.expected_outputs(base, full, opts, models=models))
    # analyze keeps accepting the config: the operator's options are validated and not used
    from shardmerge_amd.__main__ import cli
    res = CliRunner().invoke(cli, ["analyze", str(cc.write_config(tmp_path, "org/lora_full", "analysed", opts))])
    assert res.exit_code == 0, res.output


def test_cli_a_window_that_leaves_one_entry(tmp_path, emul):
    """layer 1 is covered by the third entry alone: the function at k = 1"""
    base, factors, full = lf.setup_k3(tmp_path, emul)
    models = ties_models("org/lora_full")
    models[0]["end_layer"] = 0
    cfg = yaml.safe_load(cc.write_config(tmp_path, "org/lora_full", "merged", cc.OPTIONS).read_text())
    cfg["finetune_merge"] = models
    path = tmp_path / "one_entry.yaml"
    path.write_text(yaml.safe_dump(cfg))
    res = run_cli(path)
    assert res.exit_code == 0, res.output
    assert_outputs(tmp_path / "merged", cc.expected_outputs(base, full, cc.OPTIONS, models=models))


def test_cli_in_place_equals_the_oracle(tmp_path, emul, monkeypatch):
    """the partitioned path merges block tensors itself (distributed._merge_block_tensor): it must run CABS too"""
    monkeypatch.setenv("SHARDMERGE_INPLACE", "1")
    monkeypatch.setattr(distributed, "ENGINE_FACTORY", lambda: emul)
    base, factors, full = lf.setup_k3(tmp_path, emul)
    res = run_cli(cc.write_config(tmp_path, "org/lora", "merged", cc.OPTIONS))
    assert res.exit_code == 0, res.output
    assert_outputs(tmp_path / "merged", cc.expected_outputs(base, full, cc.OPTIONS))
    readme = (tmp_path / "merged" / "README.md").read_text()
    assert "CABS" in readme and "8:32" in readme and "entry order: org/ft1 > org/ft2 > org/lora" in readme


def test_two_gloo_ranks_equal_the_oracle(tmp_path, emul):
    base, factors, full = lf.setup_k3(tmp_path, emul)
    cfg = cc.write_config(tmp_path, "org/lora", "merged", cc.OPTIONS, device="cpu")
    run_ranks(cfg)
    assert not list((tmp_path / "merged").glob(".tmp-*"))
    assert_outputs(tmp_path / "merged", cc.expected_outputs(base, full, cc.OPTIONS))
