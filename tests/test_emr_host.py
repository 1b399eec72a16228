"""operator: emr, `emr-task` and EMR packs without a GPU: the kernels of csrc/sm_emr.hpp on the CPU work-group emulator
against tests/emr_oracle.py (bit for bit, tests/emr_checks.py), the identities with the existing operators, the paper's
form in torch fp64, the YAML options, the stamp, and `python -m shard merge` / `emr-task` end to end - single process, in
place, and two gloo ranks - with the emulator as the device."""
import click
import pytest
import torch

from shardmerge_amd import distributed
from shardmerge_amd.config import EMR_OPERATORS, OPERATORS, MergeConfig
from tests import emr_checks as ec
from tests import lora_fixtures as lf
from tests.harness import DTYPES, KS, assert_outputs, emul, make_inputs, run_cli, run_ranks, write_config, yaml_config  # noqa: F401


# ---- emr_merge on the emulator against the oracle ---------------------------------------------------------------------
@pytest.mark.parametrize("lam", ec.LAMBDAS)
@pytest.mark.parametrize("own", [False, True], ids=["shared", "own"])
@pytest.mark.parametrize("k", KS)
def test_k_bases_and_lambda(emul, k, own, lam):
    ec.check_k(emul, k, own, lam)


@pytest.mark.parametrize("n", ec.SIZES)
def test_sizes(emul, n):
    ec.check_size(emul, n)


@pytest.mark.parametrize("bo_dtype", DTYPES, ids=str)
@pytest.mark.parametrize("in_dtype", DTYPES, ids=str)
def test_dtypes(emul, in_dtype, bo_dtype):
    ec.check_dtypes(emul, in_dtype, bo_dtype)


@pytest.mark.parametrize("check", ec.MERGE_CORNERS, ids=lambda f: f.__name__[len("check_"):])
def test_merge_corner(emul, check):
    check(emul)


# ---- emr_mask / emr_apply on the emulator against the oracle ---------------------------------------------------------------
@pytest.mark.parametrize("cols", ec.COLS)
def test_mask_cols(emul, cols):
    ec.check_cols(emul, cols)


@pytest.mark.parametrize("rows", ec.ROWS)
def test_mask_rows(emul, rows):
    ec.check_rows(emul, rows)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_mask_dtypes(emul, dtype):
    ec.check_mask_dtypes(emul, dtype)


@pytest.mark.parametrize("check", ec.MASK_CORNERS, ids=lambda f: f.__name__[len("check_"):])
def test_mask_corner(emul, check):
    check(emul)


def test_profile_names_and_launches(emul):
    ec.check_profile(emul)


def test_c_abi_rejects_bad_arguments(emul):
    ec.check_c_abi(emul)


# ---- independent of the oracle ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [2, 3, 5])
def test_the_papers_form_in_fp64(emul, k):
    ec.check_paper_form(emul, k)


# ---- YAML ---------------------------------------------------------------------------------------------------------------
def test_yaml_accepts_the_operator_and_its_key(tmp_path):
    from shardmerge_amd.merge import operator_class
    from shardmerge_amd.merge.emr import EmrMerge
    from shardmerge_amd.merge.fast_fourier import FourierMerge
    from shardmerge_amd.merge.ties import TiesMerge
    cls = operator_class("emr")
    assert cls is EmrMerge and issubclass(cls, TiesMerge) and "emr" in OPERATORS and EMR_OPERATORS == ("emr",)
    cfg = MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": "emr"}))
    assert cfg.operator == "emr" and cfg.merge_options == {}
    m = cls(config=cfg, index_manager=object())
    assert m.emr_lambda == 1.0
    cfg = MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": "emr", "emr_lambda": -1}))
    assert cfg.merge_options == {"emr_lambda": -1.0}
    m = cls(config=cfg, index_manager=object())
    readme = m.get_readme()
    for word in ("# EMR Merged Model", "EMR-Merging", "lambda -1", "no weights", "org/ft1"):
        assert word in readme, (word, readme)
    assert cls.merge_block is not TiesMerge.merge_block and cls._merge_layer is FourierMerge._merge_layer
    assert [m.tensor_passes(k) for k in (1, 3, 16)] == [3, 5, 18]
    overridden = {n for n in vars(cls) if not n.startswith("__") and n != "_abc_impl"}
    assert overridden == {"option_defaults", "get_readme", "merge_block", "tensor_passes", "_log_block"}, overridden


@pytest.mark.parametrize("value", [1e7, -1e7, float("nan"), "1", True, None])
def test_yaml_rejects_an_out_of_range_lambda(tmp_path, value):
    with pytest.raises(click.BadParameter, match=r"merge_options\.emr_lambda must be a number in \[-1000000\.0, 1000000\.0\]"):
        MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": "emr", "emr_lambda": value}))


@pytest.mark.parametrize("operator", [None] + [op for op in OPERATORS if op != "emr"])
def test_yaml_rejects_emr_lambda_with_another_operator(tmp_path, operator):
    opts = {"emr_lambda": 1}
    if operator:
        opts["operator"] = operator
    shown = operator or "fourier"
    with pytest.raises(click.BadParameter, match=rf"merge_options\.emr_lambda is accepted only with operator: emr \(operator '{shown}' would ignore it\)"):
        MergeConfig.from_yaml(yaml_config(tmp_path, opts))


@pytest.mark.parametrize("key,value", [("cutoff_pct", 0.08), ("cull_start_pct", 0.2), ("t_sum", 1.0), ("target_norm_offset", 1e-10),
                                       ("b", 0.1), ("norm_mode", "exact"), ("task_add_models", ["org/ft1"]), ("density", 0.2),
                                       ("ties_lambda", 1.0), ("ties_normalize", 1), ("dare_lambda", 1.0), ("dare_rescale", 1), ("seed", 1),
                                       ("gamma", 0.01), ("breadcrumbs_lambda", 1.0), ("stock_filter_wise", 1),
                                       ("select_topk", 0.5), ("sce_lambda", 1.0), ("epsilon", 0.1), ("della_lambda", 1.0),
                                       ("mask_lambda", 0.4), ("consensus_k", 2), ("karcher_max_iter", 10), ("karcher_tol", 1e-5),
                                       ("sphere_row_wise", 1), ("fusion_iqr", 1.5), ("nearswap_t", 0.001), ("pcb_ratio", 0.1),
                                       ("pcb_clip", 0.01), ("pcb_lambda", 1.0), ("tsv_rank", 8), ("tsv_power_iters", 1), ("tsv_lambda", 1.0),
                                       ("widen_ratio", 1.0), ("widen_calibration", 1.0), ("widen_lambda", 1.0), ("cabs_n", 8), ("cabs_m", 32),
                                       ("cabs_conflict_aware", 1), ("cabs_lambda", 1.0), ("iso_lambda", 1.0), ("iso_tol", 1e-4),
                                       ("iso_max_iter", 40), ("bogus", 1)])
def test_yaml_rejects_an_option_emr_would_ignore(tmp_path, key, value):
    """the message names the rejected key itself and the operator that would ignore it"""
    named = r"unknown keys \['bogus'\]" if key == "bogus" else rf"merge_options\.{key}\b.*operator 'emr'"
    with pytest.raises(click.BadParameter, match=named):
        MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": "emr", key: value}))


@pytest.mark.parametrize("alpha", [0.5, 0, -1, 2, True, "1"])
def test_yaml_rejects_an_alpha(tmp_path, alpha):
    models = [{"model": "org/ft1", "base": "org/base"}, {"model": "org/ft2", "base": "org/base", "alpha": alpha}]
    with pytest.raises(click.BadParameter, match=r"operator emr takes no weight: finetune_merge alpha of org/ft2 must be 1"):
        MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": "emr"}, models))
    models[1]["alpha"] = 1
    assert MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": "emr"}, models)).finetune_merge[1].alpha == 1


def test_config_stamp(tmp_path):
    stamp = lambda opts: distributed.config_stamp(MergeConfig.from_yaml(yaml_config(tmp_path, opts)))
    base = stamp({"operator": "emr", "emr_lambda": 1.0})
    assert base == stamp({"operator": "emr", "emr_lambda": 1.0})
    others = [stamp({"operator": "emr", "emr_lambda": 0.5}), stamp({"operator": "dare_linear", "density": 1.0}), stamp({"operator": "ties"}), stamp(None)]
    assert len({base, *others}) == len(others) + 1


# ---- end to end on the on-disk model --------------------------------------------------------------------------------------
def test_merge_task_and_pack_end_to_end(tmp_path, emul):
    ec.check_end_to_end(tmp_path, emul, "cpu")


def test_scale_per_tensor_and_full(tmp_path, emul):
    ec.check_forms(tmp_path, emul, "cpu")


def test_layer_windows_and_own_bases(tmp_path, emul):
    """layer 0: three entries, one against its own base; layer 1: two; one of them a LoRA adapter directory"""
    from tests import emr_oracle as eo
    from tests.harness import expected_by_tensor, ties_models
    base, factors, full = lf.setup_k3(tmp_path, emul)
    models = [{k: v for k, v in m.items() if k != "alpha"} for m in ties_models("org/lora_full")]
    opts = {"operator": "emr", "emr_lambda": 0.5}
    expected = expected_by_tensor(base, full, models, lambda fts, bases, alphas, bo, name: eo.emr_merge(fts, bases, bo, lam=0.5)["out"])
    res = run_cli(write_config(tmp_path, models, "merged", opts))
    assert res.exit_code == 0, res.output
    assert_outputs(tmp_path / "merged", expected)
    models[2]["model"] = "org/lora"
    res = run_cli(write_config(tmp_path, models, "merged_adapter", opts))
    assert res.exit_code == 0, res.output
    lf.assert_same_outputs(tmp_path / "merged_adapter", tmp_path / "merged")


def test_in_place_equals_the_oracle(tmp_path, emul, monkeypatch):
    """the partitioned path merges block tensors itself (distributed._merge_block_tensor): it must run emr and take a pack"""
    base, uni = ec.setup_unified(tmp_path, emul, "cpu")
    assert ec.run_cli(ec.task_args(tmp_path, "org/ft1", "org/task", "cpu")).exit_code == 0
    monkeypatch.setenv("SHARDMERGE_INPLACE", "1")
    monkeypatch.setattr(distributed, "ENGINE_FACTORY", lambda: emul)
    res = run_cli(write_config(tmp_path, ec.emr_models(), "inplace", ec.OPTIONS))
    assert res.exit_code == 0, res.output
    assert_outputs(tmp_path / "inplace", uni)
    want = ec.oracle_task(base, lf.model_tensors(1), uni)[0]
    res = run_cli(write_config(tmp_path, ec.pack_entry("org/task"), "inplace_task", ec.ONE_ENTRY))
    assert res.exit_code == 0, res.output
    assert_outputs(tmp_path / "inplace_task", want)


def test_two_gloo_ranks_equal_the_oracle(tmp_path, emul):
    base, uni = ec.setup_unified(tmp_path, emul, "cpu")
    assert ec.run_cli(ec.task_args(tmp_path, "org/ft2", "org/task", "cpu")).exit_code == 0
    run_ranks(write_config(tmp_path, ec.emr_models(), "ranks", ec.OPTIONS, device="cpu"))
    assert not list((tmp_path / "ranks").glob(".tmp-*"))
    assert_outputs(tmp_path / "ranks", uni)
    run_ranks(write_config(tmp_path, ec.pack_entry("org/task"), "ranks_task", ec.ONE_ENTRY, device="cpu"))
    assert_outputs(tmp_path / "ranks_task", ec.oracle_task(base, lf.model_tensors(2), uni)[0])


def test_the_stamp_changes_with_the_pack(tmp_path, emul):
    ec.check_stamp(tmp_path, emul, "cpu")


def test_reader_rejections(tmp_path, emul):
    ec.check_reader_rejections(tmp_path, emul, "cpu")


def test_command_rejections(tmp_path, emul, monkeypatch):
    ec.check_command_rejections(tmp_path, emul, "cpu", monkeypatch)
