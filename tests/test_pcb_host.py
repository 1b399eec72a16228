"""operator: pcb without a GPU: the kernels of csrc/sm_pcb.hpp (and the selection kernels of the task-vector statistics)
on the CPU work-group emulator against tests/pcb_oracle.py (bit for bit, tests/pcb_checks.py), sm_tanh against mpmath,
the function against a torch fp64 restatement of the paper's form, the YAML options, the stamp, and
`python -m shard merge` / `analyze` end to end - single process, in place, and two gloo ranks - with the emulator as the
device."""
import click
import pytest
import torch
import yaml
from click.testing import CliRunner

from shardmerge_amd import distributed
from shardmerge_amd.config import OPERATORS, MergeConfig
from tests import lora_fixtures as lf
from tests import pcb_checks as pc
from tests.harness import DTYPES, assert_outputs, emul, run_cli, run_ranks, ties_models, yaml_config  # noqa: F401


# ---- the kernels on the emulator against the oracle ---------------------------------------------------------
@pytest.mark.parametrize("bo_dtype", DTYPES, ids=str)
@pytest.mark.parametrize("in_dtype", DTYPES, ids=str)
def test_dtypes(emul, in_dtype, bo_dtype):
    pc.check_dtypes(emul, in_dtype, bo_dtype)


@pytest.mark.parametrize("own", [False, True], ids=["shared_base", "own_bases"])
@pytest.mark.parametrize("k", pc.KS)
def test_k(emul, k, own):
    pc.check_k(emul, k, own)


@pytest.mark.parametrize("lam", pc.LAMBDAS)
@pytest.mark.parametrize("clip", pc.CLIPS)
@pytest.mark.parametrize("ratio", pc.RATIOS)
def test_options(emul, ratio, clip, lam):
    pc.check_options(emul, ratio, clip, lam)


@pytest.mark.parametrize("n", pc.SIZES)
def test_sizes(emul, n):
    pc.check_size(emul, n)


@pytest.mark.parametrize("check", pc.CORNERS, ids=lambda f: f.__name__[len("check_"):])
def test_corner(emul, check):
    check(emul)


@pytest.mark.parametrize("k,expected", pc.PROFILES, ids=pc.PROFILE_IDS)
def test_profile_names_and_launches(emul, k, expected):
    pc.check_profile(emul, k, expected)


def test_c_abi_rejects_bad_arguments(emul):
    pc.check_c_abi(emul)


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "emulated_kernel"])
def test_sm_tanh(emul, on_device):
    pc.check_tanh(emul, on_device)


@pytest.mark.parametrize("k", [2, 3, 5])
@pytest.mark.parametrize("n", [2 ** 16, 2 ** 20])
def test_paper_form_in_fp64(emul, n, k):
    """Measured on the emulator (bf16 deltas of sigma 3e-3 (1 + 0.3 i) on a Gaussian base, ratio 0.1, clip 1e-4): see the
    README's PCB section for the largest error / bound and the counts under the den floor."""
    pc.check_paper_form(emul, n, k)


# ---- YAML ------------------------------------------------------------------------------------------------------
def test_yaml_accepts_the_operator_and_its_keys(tmp_path):
    from shardmerge_amd.merge import operator_class
    from shardmerge_amd.merge.fast_fourier import FourierMerge
    from shardmerge_amd.merge.pcb import PcbMerge
    from shardmerge_amd.merge.ties import TiesMerge
    cls = operator_class("pcb")
    assert cls is PcbMerge and issubclass(cls, TiesMerge) and "pcb" in OPERATORS
    cfg = MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": "pcb"}))
    assert cfg.operator == "pcb" and cfg.merge_options == {}
    m = cls(config=cfg, index_manager=object())
    assert (m.pcb_ratio, m.pcb_clip, m.pcb_lambda) == (0.1, 0.0001, 1.0)
    cfg = MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": "pcb", "pcb_ratio": 1, "pcb_clip": 0, "pcb_lambda": 0.7}))
    assert cfg.merge_options == {"pcb_ratio": 1.0, "pcb_clip": 0.0, "pcb_lambda": 0.7}
    m = cls(config=cfg, index_manager=object())
    readme = m.get_readme()
    for word in ("# PCB Merged Model", "PCB (", "ratio 1", "clip 0", "lambda 0.7", "org/ft1"):
        assert word in readme, (word, readme)
    for edge in ({"pcb_ratio": 1e-9}, {"pcb_ratio": 1.0}, {"pcb_clip": 0}, {"pcb_clip": 0.4999}, {"pcb_lambda": -1e6}, {"pcb_lambda": 1e6}):
        assert MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": "pcb", **edge})).merge_options == {k: float(v) for k, v in edge.items()}
    # the one method both paths call is what differs; the routing is FourierMerge's
    assert cls.merge_block is not TiesMerge.merge_block and cls._merge_layer is FourierMerge._merge_layer
    assert [m.tensor_passes(k) for k in (1, 2, 3)] == [15, 22, 29]


@pytest.mark.parametrize("options,text", [
    ({"pcb_ratio": 0}, r"\(0, 1\]"), ({"pcb_ratio": -0.1}, r"\(0, 1\]"), ({"pcb_ratio": 1.0001}, r"\(0, 1\]"), ({"pcb_ratio": "0.1"}, r"\(0, 1\]"),
    ({"pcb_ratio": True}, r"\(0, 1\]"), ({"pcb_ratio": float("nan")}, r"\(0, 1\]"),
    ({"pcb_clip": -1e-9}, r"\[0, 0\.5\)"), ({"pcb_clip": 0.5}, r"\[0, 0\.5\)"), ({"pcb_clip": 1}, r"\[0, 0\.5\)"), ({"pcb_clip": "x"}, r"\[0, 0\.5\)"),
    ({"pcb_lambda": 1e7}, r"\[-1000000\.0, 1000000\.0\]"), ({"pcb_lambda": -1e7}, r"\[-1000000\.0, 1000000\.0\]"),
    ({"pcb_lambda": "x"}, r"\[-1000000\.0, 1000000\.0\]"), ({"pcb_lambda": float("inf")}, r"\[-1000000\.0, 1000000\.0\]")], ids=str)
def test_yaml_rejects_out_of_range_values(tmp_path, options, text):
    (key, _), = options.items()
    with pytest.raises(click.BadParameter, match=rf"merge_options\.{key} must be a number in {text}"):
        MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": "pcb", **options}))


@pytest.mark.parametrize("operator", [None] + [op for op in OPERATORS if op != "pcb"])
@pytest.mark.parametrize("key", ["pcb_ratio", "pcb_clip", "pcb_lambda"])
def test_yaml_rejects_a_pcb_key_with_another_operator(tmp_path, operator, key):
    opts = {key: 0.1}
    if operator:
        opts["operator"] = operator
    shown = operator or "fourier"
    with pytest.raises(click.BadParameter, match=rf"merge_options\.{key} is accepted only with operator: pcb \(operator '{shown}' would ignore it\)"):
        MergeConfig.from_yaml(yaml_config(tmp_path, opts))


@pytest.mark.parametrize("key,value", [("cutoff_pct", 0.08), ("cull_start_pct", 0.2), ("t_sum", 1.0), ("target_norm_offset", 1e-10),
                                       ("b", 0.1), ("norm_mode", "exact"), ("task_add_models", ["org/ft1"]), ("density", 0.2),
                                       ("ties_lambda", 1.0), ("ties_normalize", 1), ("dare_lambda", 1.0), ("dare_rescale", 1),
                                       ("seed", 0), ("gamma", 0.01), ("breadcrumbs_lambda", 1.0), ("stock_filter_wise", 1),
                                       ("select_topk", 0.5), ("sce_lambda", 1.0), ("epsilon", 0.1), ("della_lambda", 1.0),
                                       ("mask_lambda", 0.4), ("consensus_k", 2), ("karcher_max_iter", 10), ("karcher_tol", 1e-5),
                                       ("sphere_row_wise", 1), ("fusion_iqr", 1.5), ("nearswap_t", 0.001), ("bogus", 1)])
def test_yaml_rejects_an_option_pcb_would_ignore(tmp_path, key, value):
    """the message names the rejected key itself and the operator that would ignore it"""
    named = r"unknown keys \['bogus'\]" if key == "bogus" else rf"merge_options\.{key}\b.*operator 'pcb'"
    with pytest.raises(click.BadParameter, match=named):
        MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": "pcb", key: value}))


def test_yaml_words_the_rejections_as_the_families_do(tmp_path):
    for opts, text in (({"karcher_tol": 1e-5}, r"merge_options\.karcher_tol is accepted only with operator: karcher or multislerp \(operator 'pcb' would ignore it\)"),
                       ({"density": 0.2}, r"merge_options\.density is an option of operator ties; operator 'pcb' would ignore it \(its keys: pcb_ratio, pcb_lambda\)"),
                       ({"seed": 1}, r"merge_options\.seed is an option of operators dare_ties / dare_linear; operator 'pcb' would ignore it \(it drops nothing at random\)"),
                       ({"cutoff_pct": 0.1}, r"merge_options\.cutoff_pct is an option of the spectral operators; operator 'pcb' would ignore it"),
                       ({"norm_mode": "exact"}, r"merge_options\.norm_mode is an option of the spectral operators; operator 'pcb' takes no norm")):
        with pytest.raises(click.BadParameter, match=text):
            MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": "pcb", **opts}))


def test_a_zero_alpha_sum_is_no_error(tmp_path):
    doc = yaml.safe_load(yaml_config(tmp_path, {"operator": "pcb"}).read_text())
    doc["finetune_merge"] = [{"model": "org/ft1", "base": "org/base", "alpha": 0.5}, {"model": "org/ft2", "base": "org/base", "alpha": -0.5}]
    (tmp_path / "cfg.yaml").write_text(yaml.safe_dump(doc))
    assert [m.alpha for m in MergeConfig.from_yaml(tmp_path / "cfg.yaml").finetune_merge] == [0.5, -0.5]


def test_config_stamp(tmp_path):
    stamp = lambda opts: distributed.config_stamp(MergeConfig.from_yaml(yaml_config(tmp_path, opts)))
    full = {"operator": "pcb", "pcb_ratio": 0.1, "pcb_clip": 0.0001, "pcb_lambda": 1.0}
    base = stamp(full)
    assert base == stamp(dict(full))
    others = [stamp({**full, "pcb_ratio": 0.2}), stamp({**full, "pcb_clip": 0.001}), stamp({**full, "pcb_lambda": 0.9}),
              stamp({"operator": "ties", "density": 0.2}), stamp({"operator": "consensus_ta"}), stamp(None)]
    assert len({base, *others}) == len(others) + 1


# ---- the CLI end to end ------------------------------------------------------------------------------------------
def test_cli_equals_the_oracle_tensor_by_tensor(tmp_path, emul):
    base, factors, full = lf.setup_k3(tmp_path, emul)
    opts = pc.OPTIONS
    expected = pc.expected_outputs(base, full, opts)
    assert any(not torch.equal(expected[n], base[n]) for n in expected if "layers" in n)
    res = run_cli(pc.write_config(tmp_path, "org/lora_full", "merged", opts))
    assert res.exit_code == 0, res.output
    assert_outputs(tmp_path / "merged", expected)
    readme = (tmp_path / "merged" / "README.md").read_text()
    for word in ("# PCB Merged Model", "PCB (", "ratio 0.3", "clip 0.01", "lambda 0.7"):
        assert word in readme, (word, readme)
    # one finetune given as a LoRA adapter directory: the run on its materialised checkpoint
    res = run_cli(pc.write_config(tmp_path, "org/lora", "merged_adapter", opts))
    assert res.exit_code == 0, res.output
    lf.assert_same_outputs(tmp_path / "merged_adapter", tmp_path / "merged")
    # the default options
    res = run_cli(pc.write_config(tmp_path, "org/lora_full", "merged_default", {"operator": "pcb"}))
    assert res.exit_code == 0, res.output
    assert_outputs(tmp_path / "merged_default", pc.expected_outputs(base, full, {"operator": "pcb"}))
    # the ratio shows in the output
    res = run_cli(pc.write_config(tmp_path, "org/lora_full", "merged_r1", {**opts, "pcb_ratio": 1.0}))
    assert res.exit_code == 0, res.output
    other = lf.read_outputs(tmp_path / "merged_r1")
    assert any(not torch.equal(other[n], expected[n]) for n in expected if "layers" in n)
    # analyze keeps accepting the config: the operator's options are validated and not used
    from shardmerge_amd.__main__ import cli
    res = CliRunner().invoke(cli, ["analyze", str(pc.write_config(tmp_path, "org/lora_full", "analysed", opts))])
    assert res.exit_code == 0, res.output


def test_cli_a_window_that_leaves_one_entry(tmp_path, emul):
    """layer 1 is covered by the third entry alone: the function at k = 1"""
    base, factors, full = lf.setup_k3(tmp_path, emul)
    models = ties_models("org/lora_full")
    models[0]["end_layer"] = 0
    cfg = yaml.safe_load(pc.write_config(tmp_path, "org/lora_full", "merged", pc.OPTIONS).read_text())
    cfg["finetune_merge"] = models
    path = tmp_path / "one_entry.yaml"
    path.write_text(yaml.safe_dump(cfg))
    res = run_cli(path)
    assert res.exit_code == 0, res.output
    assert_outputs(tmp_path / "merged", pc.expected_outputs(base, full, pc.OPTIONS, models=models))


def test_cli_in_place_equals_the_oracle(tmp_path, emul, monkeypatch):
    """the partitioned path merges block tensors itself (distributed._merge_block_tensor): it must run PCB too"""
    monkeypatch.setenv("SHARDMERGE_INPLACE", "1")
    monkeypatch.setattr(distributed, "ENGINE_FACTORY", lambda: emul)
    base, factors, full = lf.setup_k3(tmp_path, emul)
    res = run_cli(pc.write_config(tmp_path, "org/lora", "merged", pc.OPTIONS))
    assert res.exit_code == 0, res.output
    assert_outputs(tmp_path / "merged", pc.expected_outputs(base, full, pc.OPTIONS))
    assert "PCB" in (tmp_path / "merged" / "README.md").read_text()


def test_two_gloo_ranks_equal_the_oracle(tmp_path, emul):
    base, factors, full = lf.setup_k3(tmp_path, emul)
    cfg = pc.write_config(tmp_path, "org/lora", "merged", pc.OPTIONS, device="cpu")
    run_ranks(cfg)
    assert not list((tmp_path / "merged").glob(".tmp-*"))
    assert_outputs(tmp_path / "merged", pc.expected_outputs(base, full, pc.OPTIONS))
