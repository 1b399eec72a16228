"""operator: tsv without a GPU: `tsv_apply` of csrc/sm_tsv.hpp and the extraction kernels it runs on, on the CPU
work-group emulator against tests/tsv_oracle.py (bit for bit, tests/tsv_checks.py), the properties that define TSV
against torch fp64, the YAML options, and `python -m shard merge` / `analyze` end to end - single process and in place -
with the emulator as the device."""
import click
import pytest
import torch
from click.testing import CliRunner

from shardmerge_amd import distributed
from shardmerge_amd.config import OPERATORS, MergeConfig
from tests import lora_fixtures as lf
from tests import tsv_checks as tc
from tests.harness import emul, run_cli, ties_models, yaml_config  # noqa: F401


# ---- 1. tsv_apply through the probe --------------------------------------------------------------------------------
@pytest.mark.parametrize("Rp", tc.APPLY_WIDTHS)
@pytest.mark.parametrize("shape", tc.APPLY_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_apply_shapes_and_widths(emul, shape, Rp):
    for dtype in tc.DTYPES:
        tc.check_apply(emul, shape[0], shape[1], Rp, dtype)


@pytest.mark.parametrize("dtype", tc.DTYPES, ids=str)
def test_apply_views_and_special_values(emul, dtype):
    tc.check_apply(emul, 130, 257, 32, dtype, offset=1)
    tc.check_apply(emul, 17, 33, 80, dtype, offset=1, special=True)
    tc.check_apply(emul, 257, 130, 16, dtype, special=True, lam=-1.5)


def test_apply_layout_on_integers(emul):
    for rows, cols, Rp in ((17, 33, 16), (130, 257, 48), (257, 130, 256)):
        tc.check_apply_integers(emul, rows, cols, Rp)
    tc.check_apply_empty_panel(emul)


# ---- 2. the whole function -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,own", tc.MERGE_KS, ids=tc.MERGE_K_IDS)
@pytest.mark.parametrize("shape", tc.MERGE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_merge_equals_the_oracle(emul, shape, k, own):
    rep = tc.check_merge(emul, shape[0], shape[1], k, 16, 2, own)
    assert rep.R == 16 * k


@pytest.mark.parametrize("q", (0, 1))
@pytest.mark.parametrize("shape", tc.MERGE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_merge_rank_8(emul, shape, q):
    tc.check_merge(emul, shape[0], shape[1], 3, 8, q)


@pytest.mark.parametrize("base_out_dtype", (torch.float16, torch.float32), ids=str)
def test_merge_base_out_dtypes(emul, base_out_dtype):
    tc.check_merge(emul, 192, 320, 2, 8, 1, base_out_dtype=base_out_dtype)


def test_merge_with_a_zero_alpha(emul):
    rep = tc.check_merge(emul, 192, 320, 3, 16, 1, variant="zero_alpha")
    assert rep.rho == [16, 0, 16] and rep.R == 32 and rep.delta_sq[1] == 0 and rep.orth_ranks[1] == []


def test_merge_of_two_identical_finetunes(emul):
    rep = tc.check_merge(emul, 192, 320, 3, 16, 1, variant="identical")
    assert rep.R == 48 and rep.kept_U == rep.kept_W == 32


def test_merge_with_a_finetune_equal_to_its_base(emul):
    rep = tc.check_merge(emul, 320, 192, 2, 16, 1, variant="equal_base")
    assert rep.rho == [16, 0] and rep.Rp == 16 and rep.delta_sq[1] == 0 and rep.share[1] == 0


def test_merge_rejects_nan_and_inf(emul):
    tc.check_nonfinite(emul)


def test_merge_of_a_rank_3_tensor(emul):
    tc.check_rank3(emul)


@pytest.mark.parametrize("k,q", [(1, 0), (3, 2)])
def test_profile_names_and_launches(emul, k, q):
    tc.check_profile(emul, k, q)


def test_c_abi_rejects_bad_arguments(emul):
    tc.check_c_abi(emul)


# ---- 3. properties ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (2, 3, 5))
def test_singular_values_are_the_weighted_sigmas(emul, k):
    """What defines TSV: the R leading singular values of the merged delta are the sorted alpha_i sigma_ij, the next one
    is rounding, and ||merged||_F^2 = sum s^2.  The numpy restatement of the definition deviates from that by 5.5e-8 of
    s_max (values), 5.4e-8 (next) and 3.7e-8 (Frobenius) at most on these cases; the tolerances are 4 x that."""
    tc.check_singular_values(emul, k)


def test_duplicates_count_once(emul):
    """Two identical finetunes with alphas (1, 1) give the k = 1 result, not twice it: the numpy restatement gives a
    relative difference of 1.25e-7 (task arithmetic: 1.0); the tolerance is 4 x 1.3e-7."""
    tc.check_duplicates(emul)


def test_disjoint_supports_add(emul):
    """Block-diagonal deltas merge to the sum of their separate k = 1 results; the numpy restatement gives exactly that
    (difference 0), and so must the library."""
    tc.check_disjoint_supports(emul)


@pytest.mark.parametrize("rank", tc.xc.RANKS)
@pytest.mark.parametrize("which", ("decay", "gauss", "lowrank+noise"))
def test_k1_is_the_truncation(emul, which, rank):
    tc.check_truncation(emul, which, rank)


# ---- 4. YAML ---------------------------------------------------------------------------------------------------------
def test_yaml_accepts_the_operator_and_its_keys(tmp_path):
    from shardmerge_amd.merge import operator_class
    from shardmerge_amd.merge.fast_fourier import FourierMerge
    from shardmerge_amd.merge.ties import TiesMerge
    from shardmerge_amd.merge.tsv import TsvMerge
    cls = operator_class("tsv")
    assert cls is TsvMerge and issubclass(cls, TiesMerge) and "tsv" in OPERATORS
    cfg = MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": "tsv"}))
    assert cfg.operator == "tsv" and cfg.merge_options == {}
    m = cls(config=cfg, index_manager=object())
    assert (m.tsv_rank, m.tsv_power_iters, m.tsv_lambda, m.seed) == (64, 2, 1.0, 0) and isinstance(m.tsv_rank, int)
    cfg = MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": "tsv", "tsv_rank": 256, "tsv_power_iters": 0, "tsv_lambda": 0.7, "seed": 2 ** 62}))
    assert cfg.merge_options == {"tsv_rank": 256, "tsv_power_iters": 0, "tsv_lambda": 0.7, "seed": 2 ** 62}
    m = cls(config=cfg, index_manager=object())
    assert (m.tsv_rank, m.tsv_power_iters, m.seed) == (256, 0, 2 ** 62)
    readme = m.get_readme()
    for word in ("# TSV Merged Model", "TSV (", "rank 256", "power iterations 0", "lambda 0.7", f"seed {2 ** 62}", "org/ft1"):
        assert word in readme, (word, readme)
    assert cls.merge_block is not TiesMerge.merge_block and cls._merge_layer is FourierMerge._merge_layer
    assert [m.tensor_passes(k) for k in (1, 2)] == [8, 14]


@pytest.mark.parametrize("options,text", [
    ({"tsv_rank": 0}, "an integer in 1..256"), ({"tsv_rank": 257}, "an integer in 1..256"), ({"tsv_rank": 64.0}, "an integer in 1..256"),
    ({"tsv_rank": True}, "an integer in 1..256"), ({"tsv_rank": "64"}, "an integer in 1..256"),
    ({"tsv_power_iters": -1}, "an integer in 0..4"), ({"tsv_power_iters": 5}, "an integer in 0..4"), ({"tsv_power_iters": 1.5}, "an integer in 0..4"),
    ({"tsv_lambda": 1e7}, r"a number in \[-1000000\.0, 1000000\.0\]"), ({"tsv_lambda": float("nan")}, r"a number in \[-1000000\.0, 1000000\.0\]"),
    ({"seed": -1}, r"an integer in \[0, 2\^63\)"), ({"seed": 1.0}, r"an integer in \[0, 2\^63\)")], ids=str)
def test_yaml_rejects_out_of_range_values(tmp_path, options, text):
    (key, _), = options.items()
    with pytest.raises(click.BadParameter, match=rf"merge_options\.{key} must be {text}"):
        MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": "tsv", **options}))


@pytest.mark.parametrize("operator", [None] + [op for op in OPERATORS if op != "tsv"])
@pytest.mark.parametrize("key", ["tsv_rank", "tsv_power_iters", "tsv_lambda"])
def test_yaml_rejects_a_tsv_key_with_another_operator(tmp_path, operator, key):
    opts = {key: 1}
    if operator:
        opts["operator"] = operator
    shown = operator or "fourier"
    with pytest.raises(click.BadParameter, match=rf"merge_options\.{key} is accepted only with operator: tsv \(operator '{shown}' would ignore it\)"):
        MergeConfig.from_yaml(yaml_config(tmp_path, opts))


@pytest.mark.parametrize("key,value", [("cutoff_pct", 0.08), ("cull_start_pct", 0.2), ("t_sum", 1.0), ("target_norm_offset", 1e-10),
                                       ("b", 0.1), ("norm_mode", "exact"), ("task_add_models", ["org/ft1"]), ("density", 0.2),
                                       ("ties_lambda", 1.0), ("ties_normalize", 1), ("dare_lambda", 1.0), ("dare_rescale", 1),
                                       ("gamma", 0.01), ("breadcrumbs_lambda", 1.0), ("stock_filter_wise", 1),
                                       ("select_topk", 0.5), ("sce_lambda", 1.0), ("epsilon", 0.1), ("della_lambda", 1.0),
                                       ("mask_lambda", 0.4), ("consensus_k", 2), ("karcher_max_iter", 10), ("karcher_tol", 1e-5),
                                       ("sphere_row_wise", 1), ("fusion_iqr", 1.5), ("nearswap_t", 0.001), ("pcb_ratio", 0.1),
                                       ("pcb_clip", 0.01), ("pcb_lambda", 1.0), ("bogus", 1)])
def test_yaml_rejects_an_option_tsv_would_ignore(tmp_path, key, value):
    """the message names the rejected key itself and the operator that would ignore it"""
    named = r"unknown keys \['bogus'\]" if key == "bogus" else rf"merge_options\.{key}\b.*operator 'tsv'"
    with pytest.raises(click.BadParameter, match=named):
        MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": "tsv", key: value}))


@pytest.mark.parametrize("alphas", [(0.5, -0.5), (0.0, 0.0), (-1.0, 2.0), (float("inf"), 1.0)], ids=str)
def test_yaml_rejects_a_negative_alpha_or_a_zero_sum(tmp_path, alphas):
    models = [{"model": f"org/ft{i + 1}", "base": "org/base", "alpha": a} for i, a in enumerate(alphas)]
    with pytest.raises(click.BadParameter, match=r"operator tsv needs finetune_merge alphas >= 0 with a sum > 0"):
        MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": "tsv"}, models))
    models[0]["alpha"], models[1]["alpha"] = 0.0, 1.0
    assert [m.alpha for m in MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": "tsv"}, models)).finetune_merge] == [0.0, 1.0]


def test_config_stamp(tmp_path):
    stamp = lambda opts: distributed.config_stamp(MergeConfig.from_yaml(yaml_config(tmp_path, opts)))
    full = {"operator": "tsv", "tsv_rank": 64, "tsv_power_iters": 2, "tsv_lambda": 1.0, "seed": 0}
    base = stamp(full)
    assert base == stamp(dict(full))
    others = [stamp({**full, "tsv_rank": 32}), stamp({**full, "tsv_power_iters": 1}), stamp({**full, "tsv_lambda": 0.9}),
              stamp({**full, "seed": 1}), stamp({"operator": "ties", "density": 0.2}), stamp(None)]
    assert len({base, *others}) == len(others) + 1


# ---- 5. the CLI end to end -------------------------------------------------------------------------------------------
def test_cli_equals_the_oracle_and_dare_linear(tmp_path, emul):
    got = tc.check_cli(tmp_path, emul)
    # two runs give the same bytes; an adapter entry is the run on its materialised checkpoint
    res = run_cli(tc.write_config(tmp_path, "org/lora_full", "again"))
    assert res.exit_code == 0, res.output
    lf.assert_same_outputs(tmp_path / "again", tmp_path / "merged")
    assert (tmp_path / "again" / "README.md").read_bytes() == (tmp_path / "merged" / "README.md").read_bytes()
    res = run_cli(tc.write_config(tmp_path, "org/lora", "merged_adapter"))
    assert res.exit_code == 0, res.output
    lf.assert_same_outputs(tmp_path / "merged_adapter", tmp_path / "merged")
    # the seed and the rank show in the output
    for change in ({"seed": 6}, {"tsv_rank": 8}):
        res = run_cli(tc.write_config(tmp_path, "org/lora_full", "changed", {**tc.OPTIONS, **change}))
        assert res.exit_code == 0, res.output
        other = lf.read_outputs(tmp_path / "changed")
        assert any(not torch.equal(other[n], got[n]) for n in got if "proj" in n and "layers" in n), change
    # analyze keeps accepting the config: the operator's options are validated and not used
    from shardmerge_amd.__main__ import cli
    res = CliRunner().invoke(cli, ["analyze", str(tc.write_config(tmp_path, "org/lora_full", "analysed"))])
    assert res.exit_code == 0, res.output


def test_cli_a_window_that_leaves_one_entry(tmp_path, emul):
    """layer 1 is covered by the third entry alone: every tensor of it is dare_linear's at density 1, bit for bit"""
    lf.setup_k3(tmp_path, emul)
    models = ties_models("org/lora_full")
    models[0]["end_layer"] = 0
    res = run_cli(tc.write_config(tmp_path, "org/lora_full", "merged", models=models))
    assert res.exit_code == 0, res.output
    linear = {"operator": "dare_linear", "density": 1.0, "dare_lambda": tc.OPTIONS["tsv_lambda"]}
    res = run_cli(tc.write_config(tmp_path, "org/lora_full", "linear", linear, models=models))
    assert res.exit_code == 0, res.output
    got, other = lf.read_outputs(tmp_path / "merged"), lf.read_outputs(tmp_path / "linear")
    layer1 = [n for n in got if ".layers.1." in n]
    assert len(layer1) == 4 and all(torch.equal(tc.raw(got[n]), tc.raw(other[n])) for n in layer1)
    assert any(not torch.equal(got[n], other[n]) for n in got if ".layers.0." in n)


def test_cli_in_place_equals_one_process(tmp_path, emul, monkeypatch):
    """the partitioned path merges block tensors itself (distributed._merge_block_tensor): it must run TSV too"""
    lf.setup_k3(tmp_path, emul)
    res = run_cli(tc.write_config(tmp_path, "org/lora", "merged"))
    assert res.exit_code == 0, res.output
    monkeypatch.setenv("SHARDMERGE_INPLACE", "1")
    monkeypatch.setattr(distributed, "ENGINE_FACTORY", lambda: emul)
    res = run_cli(tc.write_config(tmp_path, "org/lora", "inplace"))
    assert res.exit_code == 0, res.output
    lf.assert_same_outputs(tmp_path / "inplace", tmp_path / "merged", file_bytes=False)
    assert "TSV" in (tmp_path / "inplace" / "README.md").read_text()


@pytest.mark.parametrize("inplace", [False, True], ids=["single_process", "inplace"])
def test_too_many_singular_vectors_fail_in_initialize(tmp_path, emul, monkeypatch, inplace):
    """layer 0 has three entries: 3 x min(128, rows, cols) > 256 at q_proj [128 x 128]; nothing is written"""
    if inplace:
        monkeypatch.setenv("SHARDMERGE_INPLACE", "1")
        monkeypatch.setattr(distributed, "ENGINE_FACTORY", lambda: emul)
    lf.setup_k3(tmp_path, emul)
    res = run_cli(tc.write_config(tmp_path, "org/lora_full", "merged", {"operator": "tsv", "tsv_rank": 128}))
    assert res.exit_code != 0
    text = res.output + repr(res.exception)
    assert "model.layers.0.self_attn.q_proj.weight" in text and "3 x 128 = 384" in text, text
    assert not list((tmp_path / "merged").glob("*.safetensors"))
    # 86 vectors per entry still fit (3 x 64 at the 64-row tensors, 3 x 85 = 255 at q_proj)
    res = run_cli(tc.write_config(tmp_path, "org/lora_full", "merged", {"operator": "tsv", "tsv_rank": 85, "tsv_power_iters": 0}))
    assert res.exit_code == 0, res.output
