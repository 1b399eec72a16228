"""operator: iso_c without a GPU: `iso_gemm` and the small kernels of csrc/sm_iso.hpp on the CPU work-group emulator
against tests/iso_oracle.py (bit for bit, tests/iso_checks.py), what defines Iso-C against torch fp64 `linalg.svd`, the
properties of the function, the YAML options, and `python -m shard merge` / `analyze` end to end - single process, in
place and on two gloo ranks - with the emulator as the device."""
import click
import pytest
import torch
from click.testing import CliRunner

from shardmerge_amd import distributed
from shardmerge_amd.config import OPERATORS, MergeConfig
from tests import iso_checks as ic
from tests import iso_oracle as io
from tests import lora_fixtures as lf
from tests.harness import assert_outputs, emul, run_cli, run_ranks, ties_models, yaml_config  # noqa: F401


# ---- 1. iso_gemm through the probe ---------------------------------------------------------------------------------
@pytest.mark.parametrize("K", ic.GEMM_K)
def test_gemm_shapes(emul, K):
    for M, N in ic.GEMM_MN:
        for form in (io.NT, io.NN):
            ic.check_gemm(emul, form, M, N, K)


@pytest.mark.parametrize("ep", (io.POLY, io.AXPY, io.CUBIC))
@pytest.mark.parametrize("form", (io.NT, io.NN))
def test_gemm_epilogues(emul, form, ep):
    for M, N, K in ((17, 15, 5), (129, 257, 33), (128, 128, 32)):
        ic.check_gemm(emul, form, M, N, K, ep)


@pytest.mark.parametrize("form", (io.NT, io.NN))
def test_gemm_views_and_special_values(emul, form):
    ic.check_gemm(emul, form, 129, 130, 33, io.CUBIC, offset=1)
    ic.check_gemm(emul, form, 130, 129, 35, io.POLY, offset=1, pad=3)
    ic.check_gemm(emul, form, 33, 130, 64, io.AXPY, pad=4)            # aligned rows, a pitch that is not the width
    ic.check_gemm(emul, form, 65, 47, 37, io.PLAIN, special=True)
    ic.check_gemm(emul, form, 17, 33, 9, io.POLY, offset=1, special=True)
    for poke in (float("nan"), float("inf"), float("-inf")):
        ic.check_gemm(emul, form, 33, 17, 35, io.AXPY, poke=poke)


@pytest.mark.parametrize("s,K", ic.GEMM_SYM)
def test_gemm_symmetric_mode(emul, s, K):
    ic.check_gemm_sym(emul, s, K, gram=True)
    ic.check_gemm_sym(emul, s, K, gram=False)


def test_gemm_layout_on_integers(emul):
    for form in (io.NT, io.NN):
        for M, N, K in ((17, 33, 5), (130, 257, 33), (257, 130, 64)):
            ic.check_gemm_integers(emul, form, M, N, K)


# ---- 2. the whole function -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ic.MERGE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_merge_equals_the_oracle(emul, shape):
    rep = ic.check_merge(emul, shape, 2)
    assert rep.converged and rep.transposed == (shape[0] > shape[1])


@pytest.mark.parametrize("k,own", ic.MERGE_KS, ids=ic.MERGE_K_IDS)
@pytest.mark.parametrize("shape", ((17, 33), (33, 17)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_merge_k_and_bases(emul, shape, k, own):
    ic.check_merge(emul, shape, k, own)


def test_merge_k3_own_bases_over_several_tiles(emul):
    ic.check_merge(emul, (130, 257), 3, True)


@pytest.mark.parametrize("bo_dtype", ic.DTYPES, ids=str)
@pytest.mark.parametrize("in_dtype", ic.DTYPES, ids=str)
def test_merge_dtype_pairs(emul, in_dtype, bo_dtype):
    ic.check_merge(emul, (33, 17), 2, in_dtype=in_dtype, bo_dtype=bo_dtype)


def test_merge_of_a_rank_3_tensor(emul):
    ic.check_rank3(emul)


def test_merge_of_finetunes_equal_to_their_bases(emul):
    for shape in ((17, 33), (130, 40)):
        rep = ic.check_merge(emul, shape, 2, variant="zero")
        assert rep.zero and rep.nu == 0 and rep.steps == "" and rep.e == [] and not rep.converged


def test_merge_rejects_nan_and_inf(emul):
    ic.check_nonfinite(emul)


def test_merge_max_iter_0_and_2(emul):
    rep = ic.check_merge(emul, (33, 17), 3, max_iter=0)
    assert rep.iterations == 0 and rep.steps == "" and len(rep.e) == 1 and not rep.converged
    rep = ic.check_merge(emul, (130, 257), 2, max_iter=2)
    assert rep.iterations == 2 and rep.steps == "qq" and len(rep.e) == 3 and not rep.converged


def test_merge_negative_and_zero_alphas(emul):
    ic.check_merge(emul, (17, 33), 3, variant="signs")
    ic.check_merge(emul, (33, 17), 5, True, variant="signs")


# ---- 3. what defines Iso-C -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,k", ic.SVD_CASES, ids=lambda v: str(v))
def test_merged_delta_is_the_isotropic_one(emul, shape, k):
    """Against torch fp64 `linalg.svd` of the task sum: ||merged - mean(S) U V^T||_F / ||ref||_F, |sigma_bar - mean(S)| /
    mean(S), and the spread (S_max - S_min) / sigma_bar of the merged delta's own singular values.  The numpy restatement
    deviates on these cases, measured on the CPU (iso_checks.SVD_MEASURED), by 1.02e-6 / 3.86e-7 / 1.99e-6 at 128 x 512
    with k = 3, 9.81e-7 / 3.67e-7 / 1.94e-6 at 512 x 128 with k = 2 and 1.28e-6 / 4.93e-9 / 1.62e-6 at 256 x 256 with k = 2;
    the tolerances are 4 x that."""
    ic.check_against_svd(emul, shape, k)


# ---- 4. properties ---------------------------------------------------------------------------------------------------
def test_transposed_inputs_give_the_transposed_output(emul):
    ic.check_transpose(emul)


def test_doubled_alphas_double_the_delta(emul):
    ic.check_doubled_alphas(emul)


def test_swapped_entries_with_equal_alphas(emul):
    ic.check_swapped_entries(emul)


def test_k1_partial_permutation_is_kept(emul):
    ic.check_partial_permutation(emul)


# ---- 5. host logic ---------------------------------------------------------------------------------------------------
def test_yaml_accepts_the_operator_and_its_keys(tmp_path):
    from shardmerge_amd.merge import operator_class
    from shardmerge_amd.merge.fast_fourier import FourierMerge
    from shardmerge_amd.merge.iso import IsoMerge
    from shardmerge_amd.merge.ties import TiesMerge
    cls = operator_class("iso_c")
    assert cls is IsoMerge and issubclass(cls, TiesMerge) and "iso_c" in OPERATORS
    cfg = MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": "iso_c"}))
    assert cfg.operator == "iso_c" and cfg.merge_options == {}
    m = cls(config=cfg, index_manager=object())
    assert (m.iso_lambda, m.iso_tol, m.iso_max_iter) == (1.0, 1e-4, 40) and isinstance(m.iso_max_iter, int)
    cfg = MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": "iso_c", "iso_lambda": 0.7, "iso_tol": 1, "iso_max_iter": 0}))
    assert cfg.merge_options == {"iso_lambda": 0.7, "iso_tol": 1.0, "iso_max_iter": 0}
    m = cls(config=cfg, index_manager=object())
    assert (m.iso_lambda, m.iso_tol, m.iso_max_iter) == (0.7, 1.0, 0)
    readme = m.get_readme()
    for word in ("# Iso-C Merged Model", "Iso-C (", "lambda 0.7", "tol 1", "max_iter 0", "org/ft1"):
        assert word in readme, (word, readme)
    assert cls.merge_block is not TiesMerge.merge_block and cls._merge_layer is FourierMerge._merge_layer
    assert [m.tensor_passes(k) for k in (1, 3)] == [4, 8]


@pytest.mark.parametrize("options,text", [
    ({"iso_tol": 0}, r"a number in \(0, 1\]"), ({"iso_tol": 1.5}, r"a number in \(0, 1\]"), ({"iso_tol": float("nan")}, r"a number in \(0, 1\]"),
    ({"iso_tol": "1e-4"}, r"a number in \(0, 1\]"), ({"iso_tol": True}, r"a number in \(0, 1\]"),
    ({"iso_max_iter": -1}, "an integer in 0..200"), ({"iso_max_iter": 201}, "an integer in 0..200"), ({"iso_max_iter": 40.0}, "an integer in 0..200"),
    ({"iso_max_iter": True}, "an integer in 0..200"),
    ({"iso_lambda": 1e7}, r"a number in \[-1000000\.0, 1000000\.0\]"), ({"iso_lambda": float("nan")}, r"a number in \[-1000000\.0, 1000000\.0\]")], ids=str)
def test_yaml_rejects_out_of_range_values(tmp_path, options, text):
    (key, _), = options.items()
    with pytest.raises(click.BadParameter, match=rf"merge_options\.{key} must be {text}"):
        MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": "iso_c", **options}))


@pytest.mark.parametrize("operator", [None] + [op for op in OPERATORS if op != "iso_c"])
@pytest.mark.parametrize("key", ["iso_lambda", "iso_tol", "iso_max_iter"])
def test_yaml_rejects_an_iso_key_with_another_operator(tmp_path, operator, key):
    opts = {key: 1}
    if operator:
        opts["operator"] = operator
    shown = operator or "fourier"
    with pytest.raises(click.BadParameter, match=rf"merge_options\.{key} is accepted only with operator: iso_c \(operator '{shown}' would ignore it\)"):
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
                                       ("cabs_conflict_aware", 1), ("cabs_lambda", 1.0), ("bogus", 1)])
def test_yaml_rejects_an_option_iso_c_would_ignore(tmp_path, key, value):
    """the message names the rejected key itself and the operator that would ignore it"""
    named = r"unknown keys \['bogus'\]" if key == "bogus" else rf"merge_options\.{key}\b.*operator 'iso_c'"
    with pytest.raises(click.BadParameter, match=named):
        MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": "iso_c", key: value}))


def test_yaml_accepts_alphas_of_any_sign(tmp_path):
    models = [{"model": f"org/ft{i + 1}", "base": "org/base", "alpha": a} for i, a in enumerate((-0.5, 0.0, 0.5))]
    assert [m.alpha for m in MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": "iso_c"}, models)).finetune_merge] == [-0.5, 0.0, 0.5]


def test_config_stamp(tmp_path):
    stamp = lambda opts: distributed.config_stamp(MergeConfig.from_yaml(yaml_config(tmp_path, opts)))
    full = {"operator": "iso_c", "iso_lambda": 1.0, "iso_tol": 1e-4, "iso_max_iter": 40}
    base = stamp(full)
    assert base == stamp(dict(full))
    others = [stamp({**full, "iso_lambda": 0.9}), stamp({**full, "iso_tol": 1e-3}), stamp({**full, "iso_max_iter": 39}),
              stamp({"operator": "ties", "density": 0.2}), stamp(None)]
    assert len({base, *others}) == len(others) + 1


def test_c_abi_rejects_bad_arguments(emul):
    ic.check_c_abi(emul)


def test_profile_names_and_launches(emul):
    rep = ic.check_profile(emul, (96, 160), 2)
    assert rep.converged and set(rep.steps) == {"q", "c"}
    rep = ic.check_profile(emul, (160, 96), 3, max_iter=1)
    assert rep.steps == "q" and rep.transposed
    rep = ic.check_profile(emul, (96, 160), 2, max_iter=0)
    assert rep.steps == ""
    ic.check_profile(emul, (160, 96), 2, zero=True)


@pytest.mark.parametrize("inplace", [False, True], ids=["single_process", "inplace"])
def test_a_matrix_too_large_fails_in_initialize(tmp_path, emul, monkeypatch, inplace):
    """min(rows, cols) above the limit (lowered to 100 here: q_proj is 128 x 128) is an error before anything is written"""
    from shardmerge_amd.merge import iso as iso_mod
    if inplace:
        monkeypatch.setenv("SHARDMERGE_INPLACE", "1")
        monkeypatch.setattr(distributed, "ENGINE_FACTORY", lambda: emul)
    lf.setup_k3(tmp_path, emul)
    monkeypatch.setattr(iso_mod, "ISO_MAX_S", 100)
    res = run_cli(ic.write_config(tmp_path, "org/lora_full", "merged"))
    assert res.exit_code != 0
    text = res.output + repr(res.exception)
    assert "model.layers.0.self_attn.q_proj.weight" in text and "min(rows, cols) = 128" in text and "at most 100" in text, text
    assert not list((tmp_path / "merged").glob("*.safetensors"))
    monkeypatch.setattr(iso_mod, "ISO_MAX_S", 128)
    res = run_cli(ic.write_config(tmp_path, "org/lora_full", "merged"))
    assert res.exit_code == 0, res.output


def test_engine_rejects_a_matrix_too_large(emul):
    """the engine's own limit, before any memory is touched: a [16385 x 16385] view of one element"""
    x = torch.zeros(1, dtype=torch.bfloat16).expand(16385, 16385)
    with pytest.raises(ValueError, match=r"layers\.5.*min\(rows, cols\) = 16385, at most 16384"):
        emul.iso_merge([x], [x], [1.0], x, layer_name="layers.5")


# ---- 6. the CLI end to end -------------------------------------------------------------------------------------------
def test_cli_equals_the_oracle_tensor_by_tensor(tmp_path, emul):
    expected = ic.check_cli(tmp_path, emul)
    # two runs give the same bytes; an adapter entry is the run on its materialised checkpoint
    res = run_cli(ic.write_config(tmp_path, "org/lora_full", "again"))
    assert res.exit_code == 0, res.output
    lf.assert_same_outputs(tmp_path / "again", tmp_path / "merged")
    assert (tmp_path / "again" / "README.md").read_bytes() == (tmp_path / "merged" / "README.md").read_bytes()
    res = run_cli(ic.write_config(tmp_path, "org/lora", "merged_adapter"))
    assert res.exit_code == 0, res.output
    lf.assert_same_outputs(tmp_path / "merged_adapter", tmp_path / "merged")
    # lambda shows in the output
    res = run_cli(ic.write_config(tmp_path, "org/lora_full", "changed", {**ic.OPTIONS, "iso_lambda": 0.5}))
    assert res.exit_code == 0, res.output
    other = lf.read_outputs(tmp_path / "changed")
    assert any(not torch.equal(other[n], expected[n]) for n in expected if "proj" in n and "layers" in n)
    # analyze accepts the config: the operator's options are validated and not used
    from shardmerge_amd.__main__ import cli
    res = CliRunner().invoke(cli, ["analyze", str(ic.write_config(tmp_path, "org/lora_full", "analysed"))])
    assert res.exit_code == 0, res.output


def test_cli_a_window_that_leaves_one_entry(tmp_path, emul):
    """layer 1 is covered by the third entry alone: the function at k = 1"""
    base, factors, full = lf.setup_k3(tmp_path, emul)
    models = ties_models("org/lora_full")
    models[0]["end_layer"] = 0
    res = run_cli(ic.write_config(tmp_path, "org/lora_full", "merged", models=models))
    assert res.exit_code == 0, res.output
    assert_outputs(tmp_path / "merged", ic.expected_outputs(base, full, ic.OPTIONS, models=models))


def test_cli_in_place_equals_the_oracle(tmp_path, emul, monkeypatch):
    """the partitioned path merges block tensors itself (distributed._merge_block_tensor): it must run Iso-C too"""
    monkeypatch.setenv("SHARDMERGE_INPLACE", "1")
    monkeypatch.setattr(distributed, "ENGINE_FACTORY", lambda: emul)
    base, factors, full = lf.setup_k3(tmp_path, emul)
    res = run_cli(ic.write_config(tmp_path, "org/lora", "merged"))
    assert res.exit_code == 0, res.output
    assert_outputs(tmp_path / "merged", ic.expected_outputs(base, full, ic.OPTIONS))
    assert "Iso-C" in (tmp_path / "merged" / "README.md").read_text()


def test_two_gloo_ranks_equal_the_oracle(tmp_path, emul):
    base, factors, full = lf.setup_k3(tmp_path, emul)
    cfg = ic.write_config(tmp_path, "org/lora", "merged", device="cpu")
    run_ranks(cfg)
    assert not list((tmp_path / "merged").glob(".tmp-*"))
    assert_outputs(tmp_path / "merged", ic.expected_outputs(base, full, ic.OPTIONS))
