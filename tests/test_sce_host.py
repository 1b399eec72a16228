"""operator sce without a GPU: the kernels of csrc/sm_sce.hpp on the CPU work-group emulator against tests/sce_oracle.py
(bit for bit, tests/sce_checks.py), the YAML options, the stamp, and `python -m shard merge` end to end - single process,
in place, and two gloo ranks - with the emulator as the device."""
import ctypes as C
from pathlib import Path

import click
import pytest
import torch

from shardmerge_amd import distributed
from shardmerge_amd.config import MergeConfig
from tests import lora_fixtures as lf
from tests import sce_checks as sc
from tests.harness import ALPHAS, DTYPES, KS, assert_outputs, emul, make_inputs, run_cli, run_ranks, yaml_config  # noqa: F401

REPO = Path(__file__).resolve().parents[1]


# ---- the kernels on the emulator against the oracle ---------------------------------------------------------
@pytest.mark.parametrize("bo_dtype", DTYPES, ids=str)
@pytest.mark.parametrize("in_dtype", DTYPES, ids=str)
def test_dtypes(emul, in_dtype, bo_dtype):
    sc.check_dtypes(emul, in_dtype, bo_dtype)


@pytest.mark.parametrize("topk", sc.TOPKS)
@pytest.mark.parametrize("k", KS)
def test_k_and_select_topk(emul, k, topk):
    sc.check_k_topk(emul, k, topk)


@pytest.mark.parametrize("n", sc.SIZES)
def test_sizes(emul, n):
    sc.check_sizes(emul, n)


@pytest.mark.parametrize("check", sc.PROPERTIES, ids=lambda f: f.__name__[len("check_"):])
def test_property(emul, check):
    check(emul)


@pytest.mark.parametrize("check", sc.CORNERS, ids=lambda f: f.__name__[len("check_"):])
def test_corner(emul, check):
    check(emul)


def test_largest_emulator_shape(emul):
    fts, bases, bo = make_inputs((512, 1024), 3, seed=5, own_bases=True)
    sc.check(emul, fts, bases, ALPHAS[:3], bo, select_topk=0.1, lam=0.7, label="512 x 1024")


@pytest.mark.parametrize("topk", [0.1, 1.0])
@pytest.mark.parametrize("k", [1, 2, 5, 16])
def test_profile_names_and_launches(emul, k, topk):
    """three sce_hist and three sce_select launches whatever k - ONE selection stream - and none when it is skipped"""
    sc.check_profile(emul, k, topk)


def test_c_abi_rejects_bad_arguments(emul):
    from shardmerge_amd import _lib
    x = torch.zeros(64, dtype=torch.bfloat16)
    y = torch.zeros(64, dtype=torch.bfloat16)
    out = torch.zeros(64, dtype=torch.bfloat16)

    def call(k=2, topk=0.5, lam=1.0, out_t=out, n=64, in_dtype=_lib.BF16, alpha=0.5, alpha1=None, base=y, ft=x):
        d = _lib.SceDesc()
        d.k = k
        for i in range(max(0, min(k, 16))):
            d.finetune[i], d.base[i], d.alpha[i] = (ft.data_ptr() if ft is not None else None), (base.data_ptr() if base is not None else None), alpha
        if alpha1 is not None:
            d.alpha[1] = alpha1
        d.in_dtype, d.base_out, d.base_out_dtype, d.n = in_dtype, (base.data_ptr() if base is not None else None), _lib.BF16, n
        d.select_topk, d.lam = topk, lam
        rep = _lib.SceReport()
        rc = emul.lib.dll.smhip_sce_merge(emul.ctx.h, C.byref(d), out_t.data_ptr(), None, C.byref(rep), None)
        return rc, emul.lib.dll.smhip_last_error(emul.ctx.h).decode(), rep

    rc, msg, rep = call()
    assert rc == _lib.OK, msg
    assert (rep.nz, rep.k_keep, rep.selected) == (0, 0, 0) and rep.threshold == float("inf") and rep.weight[0] == 0.5
    rc, msg, rep = call(topk=1.0)
    assert rc == _lib.OK and (rep.nz, rep.k_keep, rep.selected, rep.threshold) == (64, 64, 64, 0.0)
    assert call(alpha=0.0, alpha1=0.5)[0] == _lib.OK                       # one alpha of 0 is fine
    for kwargs, word in (({"k": 0}, "k out of range"), ({"k": 17}, "k out of range"),
                         ({"topk": 0.0}, "select_topk"), ({"topk": 1.5}, "select_topk"), ({"topk": float("nan")}, "select_topk"),
                         ({"topk": -0.5}, "select_topk"), ({"lam": float("inf")}, "lambda"),
                         ({"alpha": -0.5}, "alpha"), ({"alpha1": -0.1}, "alpha"), ({"alpha": float("nan")}, "alpha"),
                         ({"alpha1": float("inf")}, "alpha"), ({"alpha": 0.0}, "sum > 0"),
                         ({"base": None}, "null"), ({"ft": None}, "null"), ({"out_t": x}, "overlaps"), ({"in_dtype": 3}, "dtype")):
        rc, msg, _ = call(**kwargs)
        assert rc == _lib.ERR_ARG and word in msg, (kwargs, rc, msg)
    rc = emul.lib.dll.smhip_sce_merge(emul.ctx.h, None, out.data_ptr(), None, None, None)
    assert rc == _lib.ERR_ARG and "null descriptor" in emul.lib.dll.smhip_last_error(emul.ctx.h).decode()
    rc = emul.lib.dll.smhip_sce_merge(emul.ctx.h, C.byref(_lib.SceDesc()), None, None, None, None)
    assert rc == _lib.ERR_ARG
    assert call(n=0, out_t=x)[0] == _lib.OK                         # a no-op, whatever the pointers
    assert call(n=0, out_t=x, base=None, ft=None)[0] == _lib.OK


# ---- YAML ------------------------------------------------------------------------------------------------------
PAIR = [{"model": "org/ft1", "base": "org/base"}, {"model": "org/ft2", "base": "org/base"}]


def test_yaml_accepts_sce_and_its_defaults(tmp_path):
    from shardmerge_amd.merge import operator_class
    from shardmerge_amd.merge.fast_fourier import FourierMerge
    from shardmerge_amd.merge.sce import SceMerge
    from shardmerge_amd.merge.ties import TiesMerge
    cls = operator_class("sce")
    assert cls is SceMerge and issubclass(cls, TiesMerge)
    cfg = MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": "sce"}, PAIR))
    assert cfg.operator == "sce" and cfg.merge_options == {}
    m = cls(config=cfg, index_manager=object())
    assert m.select_topk == 1.0 and m.sce_lambda == 1.0                      # mergekit's name and default
    readme = m.get_readme()
    for word in ("# SCE Merged Model", "SCE (sce:", "select_topk 1", "sce_lambda 1", "org/ft1", "org/ft2"):
        assert word in readme, (word, readme)
    assert cls.merge_block is not TiesMerge.merge_block and cls._merge_layer is FourierMerge._merge_layer
    assert [m.tensor_passes(k) for k in (1, 2, 3)] == [5, 7, 9]                # no selection: 2k + 3
    assert m.block_cost_ms((128, 64), 2) == TiesMerge.block_cost_ms(m, (128, 64), 2)
    cfg = MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": "sce", "select_topk": 0.25, "sce_lambda": -2}, PAIR))
    assert cfg.merge_options == {"select_topk": 0.25, "sce_lambda": -2.0}
    m = cls(config=cfg, index_manager=object())
    assert (m.select_topk, m.sce_lambda) == (0.25, -2.0)
    assert [m.tensor_passes(k) for k in (1, 2, 3)] == [11, 16, 21]             # with selection: 5k + 6
    assert "select_topk 0.25" in m.get_readme() and "sce_lambda -2" in m.get_readme()
    # any number of entries; an alpha of 0 next to a positive one
    three = [{"model": f"org/ft{i}", "base": "org/base", "alpha": a} for i, a in enumerate((0.5, 0.0, 2))]
    assert MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": "sce"}, three)).operator == "sce"
    assert MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": "sce"}, three[:1])).operator == "sce"


@pytest.mark.parametrize("key,value", [("cutoff_pct", 0.08), ("cull_start_pct", 0.2), ("t_sum", 1.0), ("target_norm_offset", 1e-10),
                                       ("b", 0.1), ("norm_mode", "exact"), ("task_add_models", ["org/ft1"]), ("density", 0.5),
                                       ("ties_lambda", 1.0), ("ties_normalize", 1), ("dare_lambda", 1.0), ("dare_normalize", 1),
                                       ("dare_rescale", 1), ("seed", 0), ("gamma", 0.01), ("breadcrumbs_lambda", 1.0),
                                       ("breadcrumbs_normalize", 1), ("stock_filter_wise", 1), ("bogus", 1)])
def test_yaml_rejects_an_option_sce_would_ignore(tmp_path, key, value):
    with pytest.raises(click.BadParameter, match=key) as e:
        MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": "sce", key: value}, PAIR))
    assert f"merge_options.{key}" in str(e.value) or key == "bogus"
    assert "sce" in str(e.value)


@pytest.mark.parametrize("operator", [None, "fourier", "addition", "task_addition", "fourier_legacy", "ties", "dare_ties", "dare_linear",
                                      "breadcrumbs", "breadcrumbs_ties", "model_stock", "nuslerp", "slerp"])
@pytest.mark.parametrize("key", ["select_topk", "sce_lambda"])
def test_yaml_rejects_the_sce_keys_with_another_operator(tmp_path, operator, key):
    opts = {key: 0.5}
    if operator:
        opts["operator"] = operator
    with pytest.raises(click.BadParameter, match=rf"merge_options\.{key} is accepted only with operator: sce \("):
        MergeConfig.from_yaml(yaml_config(tmp_path, opts, PAIR))


def test_yaml_rejects_bad_values_and_alphas(tmp_path):
    for bad in (0, 0.0, -0.1, 1.5, "half", True, float("nan")):
        with pytest.raises(click.BadParameter, match=r"merge_options\.select_topk must be a number in \(0, 1\]"):
            MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": "sce", "select_topk": bad}, PAIR))
    for bad in (1e7, -1e7, "two", float("inf")):
        with pytest.raises(click.BadParameter, match=r"merge_options\.sce_lambda must be a number in"):
            MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": "sce", "sce_lambda": bad}, PAIR))
    entry = lambda i, a=1.0: {"model": f"org/ft{i}", "base": "org/base", "alpha": a}
    for alphas in ((-0.5, 1.0), (0.5, -0.1), (0.0, 0.0), (float("nan"), 1.0), (float("inf"), 1.0), (1.0, 1.0, -1e-9)):
        with pytest.raises(click.BadParameter, match="operator sce needs finetune_merge alphas >= 0 with a sum > 0"):
            MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": "sce"}, [entry(i, a) for i, a in enumerate(alphas)]))
    # the other delta-merge operators keep taking signed alphas
    assert MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": "ties"}, [entry(1, -0.5), entry(2, 1.0)])).operator == "ties"


def test_config_stamp(tmp_path):
    stamp = lambda opts: distributed.config_stamp(MergeConfig.from_yaml(yaml_config(tmp_path, opts, PAIR)))
    base = stamp({"operator": "sce", "select_topk": 0.5})
    assert base == stamp({"operator": "sce", "select_topk": 0.5})
    others = [stamp({"operator": "sce", "select_topk": 0.25}), stamp({"operator": "sce"}), stamp({"operator": "sce", "select_topk": 0.5, "sce_lambda": 0.5}),
              stamp({"operator": "ties"}), stamp({"operator": "model_stock"}), stamp({"operator": "dare_linear"}), stamp(None)]
    assert len({base, *others}) == len(others) + 1


def test_readme_of_the_repository_names_the_operator():
    text = (REPO / "README.md").read_text()
    for word in ("**SCE merge.**", "operator: sce", "select_topk", "sce_lambda", "tools/sce_bench.py", "smhip_sce_merge"):
        assert word in text, word
    assert "sm_sce.hpp" in (REPO / "DESIGN.md").read_text()


# ---- the CLI end to end ------------------------------------------------------------------------------------------
def test_cli_equals_the_oracle_tensor_by_tensor(tmp_path, emul):
    base, factors, full = lf.setup_k3(tmp_path, emul)
    expected = sc.expected_outputs(base, full)
    assert any(not torch.equal(expected[n], base[n]) for n in expected if "layers" in n)
    res = run_cli(sc.write_config(tmp_path, "org/lora_full", "merged"))
    assert res.exit_code == 0, res.output
    assert_outputs(tmp_path / "merged", expected)
    readme = (tmp_path / "merged" / "README.md").read_text()
    for word in sc.README_WORDS:
        assert word in readme, (word, readme)
    # one finetune given as a LoRA adapter directory: the run on its materialised checkpoint
    res = run_cli(sc.write_config(tmp_path, "org/lora", "merged_adapter"))
    assert res.exit_code == 0, res.output
    lf.assert_same_outputs(tmp_path / "merged_adapter", tmp_path / "merged")
    # another select_topk is another model
    other = sc.expected_outputs(base, full, {"operator": "sce", "select_topk": 1.0, "sce_lambda": 0.7})
    assert any(not torch.equal(other[n], expected[n]) for n in expected if "layers" in n)


def test_cli_in_place_equals_the_oracle(tmp_path, emul, monkeypatch):
    """the partitioned path merges block tensors itself (distributed._merge_block_tensor): it must run this operator too"""
    monkeypatch.setenv("SHARDMERGE_INPLACE", "1")
    monkeypatch.setattr(distributed, "ENGINE_FACTORY", lambda: emul)
    base, factors, full = lf.setup_k3(tmp_path, emul)
    res = run_cli(sc.write_config(tmp_path, "org/lora", "merged"))
    assert res.exit_code == 0, res.output
    assert_outputs(tmp_path / "merged", sc.expected_outputs(base, full))
    assert sc.README_WORDS[0] in (tmp_path / "merged" / "README.md").read_text()


def test_two_gloo_ranks_equal_the_oracle(tmp_path, emul):
    base, factors, full = lf.setup_k3(tmp_path, emul)
    cfg = sc.write_config(tmp_path, "org/lora", "merged", device="cpu")
    run_ranks(cfg)
    assert not list((tmp_path / "merged").glob(".tmp-*"))
    assert_outputs(tmp_path / "merged", sc.expected_outputs(base, full))
