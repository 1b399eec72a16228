"""operators model_stock / nuslerp / slerp without a GPU: the kernels of csrc/sm_geo.hpp on the CPU work-group emulator
against tests/geo_oracle.py (bit for bit, tests/geo_checks.py), the Gram against exact arithmetic, the YAML options, the
stamp, and `python -m shard merge` end to end - single process, in place, and two gloo ranks - with the emulator as the
device."""
import ctypes as C

import click
import pytest
import torch

from shardmerge_amd import distributed
from shardmerge_amd.config import MergeConfig
from tests import geo_checks as gc
from tests import lora_fixtures as lf
from tests.harness import ALPHAS, DTYPES, KS, assert_outputs, emul, make_inputs, run_cli, run_ranks, yaml_config  # noqa: F401

OPERATORS = ("model_stock", "nuslerp", "slerp")
# what the CLI tests run: (operator, stock_filter_wise)
CLI_CASES = [("model_stock", None), ("model_stock", 1), ("nuslerp", None), ("slerp", None)]
CLI_IDS = ["model_stock", "model_stock_filter_wise", "nuslerp", "slerp"]


# ---- the kernels on the emulator against the oracle ---------------------------------------------------------
@pytest.mark.parametrize("mode,rowwise", gc.VARIANTS, ids=gc.VARIANT_IDS)
@pytest.mark.parametrize("bo_dtype", DTYPES, ids=str)
@pytest.mark.parametrize("in_dtype", DTYPES, ids=str)
def test_dtypes(emul, in_dtype, bo_dtype, mode, rowwise):
    gc.check_dtypes(emul, in_dtype, bo_dtype, mode, rowwise)


@pytest.mark.parametrize("rowwise", [False, True], ids=["whole", "rowwise"])
@pytest.mark.parametrize("k", KS)
def test_model_stock_k(emul, k, rowwise):
    gc.check_k(emul, k, rowwise)


@pytest.mark.parametrize("check", gc.PROPERTIES, ids=lambda f: f.__name__[len("check_"):])
def test_property(emul, check):
    check(emul)


@pytest.mark.parametrize("check", gc.CORNERS, ids=lambda f: f.__name__[len("check_"):])
def test_corner(emul, check):
    check(emul)


def test_largest_emulator_shape(emul):
    fts, bases, bo = make_inputs((512, 1024), 3, seed=5, own_bases=True)
    gc.check(emul, fts, bases, ALPHAS[:3], bo, "model_stock", label="512 x 1024")
    gc.check(emul, fts, bases, ALPHAS[:3], bo, "model_stock", True, label="512 x 1024 row-wise")
    gc.check(emul, fts[:2], bases[:2], ALPHAS[:2], bo, "nuslerp", label="512 x 1024 nuslerp")


@pytest.mark.parametrize("k", [2, 5, 16])
@pytest.mark.parametrize("mode,rowwise", gc.VARIANTS, ids=gc.VARIANT_IDS)
def test_profile_names_and_launches(emul, mode, rowwise, k):
    """ONE Gram launch and ONE combine launch per call: the tiles of pairs of k > 4 are part of the Gram's grid"""
    gc.check_profile(emul, mode, rowwise, gc.variant_k(mode, k))


def test_c_abi_rejects_bad_arguments(emul):
    from shardmerge_amd import _lib
    x = torch.zeros(64, dtype=torch.bfloat16)
    y = torch.zeros(64, dtype=torch.bfloat16)
    out = torch.zeros(64, dtype=torch.bfloat16)

    def call(k=2, mode=_lib.GEO_MODEL_STOCK, rowwise=0, rows=1, out_t=out, n=64, in_dtype=_lib.BF16, alpha=0.5, alpha1=None, base=y):
        d = _lib.GeoDesc()
        d.k = k
        for i in range(max(0, min(k, 16))):
            d.finetune[i], d.base[i], d.alpha[i] = x.data_ptr(), (base.data_ptr() if base is not None else None), alpha
        if alpha1 is not None:
            d.alpha[1] = alpha1
        d.in_dtype, d.base_out, d.base_out_dtype, d.n = in_dtype, (base.data_ptr() if base is not None else None), _lib.BF16, n
        d.mode, d.rowwise, d.rows = mode, rowwise, rows
        rep = _lib.GeoReport()
        rc = emul.lib.dll.smhip_geo_merge(emul.ctx.h, C.byref(d), out_t.data_ptr(), None, C.byref(rep), None)
        return rc, emul.lib.dll.smhip_last_error(emul.ctx.h).decode(), rep

    for mode in (_lib.GEO_MODEL_STOCK, _lib.GEO_NUSLERP, _lib.GEO_SLERP):
        rc, msg, rep = call(mode=mode)
        assert rc == _lib.OK, msg
        assert rep.linear == (0 if mode == _lib.GEO_MODEL_STOCK else 1)         # zero vectors: the linear case
    assert call(rowwise=1, rows=8)[0] == _lib.OK
    assert call(mode=_lib.GEO_SLERP, base=None)[0] == _lib.OK                    # weight space reads no base
    for kwargs, word in (({"k": 0}, "k out of range"), ({"k": 17}, "k out of range"), ({"mode": 3}, "mode"), ({"mode": -1}, "mode"),
                         ({"k": 3, "mode": _lib.GEO_SLERP}, "k <= 2"), ({"k": 3, "mode": _lib.GEO_NUSLERP}, "k <= 2"),
                         ({"mode": _lib.GEO_SLERP, "alpha": -0.5}, "alphas >= 0"), ({"mode": _lib.GEO_NUSLERP, "alpha1": -0.1}, "alphas >= 0"),
                         ({"mode": _lib.GEO_NUSLERP, "alpha": 0.0}, "sum > 0"),
                         ({"mode": _lib.GEO_SLERP, "rowwise": 1}, "rowwise"), ({"mode": _lib.GEO_NUSLERP, "rowwise": 1}, "rowwise"),
                         ({"rows": 0}, "rows"), ({"rows": 7}, "rows"), ({"rowwise": 1, "rows": 5}, "rows"),
                         ({"alpha": float("nan")}, "alpha"), ({"base": None}, "null"),
                         ({"out_t": x}, "overlaps"), ({"in_dtype": 3}, "dtype")):
        rc, msg, _ = call(**kwargs)
        assert rc == _lib.ERR_ARG and word in msg, (kwargs, rc, msg)
    rc = emul.lib.dll.smhip_geo_merge(emul.ctx.h, None, out.data_ptr(), None, None, None)
    assert rc == _lib.ERR_ARG and "null descriptor" in emul.lib.dll.smhip_last_error(emul.ctx.h).decode()
    assert call(n=0, out_t=x, rows=0)[0] == _lib.OK                 # a no-op, whatever the pointers


# ---- YAML ------------------------------------------------------------------------------------------------------
PAIR = [{"model": "org/ft1", "base": "org/base"}, {"model": "org/ft2", "base": "org/base"}]


@pytest.mark.parametrize("operator", OPERATORS)
def test_yaml_accepts_the_operators_and_their_defaults(tmp_path, operator):
    from shardmerge_amd.merge import operator_class
    from shardmerge_amd.merge.fast_fourier import FourierMerge
    from shardmerge_amd.merge.geometric import ModelStockMerge, NuSlerpMerge, SlerpMerge
    from shardmerge_amd.merge.ties import TiesMerge
    cls = operator_class(operator)
    assert cls is {"model_stock": ModelStockMerge, "nuslerp": NuSlerpMerge, "slerp": SlerpMerge}[operator] and issubclass(cls, TiesMerge)
    cfg = MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": operator}, PAIR))
    assert cfg.operator == operator and cfg.merge_options == {}
    m = cls(config=cfg, index_manager=object())
    assert m.mode == operator and not m.stock_filter_wise
    readme = m.get_readme()
    for word in gc.README_WORDS[operator] + ("org/ft1", "org/ft2"):
        assert word in readme, (word, readme)
    assert cls.merge_block is not TiesMerge.merge_block and cls._merge_layer is FourierMerge._merge_layer
    assert m.tensor_passes(2) == (5 if operator == "slerp" else 7)
    assert m.block_cost_ms((128, 64), 2) == TiesMerge.block_cost_ms(m, (128, 64), 2)


def test_yaml_stock_filter_wise(tmp_path):
    from shardmerge_amd.merge.geometric import ModelStockMerge
    for value, want in ((1, 1.0), (0, 0.0), (1.0, 1.0)):
        cfg = MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": "model_stock", "stock_filter_wise": value}, PAIR))
        assert cfg.merge_options == {"stock_filter_wise": want}
        m = ModelStockMerge(config=cfg, index_manager=object())
        assert bool(m.stock_filter_wise) is bool(want)
        assert ("per row" in m.get_readme()) is bool(want)
    for bad in (2, 0.5, -1, "yes", True):
        with pytest.raises(click.BadParameter, match="stock_filter_wise must be 0 or 1"):
            MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": "model_stock", "stock_filter_wise": bad}, PAIR))
    # model_stock takes any number of entries
    three = [{"model": f"org/ft{i}", "base": "org/base"} for i in range(3)]
    assert MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": "model_stock"}, three)).operator == "model_stock"
    assert MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": "model_stock"}, three[:1])).operator == "model_stock"


@pytest.mark.parametrize("operator", [None, "fourier", "addition", "task_addition", "fourier_legacy", "ties", "dare_ties", "dare_linear",
                                      "breadcrumbs", "breadcrumbs_ties", "nuslerp", "slerp"])
def test_yaml_rejects_stock_filter_wise_with_another_operator(tmp_path, operator):
    opts = {"stock_filter_wise": 1}
    if operator:
        opts["operator"] = operator
    with pytest.raises(click.BadParameter, match=r"merge_options\.stock_filter_wise is accepted only with operator: model_stock \("):
        MergeConfig.from_yaml(yaml_config(tmp_path, opts, PAIR))


@pytest.mark.parametrize("operator", OPERATORS)
@pytest.mark.parametrize("key,value", [("cutoff_pct", 0.08), ("cull_start_pct", 0.2), ("t_sum", 1.0), ("target_norm_offset", 1e-10),
                                       ("b", 0.1), ("norm_mode", "exact"), ("task_add_models", ["org/ft1"]), ("density", 0.5),
                                       ("ties_lambda", 1.0), ("ties_normalize", 1), ("dare_lambda", 1.0), ("dare_normalize", 1),
                                       ("dare_rescale", 1), ("seed", 0), ("gamma", 0.01), ("breadcrumbs_lambda", 1.0),
                                       ("breadcrumbs_normalize", 1), ("bogus", 1)])
def test_yaml_rejects_an_option_the_operators_would_ignore(tmp_path, operator, key, value):
    with pytest.raises(click.BadParameter, match=key) as e:
        MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": operator, key: value}, PAIR))
    assert f"merge_options.{key}" in str(e.value) or key == "bogus"


@pytest.mark.parametrize("operator", ["nuslerp", "slerp"])
def test_yaml_rejects_pair_operators_without_a_pair(tmp_path, operator):
    entry = lambda i, a=1.0: {"model": f"org/ft{i}", "base": "org/base", "alpha": a}
    for models in ([entry(1)], [entry(1), entry(2), entry(3)]):
        with pytest.raises(click.BadParameter, match=f"operator {operator} interpolates between exactly two finetune_merge entries, not {len(models)}"):
            MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": operator}, models))
    for a0, a1 in ((-0.5, 1.0), (0.5, -0.1), (0.0, 0.0), (float("nan"), 1.0)):
        with pytest.raises(click.BadParameter, match=f"operator {operator} needs finetune_merge alphas >= 0 with a sum > 0"):
            MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": operator}, [entry(1, a0), entry(2, a1)]))
    assert MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": operator}, [entry(1, 1.0), entry(2, 0.0)])).operator == operator


def test_config_stamp(tmp_path):
    stamp = lambda opts: distributed.config_stamp(MergeConfig.from_yaml(yaml_config(tmp_path, opts, PAIR)))
    base = stamp({"operator": "model_stock", "stock_filter_wise": 0})
    assert base == stamp({"operator": "model_stock", "stock_filter_wise": 0})
    others = [stamp({"operator": "model_stock", "stock_filter_wise": 1}), stamp({"operator": "nuslerp"}), stamp({"operator": "slerp"}),
              stamp({"operator": "ties"}), stamp({"operator": "dare_linear"}), stamp(None)]
    assert len({base, *others}) == len(others) + 1


# ---- the CLI end to end ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("operator,filter_wise", CLI_CASES, ids=CLI_IDS)
def test_cli_equals_the_oracle_tensor_by_tensor(tmp_path, emul, operator, filter_wise):
    base, factors, full = lf.setup_k3(tmp_path, emul)
    opts = gc.options(operator, filter_wise)
    expected = gc.expected_outputs(base, full, opts)
    assert any(not torch.equal(expected[n], base[n]) for n in expected if "layers" in n)
    res = run_cli(gc.write_config(tmp_path, "org/lora_full", "merged", opts))
    assert res.exit_code == 0, res.output
    assert_outputs(tmp_path / "merged", expected)
    readme = (tmp_path / "merged" / "README.md").read_text()
    for word in gc.README_WORDS[operator] + (("per row",) if filter_wise else ()):
        assert word in readme, (word, readme)
    # one finetune given as a LoRA adapter directory: the run on its materialised checkpoint
    res = run_cli(gc.write_config(tmp_path, "org/lora", "merged_adapter", opts))
    assert res.exit_code == 0, res.output
    lf.assert_same_outputs(tmp_path / "merged_adapter", tmp_path / "merged")
    if operator == "model_stock":
        # the other granularity is another model
        other_opts = gc.options(operator, 0 if filter_wise else 1)
        other = gc.expected_outputs(base, full, other_opts)
        assert any(not torch.equal(other[n], expected[n]) for n in expected if "layers" in n)


@pytest.mark.parametrize("operator,filter_wise", CLI_CASES, ids=CLI_IDS)
def test_cli_in_place_equals_the_oracle(tmp_path, emul, monkeypatch, operator, filter_wise):
    """the partitioned path merges block tensors itself (distributed._merge_block_tensor): it must run these operators too"""
    monkeypatch.setenv("SHARDMERGE_INPLACE", "1")
    monkeypatch.setattr(distributed, "ENGINE_FACTORY", lambda: emul)
    base, factors, full = lf.setup_k3(tmp_path, emul)
    opts = gc.options(operator, filter_wise)
    res = run_cli(gc.write_config(tmp_path, "org/lora", "merged", opts))
    assert res.exit_code == 0, res.output
    assert_outputs(tmp_path / "merged", gc.expected_outputs(base, full, opts))
    assert gc.README_WORDS[operator][0] in (tmp_path / "merged" / "README.md").read_text()


@pytest.mark.parametrize("operator,filter_wise", CLI_CASES, ids=CLI_IDS)
def test_two_gloo_ranks_equal_the_oracle(tmp_path, emul, operator, filter_wise):
    base, factors, full = lf.setup_k3(tmp_path, emul)
    opts = gc.options(operator, filter_wise)
    cfg = gc.write_config(tmp_path, "org/lora", "merged", opts, device="cpu")
    run_ranks(cfg)
    assert not list((tmp_path / "merged").glob(".tmp-*"))
    assert_outputs(tmp_path / "merged", gc.expected_outputs(base, full, opts))
