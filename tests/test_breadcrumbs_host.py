"""operator: breadcrumbs / breadcrumbs_ties without a GPU: the kernels of csrc/sm_breadcrumbs.hpp on the CPU work-group
emulator against tests/breadcrumbs_oracle.py (bit for bit, tests/breadcrumbs_checks.py), the YAML options, the stamp, and
`python -m shard merge` end to end - single process, in place, and two gloo ranks - with the emulator as the device."""
import ctypes as C

import click
import pytest
import torch

from shardmerge_amd import distributed
from shardmerge_amd.config import MergeConfig
from tests import breadcrumbs_checks as bc
from tests import lora_fixtures as lf
from tests.harness import ALPHAS, DTYPES, KS, assert_outputs, emul, make_inputs, run_cli, run_ranks, yaml_config  # noqa: F401

OPERATORS = ("breadcrumbs", "breadcrumbs_ties")
MODE_IDS = ["breadcrumbs_ties", "breadcrumbs"]


# ---- the kernels on the emulator against the oracle ---------------------------------------------------------
@pytest.mark.parametrize("sign_election", bc.MODES, ids=MODE_IDS)
@pytest.mark.parametrize("bo_dtype", DTYPES, ids=str)
@pytest.mark.parametrize("in_dtype", DTYPES, ids=str)
def test_dtypes(emul, in_dtype, bo_dtype, sign_election):
    bc.check_dtypes(emul, in_dtype, bo_dtype, sign_election)


@pytest.mark.parametrize("sign_election", bc.MODES, ids=MODE_IDS)
@pytest.mark.parametrize("density,gamma", bc.DENSITY_GAMMA)
@pytest.mark.parametrize("k", KS)
def test_k_density_gamma(emul, k, density, gamma, sign_election):
    bc.check_k_density_gamma(emul, k, density, gamma, sign_election)


@pytest.mark.parametrize("sign_election", bc.MODES, ids=MODE_IDS)
@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("lam", [1.0, 0.7])
def test_lambda_and_normalize(emul, lam, normalize, sign_election):
    bc.check_lambda_normalize(emul, lam, normalize, sign_election)


@pytest.mark.parametrize("check", bc.CORNERS, ids=lambda f: f.__name__[len("check_"):])
def test_corner(emul, check):
    check(emul)


def test_largest_emulator_shape(emul):
    fts, bases, bo = make_inputs((512, 1024), 3, seed=5, own_bases=True)
    bc.check(emul, fts, bases, ALPHAS[:3], bo, density=0.2, gamma=0.01, lam=0.7, sign_election=True, label="512 x 1024")


@pytest.mark.parametrize("k,expected", [(2, {"crumbs_hist": 3, "crumbs_select": 3, "crumbs_merge": 1}),
                                        (5, {"crumbs_hist": 6, "crumbs_select": 3, "crumbs_merge": 1})], ids=["k2", "k5"])
def test_profile_names_and_launches(emul, k, expected):
    """one histogram launch per group of four finetunes and level, one select launch per level: both ranks in the same passes"""
    bc.check_profile(emul, k, expected)


def test_c_abi_rejects_bad_arguments(emul):
    from shardmerge_amd import _lib
    x = torch.zeros(64, dtype=torch.bfloat16)
    y = torch.zeros(64, dtype=torch.bfloat16)
    out = torch.zeros(64, dtype=torch.bfloat16)

    def call(k=1, density=0.2, gamma=0.01, out_t=out, n=64, in_dtype=_lib.BF16, lam=1.0, alpha=0.5):
        d = _lib.BreadcrumbsDesc()
        d.k = k
        for i in range(max(0, min(k, 16))):
            d.finetune[i], d.base[i], d.alpha[i] = x.data_ptr(), y.data_ptr(), alpha
        d.in_dtype, d.base_out, d.base_out_dtype, d.n = in_dtype, y.data_ptr(), _lib.BF16, n
        d.density, d.lam, d.normalize, d.gamma, d.sign_election = density, lam, 1, gamma, 1
        rep = _lib.BreadcrumbsReport()
        rc = emul.lib.dll.smhip_breadcrumbs_merge(emul.ctx.h, C.byref(d), out_t.data_ptr(), None, C.byref(rep), None)
        return rc, emul.lib.dll.smhip_last_error(emul.ctx.h).decode(), rep

    rc, _, rep = call()
    assert rc == _lib.OK and (rep.k_keep, rep.n_top) == (12, 0)
    rc, _, rep = call(density=0.5, gamma=0.5)
    assert rc == _lib.OK and (rep.k_keep, rep.n_top) == (32, 32)
    for kwargs, word in (({"k": 0}, "k out of range"), ({"k": 17}, "k out of range"), ({"density": 0.0}, "density"),
                         ({"density": 1.01}, "density"), ({"gamma": -0.01}, "gamma"), ({"gamma": 1.0}, "gamma"),
                         ({"gamma": float("nan")}, "gamma"), ({"density": 0.9, "gamma": 0.2}, "density + gamma"),
                         ({"lam": float("inf")}, "lambda"), ({"alpha": float("nan")}, "alpha"),
                         ({"out_t": x}, "overlaps"), ({"in_dtype": 3}, "dtype")):
        rc, msg, _ = call(**kwargs)
        assert rc == _lib.ERR_ARG and word in msg, (kwargs, rc, msg)
    rc = emul.lib.dll.smhip_breadcrumbs_merge(emul.ctx.h, None, out.data_ptr(), None, None, None)
    assert rc == _lib.ERR_ARG and "null descriptor" in emul.lib.dll.smhip_last_error(emul.ctx.h).decode()
    assert call(n=0, out_t=x)[0] == _lib.OK                     # a no-op, whatever the pointers


# ---- YAML ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("operator", OPERATORS)
def test_yaml_accepts_the_operators_and_their_keys(tmp_path, operator):
    from shardmerge_amd.merge import operator_class
    from shardmerge_amd.merge.breadcrumbs import BreadcrumbsMerge, BreadcrumbsTiesMerge
    from shardmerge_amd.merge.fast_fourier import FourierMerge
    from shardmerge_amd.merge.ties import TiesMerge
    cls = operator_class(operator)
    assert cls is (BreadcrumbsTiesMerge if operator == "breadcrumbs_ties" else BreadcrumbsMerge) and issubclass(cls, TiesMerge)
    assert cls.sign_election is (operator == "breadcrumbs_ties")
    cfg = MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": operator}))
    assert cfg.operator == operator and cfg.merge_options == {}
    m = cls(config=cfg, index_manager=object())
    assert (m.density, m.gamma, m.breadcrumbs_lambda, bool(m.breadcrumbs_normalize)) == (0.9, 0.01, 1.0, True)
    cfg = MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": operator, "density": 1, "gamma": 0, "breadcrumbs_lambda": 0.7,
                                                 "breadcrumbs_normalize": 0}))
    assert cfg.merge_options == {"density": 1.0, "gamma": 0.0, "breadcrumbs_lambda": 0.7, "breadcrumbs_normalize": 0.0}
    m = cls(config=cfg, index_manager=object())
    assert (m.density, m.gamma, m.breadcrumbs_lambda, bool(m.breadcrumbs_normalize)) == (1.0, 0.0, 0.7, False)
    cfg = MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": operator, "density": 0.2, "gamma": 0.05, "breadcrumbs_lambda": 0.7}))
    readme = cls(config=cfg, index_manager=object()).get_readme()
    for word in ("# Breadcrumbs Merged Model", operator + ":", "density 0.2", "gamma 0.05", "lambda 0.7", "org/ft1",
                 "agreeing weights" if operator == "breadcrumbs_ties" else "sum of the weights"):
        assert word in readme, (word, readme)
    assert MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": operator, "density": 0.5, "gamma": 0.5})).merge_options == \
        {"density": 0.5, "gamma": 0.5}
    # the one method both paths call is what differs; the cost model is TIES's
    assert cls.merge_block is not TiesMerge.merge_block and cls._merge_layer is FourierMerge._merge_layer
    assert m.block_cost_ms((128, 64), 3) == TiesMerge.block_cost_ms(m, (128, 64), 3)


@pytest.mark.parametrize("operator", OPERATORS)
@pytest.mark.parametrize("options", [{"density": 0}, {"density": -0.1}, {"density": 1.0001}, {"density": "0.2"}, {"density": True},
                                     {"gamma": -0.01}, {"gamma": 1}, {"gamma": 1.5}, {"gamma": "0.01"}, {"gamma": True},
                                     {"gamma": float("nan")},
                                     {"breadcrumbs_lambda": 1e7}, {"breadcrumbs_lambda": -1e7}, {"breadcrumbs_lambda": "x"},
                                     {"breadcrumbs_normalize": 2}, {"breadcrumbs_normalize": 0.5}, {"breadcrumbs_normalize": -1},
                                     {"breadcrumbs_normalize": "yes"}], ids=str)
def test_yaml_rejects_out_of_range_values(tmp_path, operator, options):
    (key, _), = options.items()
    with pytest.raises(click.BadParameter, match=key):
        MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": operator, **options}))


@pytest.mark.parametrize("operator", OPERATORS)
@pytest.mark.parametrize("options", [{"density": 0.9, "gamma": 0.2}, {"density": 1}, {"gamma": 0.11}, {"density": 0.5, "gamma": 0.5000001}],
                         ids=str)
def test_yaml_rejects_density_plus_gamma_above_one(tmp_path, operator, options):
    """(the defaults take part: density 1 with the default gamma 0.01 is out of range)"""
    with pytest.raises(click.BadParameter) as e:
        MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": operator, **options}))
    assert "density" in str(e.value) and "gamma" in str(e.value)


@pytest.mark.parametrize("operator", [None, "fourier", "addition", "task_addition", "fourier_legacy", "ties", "dare_ties", "dare_linear"])
@pytest.mark.parametrize("key", ["gamma", "breadcrumbs_lambda", "breadcrumbs_normalize"])
def test_yaml_rejects_a_breadcrumbs_key_with_another_operator(tmp_path, operator, key):
    opts = {key: 0}
    if operator:
        opts["operator"] = operator
    with pytest.raises(click.BadParameter, match=rf"merge_options\.{key} is accepted only with operator: breadcrumbs"):
        MergeConfig.from_yaml(yaml_config(tmp_path, opts))


@pytest.mark.parametrize("operator", OPERATORS)
@pytest.mark.parametrize("key,value", [("cutoff_pct", 0.08), ("cull_start_pct", 0.2), ("t_sum", 1.0), ("target_norm_offset", 1e-10),
                                       ("b", 0.1), ("norm_mode", "exact"), ("task_add_models", ["org/ft1"]), ("ties_lambda", 1.0),
                                       ("ties_normalize", 1), ("dare_lambda", 1.0), ("dare_normalize", 1), ("dare_rescale", 1),
                                       ("seed", 0), ("bogus", 1)])
def test_yaml_rejects_an_option_breadcrumbs_would_ignore(tmp_path, operator, key, value):
    with pytest.raises(click.BadParameter, match=key):
        MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": operator, key: value}))


def test_config_stamp(tmp_path):
    stamp = lambda opts: distributed.config_stamp(MergeConfig.from_yaml(yaml_config(tmp_path, opts)))
    full = {"operator": "breadcrumbs", "density": 0.9, "gamma": 0.01, "breadcrumbs_lambda": 1.0, "breadcrumbs_normalize": 1}
    base = stamp(full)
    assert base == stamp(dict(full))
    others = [stamp({**full, "operator": "breadcrumbs_ties"}), stamp({**full, "density": 0.8}), stamp({**full, "gamma": 0.02}),
              stamp({**full, "breadcrumbs_lambda": 0.9}), stamp({**full, "breadcrumbs_normalize": 0}),
              stamp({"operator": "ties", "density": 0.9}), stamp({"operator": "dare_linear", "density": 0.9}), stamp(None)]
    assert len({base, *others}) == len(others) + 1


# ---- the CLI end to end ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("operator", OPERATORS)
def test_cli_equals_the_oracle_tensor_by_tensor(tmp_path, emul, operator):
    base, factors, full = lf.setup_k3(tmp_path, emul)
    opts = bc.options(operator)
    expected = bc.expected_outputs(base, full, opts)
    assert any(not torch.equal(expected[n], base[n]) for n in expected if "layers" in n)
    res = run_cli(bc.write_config(tmp_path, "org/lora_full", "merged", opts))
    assert res.exit_code == 0, res.output
    assert_outputs(tmp_path / "merged", expected)
    readme = (tmp_path / "merged" / "README.md").read_text()
    for word in ("# Breadcrumbs Merged Model", operator + ":", "density 0.3", "gamma 0.05", "lambda 0.7"):
        assert word in readme, (word, readme)
    # one finetune given as a LoRA adapter directory: the run on its materialised checkpoint
    res = run_cli(bc.write_config(tmp_path, "org/lora", "merged_adapter", opts))
    assert res.exit_code == 0, res.output
    lf.assert_same_outputs(tmp_path / "merged_adapter", tmp_path / "merged")
    # the default options
    res = run_cli(bc.write_config(tmp_path, "org/lora_full", "merged_default", {"operator": operator}))
    assert res.exit_code == 0, res.output
    assert_outputs(tmp_path / "merged_default", bc.expected_outputs(base, full, {"operator": operator}))
    # the upper cut shows in the output: gamma 0 is another model
    res = run_cli(bc.write_config(tmp_path, "org/lora_full", "merged_gamma0", {**opts, "gamma": 0}))
    assert res.exit_code == 0, res.output
    other = lf.read_outputs(tmp_path / "merged_gamma0")
    assert any(not torch.equal(other[n], expected[n]) for n in expected if "layers" in n)
    assert_outputs(tmp_path / "merged_gamma0", bc.expected_outputs(base, full, {**opts, "gamma": 0}))


@pytest.mark.parametrize("operator", OPERATORS)
def test_cli_in_place_equals_the_oracle(tmp_path, emul, monkeypatch, operator):
    """the partitioned path merges block tensors itself (distributed._merge_block_tensor): it must run Breadcrumbs too"""
    monkeypatch.setenv("SHARDMERGE_INPLACE", "1")
    monkeypatch.setattr(distributed, "ENGINE_FACTORY", lambda: emul)
    base, factors, full = lf.setup_k3(tmp_path, emul)
    opts = bc.options(operator)
    res = run_cli(bc.write_config(tmp_path, "org/lora", "merged", opts))
    assert res.exit_code == 0, res.output
    assert_outputs(tmp_path / "merged", bc.expected_outputs(base, full, opts))
    assert "Breadcrumbs" in (tmp_path / "merged" / "README.md").read_text()


@pytest.mark.parametrize("operator", OPERATORS)
def test_two_gloo_ranks_equal_the_oracle(tmp_path, emul, operator):
    base, factors, full = lf.setup_k3(tmp_path, emul)
    opts = bc.options(operator)
    cfg = bc.write_config(tmp_path, "org/lora", "merged", opts, device="cpu")
    run_ranks(cfg)
    assert not list((tmp_path / "merged").glob(".tmp-*"))
    assert_outputs(tmp_path / "merged", bc.expected_outputs(base, full, opts))
