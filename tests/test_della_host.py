"""operator: della / della_linear without a GPU: the kernels of csrc/sm_della.hpp on the CPU work-group emulator against
tests/della_oracle.py (bit for bit, tests/della_checks.py), the YAML options and the load-time argument rules, the stamp,
and `python -m shard merge` end to end - single process, an adapter entry, in place, and two gloo ranks - with the
emulator as the device."""
import ctypes as C

import click
import pytest
import torch
import yaml

from shardmerge_amd import distributed
from shardmerge_amd.config import MergeConfig
from tests import della_checks as dc
from tests import lora_fixtures as lf
from tests.harness import DTYPES, KS, assert_outputs, emul, run_cli, run_ranks, yaml_config  # noqa: F401

OPERATORS = ("della", "della_linear")
MODE_IDS = ["della", "della_linear"]


# ---- the kernels on the emulator against the oracle ---------------------------------------------------------
@pytest.mark.parametrize("sign_election", dc.MODES, ids=MODE_IDS)
@pytest.mark.parametrize("bo_dtype", DTYPES, ids=str)
@pytest.mark.parametrize("in_dtype", DTYPES, ids=str)
def test_dtypes(emul, in_dtype, bo_dtype, sign_election):
    dc.check_dtypes(emul, in_dtype, bo_dtype, sign_election)


@pytest.mark.parametrize("sign_election", dc.MODES, ids=MODE_IDS)
@pytest.mark.parametrize("window", dc.WINDOWS, ids=lambda w: f"{w[0]:.4g}-{w[1]:g}")
@pytest.mark.parametrize("k", KS)
def test_k_and_window(emul, k, window, sign_election):
    dc.check_k_window(emul, k, window, sign_election)


@pytest.mark.parametrize("sign_election", dc.MODES, ids=MODE_IDS)
@pytest.mark.parametrize("rescale", [True, False])
@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("lam", [1.0, 0.7])
def test_lambda_normalize_rescale(emul, lam, normalize, rescale, sign_election):
    dc.check_options(emul, lam, normalize, rescale, sign_election)


@pytest.mark.parametrize("c", dc.ROW_LENGTHS)
def test_row_length(emul, c):
    dc.check_row_length(emul, c)


CORNERS = [dc.check_signed_alphas, dc.check_row_too_long, dc.check_row_contents, dc.check_zero_delta, dc.check_denormals,
           dc.check_unaligned_and_rank3, dc.check_nonfinite, dc.check_arguments, dc.check_epsilon_zero_is_dare,
           dc.check_order_independence, dc.check_monotone_and_nested, dc.check_slabs, dc.check_determinism]


@pytest.mark.parametrize("check", CORNERS, ids=lambda f: f.__name__[len("check_"):])
def test_corner(emul, check):
    check(emul)


@pytest.mark.parametrize("window", dc.STAT_WINDOWS, ids=lambda w: f"{w[0]:g}-{w[1]:g}")
def test_statistics(emul, window):
    dc.check_statistics(emul, window)


def test_c_abi_rejects_bad_arguments(emul):
    from shardmerge_amd import _lib
    x = torch.zeros(64, dtype=torch.bfloat16)
    y = torch.zeros(64, dtype=torch.bfloat16)
    out = torch.zeros(64, dtype=torch.bfloat16)
    thr = torch.zeros(64, dtype=torch.int16)

    def call(k=1, density=0.5, epsilon=0.15, out_t=out, n=64, rows=8, in_dtype=_lib.BF16, thr_t=None):
        d = _lib.DellaDesc()
        d.k = k
        for i in range(max(0, min(k, 16))):
            d.finetune[i], d.base[i], d.alpha[i], d.stream_id[i] = x.data_ptr(), y.data_ptr(), 0.5, i
        d.in_dtype, d.base_out, d.base_out_dtype, d.n = in_dtype, y.data_ptr(), _lib.BF16, n
        d.density, d.lam, d.normalize, d.key, d.rescale, d.sign_election = density, 1.0, 1, 7, 1, 1
        d.epsilon, d.rows = epsilon, rows
        rep = _lib.DellaReport()
        rc = emul.lib.dll.smhip_della_merge(emul.ctx.h, C.byref(d), out_t.data_ptr(), None, thr_t.data_ptr() if thr_t is not None else None,
                                            C.byref(rep), None)
        return rc, emul.lib.dll.smhip_last_error(emul.ctx.h).decode(), rep
    assert C.sizeof(_lib.DellaDesc) == C.sizeof(_lib.DareDesc) + 16

    rc, _, rep = call(thr_t=thr)
    assert rc == _lib.OK and (rep.T_lo, rep.T_hi) == (22937, 42598)
    assert set(thr.tolist()) == {22937}                          # all-zero deltas: every rank is 0
    rc, _, rep = call(density=2.0 ** -15 + 0.01, epsilon=0.01)
    assert rc == _lib.OK and rep.T_lo == 2
    rc, _, rep = call(density=1.0, epsilon=0.0)
    assert rc == _lib.OK and (rep.T_lo, rep.T_hi) == (65536, 65536)
    for kwargs, word in (({"k": 0}, "k out of range"), ({"k": 17}, "k out of range"), ({"density": 0.0}, "density"),
                         ({"density": 1.01}, "density"), ({"epsilon": -0.1}, "epsilon"), ({"epsilon": float("nan")}, "epsilon"),
                         ({"density": 1.0}, "requires epsilon 0"), ({"density": 0.9, "epsilon": 0.1}, "below 1"),
                         ({"density": 0.1, "epsilon": 0.1}, "at least 1"), ({"density": 2.0 ** -17, "epsilon": 0.0}, "smallest density"),
                         ({"rows": 0}, "rows"), ({"rows": 7}, "rows"), ({"out_t": x}, "overlaps"), ({"in_dtype": 3}, "dtype"),
                         ({"thr_t": out}, "threshold_out")):
        rc, msg, _ = call(**kwargs)
        assert rc == _lib.ERR_ARG and word in msg, (kwargs, rc, msg)
    big = torch.zeros(32769, dtype=torch.bfloat16)
    x, y, out = big, big.clone(), big.clone()                   # (call reads x and y when it runs; its out_t default is the short one)
    rc, msg, _ = call(n=32769, rows=1, out_t=out)
    assert rc == _lib.ERR_SHAPE and "32769" in msg and "32768" in msg, (rc, msg)
    assert call(n=32769, rows=1, epsilon=0.0, out_t=out)[0] == _lib.OK
    assert call(n=0, out_t=x)[0] == _lib.OK                     # a no-op, whatever the pointers


# ---- YAML ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("operator", OPERATORS)
def test_yaml_accepts_the_operators_and_their_keys(tmp_path, operator):
    from shardmerge_amd.merge import operator_class
    from shardmerge_amd.merge.dare import DareTiesMerge
    from shardmerge_amd.merge.della import DellaLinearMerge, DellaMerge
    from shardmerge_amd.merge.fast_fourier import FourierMerge
    cls = operator_class(operator)
    assert cls is (DellaMerge if operator == "della" else DellaLinearMerge) and issubclass(cls, DareTiesMerge)
    assert cls.sign_election is (operator == "della")
    cfg = MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": operator}))
    assert cfg.operator == operator and cfg.merge_options == {}
    m = cls(config=cfg, index_manager=object())
    assert (m.density, m.epsilon, m.della_lambda, bool(m.della_normalize), bool(m.della_rescale), m.seed) == (0.5, 0.15, 1.0, True, True, 0)
    seed = 2 ** 63 - 1
    cfg = MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": operator, "density": 1, "epsilon": 0, "della_lambda": 0.7, "della_normalize": 0,
                                                 "della_rescale": 0, "seed": seed}))
    assert cfg.merge_options == {"density": 1.0, "epsilon": 0.0, "della_lambda": 0.7, "della_normalize": 0.0, "della_rescale": 0.0, "seed": seed}
    m = cls(config=cfg, index_manager=object())
    assert (m.density, m.epsilon, m.della_lambda, bool(m.della_normalize), bool(m.della_rescale)) == (1.0, 0.0, 0.7, False, False)
    assert m.seed == seed and isinstance(m.seed, int)
    cfg = MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": operator, "density": 0.5, "epsilon": 0.15, "della_lambda": 0.7, "seed": 42}))
    readme = cls(config=cfg, index_manager=object()).get_readme()
    for word in ("DELLA", f"({operator}:", "density 0.5", "epsilon 0.15", "22937/65536", "42598/65536", "0.349991", "0.649994", "lambda 0.7",
                 "seed 42", "org/ft1"):
        assert word in readme, (word, readme)
    assert cls.merge_block is not DareTiesMerge.merge_block and cls._merge_layer is FourierMerge._merge_layer


@pytest.mark.parametrize("operator", OPERATORS)
@pytest.mark.parametrize("opts,word", [({"density": 0}, "density"), ({"density": 1.0001}, "density"), ({"density": "0.2"}, "density"),
                                       ({"epsilon": -0.01}, "epsilon"), ({"epsilon": 1}, "epsilon"), ({"epsilon": "x"}, "epsilon"), ({"epsilon": True}, "epsilon"),
                                       ({"density": 1}, "requires merge_options.epsilon 0"), ({"density": 1, "epsilon": 0.1}, "requires merge_options.epsilon 0"),
                                       ({"density": 0.9}, "must be below 1"), ({"density": 0.5, "epsilon": 0.5}, "must be below 1"),
                                       ({"density": 0.1, "epsilon": 0.1}, "at least 1"), ({"density": 2.0 ** -17, "epsilon": 0}, "at least 1"),
                                       ({"della_lambda": 1e7}, "della_lambda"), ({"della_normalize": 2}, "della_normalize"),
                                       ({"della_rescale": 0.5}, "della_rescale"), ({"seed": 1.5}, "seed"), ({"seed": -1}, "seed"), ({"seed": 2 ** 63}, "seed")])
def test_yaml_rejects_out_of_range_values(tmp_path, operator, opts, word):
    with pytest.raises(click.BadParameter, match=word):
        MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": operator, **opts}))


def test_yaml_accepts_the_corners_of_the_window(tmp_path):
    for opts in ({"density": 1, "epsilon": 0}, {"density": 0.1 + 2.0 ** -16, "epsilon": 0.1}, {"density": 2.0 ** -16, "epsilon": 0},
                 {"density": 0.7, "epsilon": 0.29}):
        MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": "della", **opts}))


@pytest.mark.parametrize("operator", [None, "fourier", "addition", "task_addition", "fourier_legacy", "ties", "dare_ties", "dare_linear",
                                      "breadcrumbs", "breadcrumbs_ties", "model_stock", "nuslerp", "slerp", "sce"])
@pytest.mark.parametrize("key", ["epsilon", "della_lambda", "della_normalize", "della_rescale"])
def test_yaml_rejects_a_della_key_with_another_operator(tmp_path, operator, key):
    opts = {key: 0}
    if operator:
        opts["operator"] = operator
    doc = yaml.safe_load(yaml_config(tmp_path, opts).read_text())
    if operator in ("nuslerp", "slerp"):
        doc["finetune_merge"] = doc["finetune_merge"] * 2
    p = tmp_path / "other.yaml"
    p.write_text(yaml.safe_dump(doc))
    with pytest.raises(click.BadParameter, match=f"{key}.*della or della_linear"):
        MergeConfig.from_yaml(p)


@pytest.mark.parametrize("operator", OPERATORS)
@pytest.mark.parametrize("key,value", [("cutoff_pct", 0.08), ("cull_start_pct", 0.2), ("t_sum", 1.0), ("target_norm_offset", 1e-10),
                                       ("b", 0.1), ("norm_mode", "exact"), ("task_add_models", ["org/ft1"]), ("ties_lambda", 1.0),
                                       ("ties_normalize", 1), ("dare_lambda", 1.0), ("dare_normalize", 1), ("dare_rescale", 1), ("gamma", 0.01),
                                       ("breadcrumbs_lambda", 1.0), ("stock_filter_wise", 1), ("select_topk", 0.5), ("sce_lambda", 1.0),
                                       ("bogus", 1)])
def test_yaml_rejects_an_option_della_would_ignore(tmp_path, operator, key, value):
    with pytest.raises(click.BadParameter, match=key):
        MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": operator, key: value}))


def test_config_stamp(tmp_path):
    stamp = lambda opts: distributed.config_stamp(MergeConfig.from_yaml(yaml_config(tmp_path, opts)))
    full = {"operator": "della", "density": 0.5, "epsilon": 0.15, "della_lambda": 1.0, "della_normalize": 1, "della_rescale": 1, "seed": 2 ** 62}
    base = stamp(full)
    assert base == stamp(dict(full))
    others = [stamp({**full, "operator": "della_linear"}), stamp({**full, "density": 0.3}), stamp({**full, "epsilon": 0.1}),
              stamp({**full, "della_lambda": 0.9}), stamp({**full, "della_normalize": 0}), stamp({**full, "della_rescale": 0}),
              stamp({**full, "seed": 2 ** 62 + 1}), stamp({**full, "seed": 0}), stamp({"operator": "dare_ties", "density": 0.5}), stamp(None)]
    assert len({base, *others}) == len(others) + 1


# ---- the CLI end to end ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("operator", OPERATORS)
def test_cli_equals_the_oracle_tensor_by_tensor(tmp_path, emul, operator):
    base, factors, full = lf.setup_k3(tmp_path, emul)
    opts = dc.options(operator)
    expected = dc.expected_outputs(base, full, opts)
    assert any(not torch.equal(expected[n], base[n]) for n in expected if "layers" in n)
    res = run_cli(dc.write_config(tmp_path, "org/lora_full", "merged", opts))
    assert res.exit_code == 0, res.output
    assert_outputs(tmp_path / "merged", expected)
    readme = (tmp_path / "merged" / "README.md").read_text()
    for word in ("DELLA", operator, "density 0.4", "epsilon 0.2", "13107/65536", "39321/65536", "lambda 0.7", f"seed {opts['seed']}"):
        assert word in readme, (word, readme)
    # one finetune given as a LoRA adapter directory: the run on its materialised checkpoint
    res = run_cli(dc.write_config(tmp_path, "org/lora", "merged_adapter", opts))
    assert res.exit_code == 0, res.output
    lf.assert_same_outputs(tmp_path / "merged_adapter", tmp_path / "merged")
    # the default options
    res = run_cli(dc.write_config(tmp_path, "org/lora_full", "merged_default", {"operator": operator}))
    assert res.exit_code == 0, res.output
    assert_outputs(tmp_path / "merged_default", dc.expected_outputs(base, full, {"operator": operator}))
    # no window: the DARE operator of the same mode, byte for byte
    from tests import dare_checks
    dare = {"operator": "dare_ties" if operator == "della" else "dare_linear", "density": 0.4, "dare_lambda": 0.7, "seed": opts["seed"]}
    res = run_cli(dc.write_config(tmp_path, "org/lora_full", "merged_flat", {**opts, "epsilon": 0}))
    assert res.exit_code == 0, res.output
    assert_outputs(tmp_path / "merged_flat", dare_checks.expected_outputs(base, full, dare))


@pytest.mark.parametrize("operator", OPERATORS)
def test_cli_in_place_equals_the_oracle(tmp_path, emul, monkeypatch, operator):
    """the partitioned path merges block tensors itself (distributed._merge_block_tensor): the same ranks and mask there"""
    monkeypatch.setenv("SHARDMERGE_INPLACE", "1")
    monkeypatch.setattr(distributed, "ENGINE_FACTORY", lambda: emul)
    base, factors, full = lf.setup_k3(tmp_path, emul)
    opts = dc.options(operator)
    res = run_cli(dc.write_config(tmp_path, "org/lora", "merged", opts))
    assert res.exit_code == 0, res.output
    assert_outputs(tmp_path / "merged", dc.expected_outputs(base, full, opts))
    assert "DELLA" in (tmp_path / "merged" / "README.md").read_text()


@pytest.mark.parametrize("operator", OPERATORS)
def test_two_gloo_ranks_equal_the_oracle(tmp_path, emul, operator):
    base, factors, full = lf.setup_k3(tmp_path, emul)
    opts = dc.options(operator)
    cfg = dc.write_config(tmp_path, "org/lora", "merged", opts, device="cpu")
    run_ranks(cfg)
    assert not list((tmp_path / "merged").glob(".tmp-*"))
    assert_outputs(tmp_path / "merged", dc.expected_outputs(base, full, opts))
