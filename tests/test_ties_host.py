"""operator: ties without a GPU: the kernels of csrc/sm_ties.hpp on the CPU work-group emulator against
tests/ties_oracle.py (bit for bit, tests/ties_checks.py), the YAML options, the stamp, and `python -m shard merge`
end to end - single process, in place, and two gloo ranks - with the emulator as the device."""
import json
import re

import click
import pytest
import torch
import yaml
from click.testing import CliRunner

from shardmerge_amd import distributed
from shardmerge_amd.config import MergeConfig
from tests import lora_fixtures as lf
from tests import ties_checks as tc
from tests import ties_oracle
from tests.harness import (ALPHAS, DTYPES, KS, assert_outputs, emul, make_inputs, run_cli, run_ranks, ties_models,  # noqa: F401
                           yaml_config)


# ---- the kernels on the emulator against the oracle ---------------------------------------------------------
@pytest.mark.parametrize("bo_dtype", DTYPES, ids=str)
@pytest.mark.parametrize("in_dtype", DTYPES, ids=str)
def test_dtypes(emul, in_dtype, bo_dtype):
    tc.check_dtypes(emul, in_dtype, bo_dtype)


@pytest.mark.parametrize("density", tc.DENSITIES)
@pytest.mark.parametrize("k", KS)
def test_k_and_density(emul, k, density):
    tc.check_k_density(emul, k, density)


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("lam", [1.0, 0.7])
def test_lambda_and_normalize(emul, lam, normalize):
    tc.check_lambda_normalize(emul, lam, normalize)


@pytest.mark.parametrize("check", [tc.check_signed_alphas, tc.check_zero_delta, tc.check_opposite_deltas,
                                   tc.check_tiny_weight_sum, tc.check_ties_exceed_k, tc.check_denormals, tc.check_unaligned,
                                   tc.check_tiny_and_rank3, tc.check_nonfinite, tc.check_determinism, tc.check_arguments],
                         ids=lambda f: f.__name__[len("check_"):])
def test_corner(emul, check):
    check(emul)


def test_largest_emulator_shape(emul):
    fts, bases, bo = make_inputs((512, 1024), 3, seed=5, own_bases=True)
    tc.check(emul, fts, bases, ALPHAS[:3], bo, density=0.2, lam=0.7, label="512 x 1024")


def test_profile_names_and_launches(emul):
    """K = 5: two groups of finetunes per selection level"""
    fts, bases, bo = make_inputs((40, 50), 5, seed=6)
    emul.ctx.profile(True)
    emul.ctx.profile_reset()
    try:
        emul.ties_merge(fts, bases, ALPHAS[:5], bo)
        table = emul.ctx.profile_table()
    finally:
        emul.ctx.profile(False)
    assert {n: table[n][0] for n in ("ties_hist", "ties_select", "ties_merge")} == {"ties_hist": 6, "ties_select": 3, "ties_merge": 1}
    assert set(table) == {"ties_hist", "ties_select", "ties_merge"}


def test_c_abi_rejects_bad_arguments(emul):
    import ctypes as C
    from shardmerge_amd import _lib
    x = torch.zeros(64, dtype=torch.bfloat16)
    y = torch.zeros(64, dtype=torch.bfloat16)
    out = torch.zeros(64, dtype=torch.bfloat16)

    def call(k=1, density=0.2, out_t=out, n=64, in_dtype=_lib.BF16):
        d = _lib.TiesDesc()
        d.k = k
        for i in range(max(0, min(k, 16))):
            d.finetune[i], d.base[i], d.alpha[i] = x.data_ptr(), y.data_ptr(), 0.5
        d.in_dtype, d.base_out, d.base_out_dtype, d.n = in_dtype, y.data_ptr(), _lib.BF16, n
        d.density, d.lam, d.normalize = density, 1.0, 1
        rc = emul.lib.dll.smhip_ties_merge(emul.ctx.h, C.byref(d), out_t.data_ptr(), None, None, None)
        return rc, emul.lib.dll.smhip_last_error(emul.ctx.h).decode()

    assert call()[0] == _lib.OK
    for kwargs, word in (({"k": 0}, "k out of range"), ({"k": 17}, "k out of range"), ({"density": 0.0}, "density"),
                         ({"density": 1.01}, "density"), ({"out_t": x}, "overlaps"), ({"in_dtype": 3}, "dtype")):
        rc, msg = call(**kwargs)
        assert rc == _lib.ERR_ARG and word in msg, (kwargs, rc, msg)
    assert call(n=0, out_t=x)[0] == _lib.OK                     # a no-op, whatever the pointers


# ---- YAML ------------------------------------------------------------------------------------------------------
def test_yaml_accepts_the_operator_and_its_keys(tmp_path):
    from shardmerge_amd.merge import operator_class
    from shardmerge_amd.merge.fast_fourier import FourierMerge
    from shardmerge_amd.merge.ties import TiesMerge
    assert operator_class("ties") is TiesMerge
    cfg = MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": "ties"}))
    assert cfg.operator == "ties" and cfg.merge_options == {}
    m = TiesMerge(config=cfg, index_manager=object())
    assert (m.density, m.ties_lambda, bool(m.ties_normalize)) == (0.2, 1.0, True)
    cfg = MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": "ties", "density": 1, "ties_lambda": 0.7, "ties_normalize": 0}))
    assert cfg.merge_options == {"density": 1.0, "ties_lambda": 0.7, "ties_normalize": 0.0}
    m = TiesMerge(config=cfg, index_manager=object())
    assert (m.density, m.ties_lambda, bool(m.ties_normalize)) == (1.0, 0.7, False)
    readme = m.get_readme()
    assert "TIES" in readme and "density 1" in readme and "lambda 0.7" in readme and "org/ft1" in readme
    # the spectral operator's merge is what it was: TiesMerge overrides the one method both paths call
    assert TiesMerge.merge_block is not FourierMerge.merge_block and TiesMerge._merge_layer is FourierMerge._merge_layer


@pytest.mark.parametrize("key,value", [("density", 0), ("density", -0.1), ("density", 1.0001), ("density", "0.2"), ("density", True),
                                       ("ties_lambda", 1e7), ("ties_lambda", -1e7), ("ties_lambda", "x"),
                                       ("ties_normalize", 2), ("ties_normalize", 0.5), ("ties_normalize", -1), ("ties_normalize", "yes")])
def test_yaml_rejects_out_of_range_values(tmp_path, key, value):
    with pytest.raises(click.BadParameter, match=key):
        MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": "ties", key: value}))


@pytest.mark.parametrize("operator", [None, "fourier", "addition", "task_addition", "fourier_legacy"])
@pytest.mark.parametrize("key", ["density", "ties_lambda", "ties_normalize"])
def test_yaml_rejects_a_ties_key_with_another_operator(tmp_path, operator, key):
    opts = {key: 1}
    if operator:
        opts["operator"] = operator
    with pytest.raises(click.BadParameter, match=key):
        MergeConfig.from_yaml(yaml_config(tmp_path, opts))


@pytest.mark.parametrize("key,value", [("cutoff_pct", 0.08), ("cull_start_pct", 0.2), ("t_sum", 1.0), ("target_norm_offset", 1e-10),
                                       ("b", 0.1), ("norm_mode", "exact"), ("task_add_models", ["org/ft1"]), ("bogus", 1)])
def test_yaml_rejects_an_option_ties_would_ignore(tmp_path, key, value):
    with pytest.raises(click.BadParameter, match=key):
        MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": "ties", key: value}))


def test_config_stamp(tmp_path):
    stamp = lambda opts: distributed.config_stamp(MergeConfig.from_yaml(yaml_config(tmp_path, opts)))
    base = stamp({"operator": "ties", "density": 0.2, "ties_lambda": 1.0, "ties_normalize": 1})
    assert base == stamp({"operator": "ties", "density": 0.2, "ties_lambda": 1.0, "ties_normalize": 1})
    others = [stamp({"operator": "ties", "density": 0.3, "ties_lambda": 1.0, "ties_normalize": 1}),
              stamp({"operator": "ties", "density": 0.2, "ties_lambda": 0.9, "ties_normalize": 1}),
              stamp({"operator": "ties", "density": 0.2, "ties_lambda": 1.0, "ties_normalize": 0}),
              stamp(None)]
    assert len({base, *others}) == 5
    # a configuration without operator: ties stamps as it always did
    import hashlib
    from dataclasses import asdict
    from shardmerge_amd.constants import DEFAULT_NORM_MODE
    cfg = MergeConfig.from_yaml(yaml_config(tmp_path, {"cutoff_pct": 0.05}))
    doc = {"output_base_model": cfg.output_base_model, "output_dtype": cfg.output_dtype,
           "finetune_merge": [asdict(m) for m in cfg.finetune_merge], "merge_options": {"cutoff_pct": 0.05},
           "operator": "fourier", "norm_mode": DEFAULT_NORM_MODE}
    assert distributed.config_stamp(cfg) == hashlib.sha256(json.dumps(doc, sort_keys=True, default=str).encode()).hexdigest()[:16]


# ---- the CLI end to end ------------------------------------------------------------------------------------------
def test_cli_equals_the_oracle_tensor_by_tensor(tmp_path, emul):
    base, factors, full = lf.setup_k3(tmp_path, emul)
    expected = tc.expected_outputs(base, full)
    assert any(not torch.equal(expected[n], base[n]) for n in expected if "layers" in n)
    res = run_cli(tc.write_config(tmp_path, "org/lora_full", "merged"))
    assert res.exit_code == 0, res.output
    assert_outputs(tmp_path / "merged", expected)
    readme = (tmp_path / "merged" / "README.md").read_text()
    assert "TIES" in readme and "density 0.3" in readme and "lambda 0.7" in readme
    # one finetune given as a LoRA adapter directory: the run on its materialised checkpoint
    res = run_cli(tc.write_config(tmp_path, "org/lora", "merged_adapter"))
    assert res.exit_code == 0, res.output
    lf.assert_same_outputs(tmp_path / "merged_adapter", tmp_path / "merged")
    # the default options
    res = run_cli(tc.write_config(tmp_path, "org/lora_full", "merged_default", {"operator": "ties"}))
    assert res.exit_code == 0, res.output
    assert_outputs(tmp_path / "merged_default", tc.expected_outputs(base, full, {}))


def test_cli_in_place_equals_the_oracle(tmp_path, emul, monkeypatch):
    """the partitioned path merges block tensors itself (distributed._merge_block_tensor): it must run TIES too"""
    monkeypatch.setenv("SHARDMERGE_INPLACE", "1")
    monkeypatch.setattr(distributed, "ENGINE_FACTORY", lambda: emul)
    base, factors, full = lf.setup_k3(tmp_path, emul)
    res = run_cli(tc.write_config(tmp_path, "org/lora", "merged"))
    assert res.exit_code == 0, res.output
    assert_outputs(tmp_path / "merged", tc.expected_outputs(base, full))
    assert "TIES" in (tmp_path / "merged" / "README.md").read_text()


def test_two_gloo_ranks_equal_the_oracle(tmp_path, emul):
    base, factors, full = lf.setup_k3(tmp_path, emul)
    cfg = tc.write_config(tmp_path, "org/lora", "merged", device="cpu")
    run_ranks(cfg)
    assert not list((tmp_path / "merged").glob(".tmp-*"))
    assert_outputs(tmp_path / "merged", tc.expected_outputs(base, full))


def test_uncovered_layer_is_the_same_error(tmp_path, emul, caplog):
    lf.setup_k3(tmp_path, emul)
    models = ties_models("org/lora_full")
    for m in models:
        m["end_layer"] = 0                              # nobody covers layer 1
    cfg = yaml.safe_load(tc.write_config(tmp_path, "org/lora_full", "merged").read_text())
    cfg["finetune_merge"] = models
    p = tmp_path / "uncovered.yaml"
    p.write_text(yaml.safe_dump(cfg))
    res = run_cli(p)
    assert res.exit_code != 0
    assert any("No finetune covers layer 1" in r.getMessage() for r in caplog.records) or "No finetune covers layer 1" in str(res.exception)
