"""operator: dare_ties / dare_linear without a GPU: the generator's known answers, the kernel of csrc/sm_dare.hpp on
the CPU work-group emulator against tests/dare_oracle.py (bit for bit, tests/dare_checks.py), the mask helper at 64-bit
indices, the YAML options, the stamp, and `python -m shard merge` end to end - single process, in place, and two gloo
ranks - with the emulator as the device."""
import ctypes as C
import fcntl
import os
import subprocess
from pathlib import Path

import click
import numpy as np
import pytest
import torch
import yaml

from shardmerge_amd import distributed
from shardmerge_amd.config import MergeConfig
from tests import dare_checks as dc
from tests import dare_oracle
from tests import lora_fixtures as lf
from tests.harness import ALPHAS, DTYPES, KS, assert_outputs, emul, make_inputs, run_cli, run_ranks, yaml_config  # noqa: F401

REPO = Path(__file__).resolve().parents[1]
OPERATORS = ("dare_ties", "dare_linear")
MODE_IDS = ["dare_ties", "dare_linear"]


# ---- the generator ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counter,key,expected", dare_oracle.KNOWN_ANSWERS, ids=["zeros", "ones", "pi"])
def test_oracle_philox_known_answers(counter, key, expected):
    got = dare_oracle.philox4x32_10(*[np.array([c], dtype=np.uint64) for c in counter], key[0], key[1])
    assert tuple(int(w[0]) for w in got) == expected


def test_oracle_draws_follow_the_definition():
    """h of element j: word (j & 7) >> 1 of the block of octet j >> 3, its low half for even j"""
    key, sid = 0x299f31d0a4093822, 0x13198a2e
    blk = dare_oracle.philox4x32_10(*[np.array([c], dtype=np.uint64) for c in (5, 0, sid, 0)], key & 0xFFFFFFFF, key >> 32)
    h = dare_oracle.draws(key, sid, 5, 1)
    for e in range(8):
        w = int(blk[e >> 1][0])
        assert int(h[e]) == ((w >> 16) if e & 1 else (w & 0xFFFF))
    assert dare_oracle.threshold(1.0) == 65536 and dare_oracle.threshold(0.2) == 13107 and dare_oracle.threshold(2.0 ** -16) == 1
    assert dare_oracle.tensor_key(0, "model.layers.3.mlp.up_proj.weight") == int.from_bytes(
        __import__("hashlib").sha256(b"0\nmodel.layers.3.mlp.up_proj.weight").digest()[:8], "little")


def _probe():
    """tests/emul/dare_mask_probe.cpp built with g++ the way tests/emul/loader.py builds the emulator"""
    here = REPO / "tests" / "emul"
    so, src = here / "libdare_mask_probe.so", here / "dare_mask_probe.cpp"
    csrc = REPO / "shardmerge_amd" / "csrc"
    newest = max(p.stat().st_mtime for p in [src] + sorted(csrc.glob("*.hpp")))
    stale = lambda: not so.exists() or so.stat().st_mtime < newest
    if stale():
        with open(here / ".build.lock", "w") as lock:
            fcntl.flock(lock, fcntl.LOCK_EX)
            if stale():
                tmp = so.with_suffix(f".so.{os.getpid()}.tmp")
                subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-variable",
                                str(src), "-o", str(tmp)], check=True)
                os.replace(tmp, so)
    dll = C.CDLL(str(so))
    dll.dare_mask_probe.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64), C.c_int, C.POINTER(C.c_uint8)]
    dll.dare_mask_probe.restype = None
    return dll


def test_mask_helper_at_64_bit_indices():
    """the ONE mask helper of sm_dare.hpp against the oracle where no tensor reaches: the counter's high word"""
    dll = _probe()
    js = [0, 7, 8, 2 ** 32 - 1, 2 ** 35 + 5, 2 ** 40 + 3]
    js += [j + e for j in (2 ** 35, 2 ** 40, 2 ** 63) for e in range(8)]          # whole octets beyond 2^32 octets
    arr = (C.c_uint64 * len(js))(*js)
    keep = (C.c_uint8 * len(js))()
    seen = set()
    for key in (0, dc.KEY, dc.STAT_KEY, 2 ** 64 - 1):
        for sid in (0, 3, 2 ** 32 - 1):
            for T in [dare_oracle.threshold(d) for d in dc.DENSITIES] + [32768, 65535]:
                dll.dare_mask_probe(key, sid, T, arr, len(js), keep)
                want = [int(dare_oracle.keep_bit(key, sid, j, T)) for j in js]
                assert list(keep) == want, (key, sid, T)
                seen.add(tuple(want))
    assert len(seen) > 20                        # (the bits do depend on key, stream and T)
    # the high word matters: octet 2^32 is not octet 0
    assert not np.array_equal(dare_oracle.draws(dc.KEY, 0, 0, 1), dare_oracle.draws(dc.KEY, 0, 2 ** 32, 1))


# ---- the kernel on the emulator against the oracle ----------------------------------------------------------
@pytest.mark.parametrize("sign_election", dc.MODES, ids=MODE_IDS)
@pytest.mark.parametrize("bo_dtype", DTYPES, ids=str)
@pytest.mark.parametrize("in_dtype", DTYPES, ids=str)
def test_dtypes(emul, in_dtype, bo_dtype, sign_election):
    dc.check_dtypes(emul, in_dtype, bo_dtype, sign_election)


@pytest.mark.parametrize("sign_election", dc.MODES, ids=MODE_IDS)
@pytest.mark.parametrize("density", dc.DENSITIES)
@pytest.mark.parametrize("k", KS)
def test_k_and_density(emul, k, density, sign_election):
    dc.check_k_density(emul, k, density, sign_election)


@pytest.mark.parametrize("sign_election", dc.MODES, ids=MODE_IDS)
@pytest.mark.parametrize("rescale", [True, False])
@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("lam", [1.0, 0.7])
def test_lambda_normalize_rescale(emul, lam, normalize, rescale, sign_election):
    dc.check_options(emul, lam, normalize, rescale, sign_election)


CORNERS = [dc.check_signed_alphas, dc.check_zero_delta, dc.check_tiny_weight_sum, dc.check_denormals, dc.check_unaligned,
           dc.check_tiny_and_rank3, dc.check_nonfinite, dc.check_arguments, dc.check_density_one_is_ties, dc.check_nested_masks,
           dc.check_determinism, dc.check_slices, dc.check_streams_and_keys]


@pytest.mark.parametrize("check", CORNERS, ids=lambda f: f.__name__[len("check_"):])
def test_corner(emul, check):
    check(emul)


@pytest.mark.parametrize("density", dc.DENSITIES)
def test_statistics(emul, density):
    dc.check_statistics(emul, density)


def test_largest_emulator_shape(emul):
    fts, bases, bo = make_inputs((512, 1024), 3, seed=5, own_bases=True)
    dc.check(emul, fts, bases, ALPHAS[:3], bo, density=0.2, lam=0.7, label="512 x 1024")


def test_profile_names_and_launches(emul):
    fts, bases, bo = make_inputs((40, 50), 5, seed=6)
    emul.ctx.profile(True)
    emul.ctx.profile_reset()
    try:
        emul.dare_merge(fts, bases, ALPHAS[:5], bo)
        table = emul.ctx.profile_table()
    finally:
        emul.ctx.profile(False)
    assert {n: table[n][0] for n in table} == {"dare_merge": 1}


def test_c_abi_rejects_bad_arguments(emul):
    import math
    from shardmerge_amd import _lib
    x = torch.zeros(64, dtype=torch.bfloat16)
    y = torch.zeros(64, dtype=torch.bfloat16)
    out = torch.zeros(64, dtype=torch.bfloat16)

    def call(k=1, density=0.2, out_t=out, n=64, in_dtype=_lib.BF16):
        d = _lib.DareDesc()
        d.k = k
        for i in range(max(0, min(k, 16))):
            d.finetune[i], d.base[i], d.alpha[i], d.stream_id[i] = x.data_ptr(), y.data_ptr(), 0.5, i
        d.in_dtype, d.base_out, d.base_out_dtype, d.n = in_dtype, y.data_ptr(), _lib.BF16, n
        d.density, d.lam, d.normalize, d.key, d.rescale, d.sign_election = density, 1.0, 1, 7, 1, 1
        rep = _lib.DareReport()
        rc = emul.lib.dll.smhip_dare_merge(emul.ctx.h, C.byref(d), out_t.data_ptr(), None, C.byref(rep), None)
        return rc, emul.lib.dll.smhip_last_error(emul.ctx.h).decode(), rep

    assert call()[0] == _lib.OK
    rc, _, rep = call(density=2.0 ** -16)
    assert rc == _lib.OK and rep.T == 1
    for kwargs, word in (({"k": 0}, "k out of range"), ({"k": 17}, "k out of range"), ({"density": 0.0}, "density"),
                         ({"density": 1.01}, "density"), ({"density": math.nextafter(2.0 ** -16, 0.0)}, "smallest density"),
                         ({"out_t": x}, "overlaps"), ({"in_dtype": 3}, "dtype")):
        rc, msg, _ = call(**kwargs)
        assert rc == _lib.ERR_ARG and word in msg, (kwargs, rc, msg)
    assert call(n=0, out_t=x)[0] == _lib.OK                     # a no-op, whatever the pointers


# ---- YAML ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("operator", OPERATORS)
def test_yaml_accepts_the_operators_and_their_keys(tmp_path, operator):
    from shardmerge_amd.merge import operator_class
    from shardmerge_amd.merge.dare import DareLinearMerge, DareTiesMerge
    from shardmerge_amd.merge.fast_fourier import FourierMerge
    from shardmerge_amd.merge.ties import TiesMerge
    cls = operator_class(operator)
    assert cls is (DareTiesMerge if operator == "dare_ties" else DareLinearMerge) and issubclass(cls, TiesMerge)
    assert cls.sign_election is (operator == "dare_ties")
    cfg = MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": operator}))
    assert cfg.operator == operator and cfg.merge_options == {}
    m = cls(config=cfg, index_manager=object())
    assert (m.density, m.dare_lambda, bool(m.dare_normalize), bool(m.dare_rescale), m.seed) == (0.2, 1.0, True, True, 0)
    seed = 2 ** 63 - 1                                           # not representable in a double: it must survive exactly
    cfg = MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": operator, "density": 1, "dare_lambda": 0.7, "dare_normalize": 0,
                                                 "dare_rescale": 0, "seed": seed}))
    assert cfg.merge_options == {"density": 1.0, "dare_lambda": 0.7, "dare_normalize": 0.0, "dare_rescale": 0.0, "seed": seed}
    assert isinstance(cfg.merge_options["seed"], int)
    m = cls(config=cfg, index_manager=object())
    assert (m.density, m.dare_lambda, bool(m.dare_normalize), bool(m.dare_rescale)) == (1.0, 0.7, False, False)
    assert m.seed == seed and isinstance(m.seed, int)
    cfg = MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": operator, "density": 0.2, "dare_lambda": 0.7, "seed": 42}))
    readme = cls(config=cfg, index_manager=object()).get_readme()
    for word in ("DARE", operator, "density 0.2", "13107/65536", "0.199997", "lambda 0.7", "seed 42", "org/ft1"):
        assert word in readme, (word, readme)
    assert MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": operator, "density": 2.0 ** -16})).merge_options == {"density": 2.0 ** -16}
    # the one method both paths call is what differs
    assert cls.merge_block is not TiesMerge.merge_block and cls._merge_layer is FourierMerge._merge_layer


def test_stream_ids_are_positions_in_the_config(tmp_path):
    from shardmerge_amd.merge.dare import DareTiesMerge, tensor_key
    doc = yaml.safe_load(yaml_config(tmp_path, {"operator": "dare_ties"}).read_text())
    doc["finetune_merge"] = dc.dare_models("org/ft3")
    p = tmp_path / "three.yaml"
    p.write_text(yaml.safe_dump(doc))
    m = DareTiesMerge(config=MergeConfig.from_yaml(p), index_manager=object())
    assert m.stream_ids("model.layers.0.mlp.up_proj.weight", 3) == [0, 1, 2]
    assert m.stream_ids("model.layers.1.mlp.up_proj.weight", 2) == [0, 2]
    with pytest.raises(ValueError, match="cover layer 1"):
        m.stream_ids("model.layers.1.mlp.up_proj.weight", 3)
    assert tensor_key(5, "model.layers.1.mlp.up_proj.weight") == dare_oracle.tensor_key(5, "model.layers.1.mlp.up_proj.weight")
    assert tensor_key(5, "a") != tensor_key(6, "a") and tensor_key(5, "a") != tensor_key(5, "b")


@pytest.mark.parametrize("operator", OPERATORS)
@pytest.mark.parametrize("key,value", [("density", 0), ("density", -0.1), ("density", 1.0001), ("density", "0.2"), ("density", True),
                                       ("density", 2.0 ** -17), ("density", 1.5258789e-05),
                                       ("dare_lambda", 1e7), ("dare_lambda", -1e7), ("dare_lambda", "x"),
                                       ("dare_normalize", 2), ("dare_normalize", 0.5), ("dare_normalize", -1), ("dare_normalize", "yes"),
                                       ("dare_rescale", 2), ("dare_rescale", 0.5), ("dare_rescale", -1), ("dare_rescale", "no"),
                                       ("seed", 1.5), ("seed", 1.0), ("seed", True), ("seed", -1), ("seed", 2 ** 63), ("seed", "7")])
def test_yaml_rejects_out_of_range_values(tmp_path, operator, key, value):
    with pytest.raises(click.BadParameter, match=key):
        MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": operator, key: value}))


@pytest.mark.parametrize("operator", [None, "fourier", "addition", "task_addition", "fourier_legacy", "ties"])
@pytest.mark.parametrize("key", ["dare_lambda", "dare_normalize", "dare_rescale", "seed"])
def test_yaml_rejects_a_dare_key_with_another_operator(tmp_path, operator, key):
    opts = {key: 1}
    if operator:
        opts["operator"] = operator
    with pytest.raises(click.BadParameter, match=key):
        MergeConfig.from_yaml(yaml_config(tmp_path, opts))


@pytest.mark.parametrize("operator", OPERATORS)
@pytest.mark.parametrize("key,value", [("cutoff_pct", 0.08), ("cull_start_pct", 0.2), ("t_sum", 1.0), ("target_norm_offset", 1e-10),
                                       ("b", 0.1), ("norm_mode", "exact"), ("task_add_models", ["org/ft1"]), ("ties_lambda", 1.0),
                                       ("ties_normalize", 1), ("bogus", 1)])
def test_yaml_rejects_an_option_dare_would_ignore(tmp_path, operator, key, value):
    with pytest.raises(click.BadParameter, match=key):
        MergeConfig.from_yaml(yaml_config(tmp_path, {"operator": operator, key: value}))


def test_config_stamp(tmp_path):
    stamp = lambda opts: distributed.config_stamp(MergeConfig.from_yaml(yaml_config(tmp_path, opts)))
    full = {"operator": "dare_ties", "density": 0.2, "dare_lambda": 1.0, "dare_normalize": 1, "dare_rescale": 1, "seed": 2 ** 62}
    base = stamp(full)
    assert base == stamp(dict(full))
    others = [stamp({**full, "operator": "dare_linear"}), stamp({**full, "density": 0.3}), stamp({**full, "dare_lambda": 0.9}),
              stamp({**full, "dare_normalize": 0}), stamp({**full, "dare_rescale": 0}),
              stamp({**full, "seed": 2 ** 62 + 1}),                  # (the two seeds are the same double)
              stamp({**full, "seed": 0}), stamp({"operator": "ties", "density": 0.2}), stamp(None)]
    assert len({base, *others}) == len(others) + 1
    # a configuration without the DARE operators stamps as it always did
    import hashlib
    import json
    from dataclasses import asdict
    from shardmerge_amd.constants import DEFAULT_NORM_MODE
    for opts, operator in (({"cutoff_pct": 0.05}, "fourier"), ({"operator": "ties", "density": 0.25, "ties_lambda": 0.5}, "ties")):
        cfg = MergeConfig.from_yaml(yaml_config(tmp_path, opts))
        doc = {"output_base_model": cfg.output_base_model, "output_dtype": cfg.output_dtype,
               "finetune_merge": [asdict(m) for m in cfg.finetune_merge],
               "merge_options": {k: float(v) for k, v in opts.items() if k != "operator"},
               "operator": operator, "norm_mode": DEFAULT_NORM_MODE}
        assert distributed.config_stamp(cfg) == hashlib.sha256(json.dumps(doc, sort_keys=True, default=str).encode()).hexdigest()[:16]


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
    for word in ("DARE", operator, "density 0.3", "19660/65536", "lambda 0.7", f"seed {opts['seed']}"):
        assert word in readme, (word, readme)
    # one finetune given as a LoRA adapter directory: the run on its materialised checkpoint
    res = run_cli(dc.write_config(tmp_path, "org/lora", "merged_adapter", opts))
    assert res.exit_code == 0, res.output
    lf.assert_same_outputs(tmp_path / "merged_adapter", tmp_path / "merged")
    # the default options
    res = run_cli(dc.write_config(tmp_path, "org/lora_full", "merged_default", {"operator": operator}))
    assert res.exit_code == 0, res.output
    assert_outputs(tmp_path / "merged_default", dc.expected_outputs(base, full, {"operator": operator}))
    # another seed: another model
    res = run_cli(dc.write_config(tmp_path, "org/lora_full", "merged_seed", {**opts, "seed": 1}))
    assert res.exit_code == 0, res.output
    other = lf.read_outputs(tmp_path / "merged_seed")
    assert any(not torch.equal(other[n], expected[n]) for n in expected if "layers" in n)
    assert_outputs(tmp_path / "merged_seed", dc.expected_outputs(base, full, {**opts, "seed": 1}))


def test_expected_outputs_depend_on_the_stream_of_the_windowed_layer(tmp_path, emul):
    """the CLI tests can tell a stream id taken from the wrong list: on layer 1 stream 1 gives other bytes than stream 2"""
    base, factors, full = lf.setup_k3(tmp_path, emul)
    opts = dc.options("dare_ties")
    ft1 = lf.model_tensors(1)
    name = next(n for n, _ in lf.TENSORS if n.startswith("model.layers.1."))
    call = lambda sids: dare_oracle.dare_merge([ft1[name], full[name]], [base[name], base[name]], [0.5, 0.4], base[name], density=0.3,
                                               lam=0.7, key=dare_oracle.tensor_key(opts["seed"], name), stream_ids=sids)[0]
    assert not torch.equal(call([0, 1]), call([0, 2]))
    assert torch.equal(call([0, 2]), dc.expected_outputs(base, full, opts)[name])


@pytest.mark.parametrize("operator", OPERATORS)
def test_cli_in_place_equals_the_oracle(tmp_path, emul, monkeypatch, operator):
    """the partitioned path merges block tensors itself (distributed._merge_block_tensor): the same mask there"""
    monkeypatch.setenv("SHARDMERGE_INPLACE", "1")
    monkeypatch.setattr(distributed, "ENGINE_FACTORY", lambda: emul)
    base, factors, full = lf.setup_k3(tmp_path, emul)
    opts = dc.options(operator)
    res = run_cli(dc.write_config(tmp_path, "org/lora", "merged", opts))
    assert res.exit_code == 0, res.output
    assert_outputs(tmp_path / "merged", dc.expected_outputs(base, full, opts))
    assert "DARE" in (tmp_path / "merged" / "README.md").read_text()


@pytest.mark.parametrize("operator", OPERATORS)
def test_two_gloo_ranks_equal_the_oracle(tmp_path, emul, operator):
    base, factors, full = lf.setup_k3(tmp_path, emul)
    opts = dc.options(operator)
    cfg = dc.write_config(tmp_path, "org/lora", "merged", opts, device="cpu")
    run_ranks(cfg)
    assert not list((tmp_path / "merged").glob(".tmp-*"))
    assert_outputs(tmp_path / "merged", dc.expected_outputs(base, full, opts))
