"""LoRA adapters as finetunes, CPU tier: adapter_config.json parsing and validation, smhip_lora_apply through the CPU
work-group emulator against fp64, and the CLI end to end with an adapter entry (the emulator as the device)."""
import asyncio
import json
import math
import os

import pytest
import torch
from click.testing import CliRunner

from shardmerge_amd import distributed
from shardmerge_amd.adapter import AdapterError, LoraAdapter, pattern_key
from shardmerge_amd.config import MergeConfig
from shardmerge_amd.index import LocalModelIndex
from tests import lora_fixtures as lf
from tests.harness import emul  # noqa: F401

DTYPES = (torch.bfloat16, torch.float16, torch.float32)


def _run_cli(cfg_path):
    from shardmerge_amd.__main__ import cli
    return CliRunner().invoke(cli, ["merge", str(cfg_path)])


def _assert_rejected(res, caplog, tmp_path, *words):
    """the CLI failed with an AdapterError naming the adapter and `words`, and wrote no output"""
    assert res.exit_code != 0
    errors = [r.getMessage() for r in caplog.records if "LoRA adapter org/lora" in r.getMessage()]
    assert errors and all(w in errors[0] for w in words), (errors, words)
    assert not (tmp_path / "merged").exists()


# ---- adapter_config.json ----------------------------------------------------------------------------------
def _adapter(tmp_path, rank=8, factors=None, **cfg):
    storage = tmp_path / "storage"
    lf.write_adapter(storage, "org/lora", factors if factors is not None else lf.adapter_factors(rank),
                     lf.adapter_config(rank, **cfg))
    return LoraAdapter("org/lora", storage / "org/lora")


def test_scale_plain_rslora_and_alpha_pattern(tmp_path):
    q = "model.layers.0.self_attn.q_proj.weight"
    v = "model.layers.1.self_attn.v_proj.weight"
    ad = _adapter(tmp_path, rank=8, alpha=16)
    assert ad.pairs[q].scale == 2.0 and ad.pairs[q].rank == 8
    ad = _adapter(tmp_path, rank=8, alpha=16, use_rslora=True)
    assert ad.pairs[q].scale == 16 / math.sqrt(8)
    ad = _adapter(tmp_path, rank=8, alpha=16, alpha_pattern={"layers\\.1\\.self_attn\\.v_proj": 4, "v_proj": 32})
    assert ad.pairs[v].scale == 4 / 8                     # the first matching key in file order wins
    assert ad.pairs["model.layers.0.self_attn.v_proj.weight"].scale == 32 / 8
    assert ad.pairs[q].scale == 2.0


def test_rank_pattern_must_agree_with_the_factors(tmp_path):
    f = lf.adapter_factors(8)
    k = "base_model.model.model.layers.0.self_attn.q_proj"
    f[f"{k}.lora_A.weight"] = f[f"{k}.lora_A.weight"][:4].clone()
    f[f"{k}.lora_B.weight"] = f[f"{k}.lora_B.weight"][:, :4].clone()
    ad = _adapter(tmp_path, rank=8, factors=f, rank_pattern={"layers.0.self_attn.q_proj": 4})
    assert ad.pairs["model.layers.0.self_attn.q_proj.weight"].rank == 4
    assert ad.pairs["model.layers.0.self_attn.q_proj.weight"].scale == 16 / 4
    with pytest.raises(AdapterError, match=r"org/lora.*rank 4.*\br\b says 8"):
        _adapter(tmp_path, rank=8, factors=f)
    with pytest.raises(AdapterError, match=r"rank_pattern\['q_proj'\] says 2"):
        _adapter(tmp_path, rank=8, factors=f, rank_pattern={"q_proj": 2})


def test_pattern_keys_match_as_peft_matches_them():
    assert pattern_key({"q_proj": 1}, "model.layers.0.self_attn.q_proj") == "q_proj"
    assert pattern_key({"q_proj": 1}, "q_proj") == "q_proj"
    assert pattern_key({"q_proj": 1}, "model.layers.0.self_attn.xq_proj") is None
    assert pattern_key({r"layers\.[01]\.self_attn\.q_proj": 1}, "model.layers.1.self_attn.q_proj") is not None
    assert pattern_key({"a": 1, "q_proj": 2}, "x.q_proj") == "q_proj"


def test_key_mapping(tmp_path):
    ad = _adapter(tmp_path)
    want = {n for n, s in lf.TENSORS if len(s) == 2 and any(f".{t}." in n for t in lf.TARGETS)}
    assert set(ad.pairs) == want and len(want) == 4
    p = ad.pairs["model.layers.1.self_attn.v_proj.weight"]
    assert p.a_key == "base_model.model.model.layers.1.self_attn.v_proj.lora_A.weight"
    assert p.b_key == "base_model.model.model.layers.1.self_attn.v_proj.lora_B.weight"
    assert set(ad.weight_map()) == set(ad.header)


def _k3_dir(tmp_path, emul, config=None, factors=None, bin_only=False):
    base, f, _ = lf.setup_k3(tmp_path, emul)
    d = tmp_path / "storage" / "org/lora"
    if config is not None:
        (d / "adapter_config.json").write_text(json.dumps(config))
    if factors is not None:
        lf.write_adapter(tmp_path / "storage", "org/lora", factors, json.loads((d / "adapter_config.json").read_text()))
    if bin_only:
        os.replace(d / "adapter_model.safetensors", d / "adapter_model.bin")
    return lf.write_config(tmp_path, lf.k3_models("org/lora"), "merged")


def _bad_factors(kind):
    f = lf.adapter_factors(8)
    q = "base_model.model.model.layers.0.self_attn.q_proj"
    if kind == "embedding":
        f["base_model.model.model.embed_tokens.lora_embedding_A"] = torch.zeros(8, 64, dtype=torch.bfloat16)
    elif kind == "magnitude":
        f[f"{q}.lora_magnitude_vector"] = torch.ones(128, dtype=torch.bfloat16)
    elif kind == "full":
        f["base_model.model.model.norm.weight"] = torch.ones(128, dtype=torch.bfloat16)
    elif kind == "unpaired":
        del f[f"{q}.lora_B.weight"]
    elif kind == "shape":
        f[f"{q}.lora_A.weight"] = torch.zeros(8, 96, dtype=torch.bfloat16)
    elif kind == "not2d":
        f["base_model.model.model.layers.0.input_layernorm.lora_A.weight"] = torch.zeros(8, 128, dtype=torch.bfloat16)
        f["base_model.model.model.layers.0.input_layernorm.lora_B.weight"] = torch.zeros(128, 8, dtype=torch.bfloat16)
    return f


@pytest.mark.parametrize("field,value,msg", [
    ("peft_type", "IA3", "peft_type"), ("use_dora", True, "use_dora"), ("fan_in_fan_out", True, "fan_in_fan_out"),
    ("bias", "lora_only", "bias"), ("modules_to_save", ["lm_head"], "modules_to_save"),
    ("layer_replication", [[0, 2]], "layer_replication")])
def test_config_rejections_fail_before_any_output(tmp_path, emul, caplog, field, value, msg):
    cfg = lf.adapter_config(8, 16)
    cfg[field] = value
    _assert_rejected(_run_cli(_k3_dir(tmp_path, emul, config=cfg)), caplog, tmp_path, msg)


@pytest.mark.parametrize("kind,msg", [
    ("embedding", "lora_embedding_A"), ("magnitude", "lora_magnitude_vector"), ("full", "model.norm.weight"),
    ("unpaired", "q_proj.lora_A.weight"), ("shape", "q_proj.lora_A.weight"), ("not2d", "input_layernorm")])
def test_tensor_rejections_fail_before_any_output(tmp_path, emul, caplog, kind, msg):
    _assert_rejected(_run_cli(_k3_dir(tmp_path, emul, factors=_bad_factors(kind))), caplog, tmp_path, msg)


def test_bin_only_adapter_is_rejected_and_plain_missing_dir_keeps_its_error(tmp_path, emul, caplog):
    _assert_rejected(_run_cli(_k3_dir(tmp_path, emul, bin_only=True)), caplog, tmp_path, "adapter_model.bin")
    idx = LocalModelIndex(tmp_path / "storage")
    (tmp_path / "storage" / "org/lora").rename(tmp_path / "storage" / "org/lora_bin")
    with pytest.raises(AdapterError, match="org/lora_bin: only adapter_model.bin"):
        asyncio.run(idx.add_model("org/lora_bin"))
    idx = LocalModelIndex(tmp_path / "storage")
    (tmp_path / "storage" / "org/empty").mkdir(parents=True)
    with pytest.raises(FileNotFoundError, match="model.safetensors.index.json not found"):
        asyncio.run(idx.add_model("org/empty"))


def test_directory_with_an_index_stays_a_full_model(tmp_path, emul):
    storage = tmp_path / "storage"
    lf.write_model(storage, "org/both", lf.model_tensors(1))
    lf.write_adapter(storage, "org/both", lf.adapter_factors(8), lf.adapter_config(8))
    idx = LocalModelIndex(storage)
    asyncio.run(idx.add_model("org/both"))
    assert idx.adapter("org/both") is None and idx.get_model_keys("org/both") == {n for n, _ in lf.TENSORS}


# ---- smhip_lora_apply on the emulator ----------------------------------------------------------------------
def _ref(base, a, b, s):
    return base.double() + float(torch.tensor(s, dtype=torch.float32)) * (b.double() @ a.double())


def _ulp_diff(out, e, dtype, acc_err=0.0):
    """|out - round(e)| less acc_err (what the contract's fp32 sum may lose where the result cancels against the base),
    in units of the dtype's spacing at round(e); and the number of elements that differ from round(e)"""
    r = e.to(dtype)
    nxt = torch.nextafter(r.float().abs().to(dtype), torch.tensor(float("inf"), dtype=dtype)).double() - r.double().abs()
    return ((((out.double() - r.double()).abs() - acc_err).clamp_min(0)) / nxt).max().item(), (out != r).sum().item()


@pytest.mark.parametrize("shape", [(1, 4096), (37, 53), (96, 160)])
@pytest.mark.parametrize("rank", [1, 7, 64])
def test_lora_apply_emulator_against_fp64(emul, shape, rank):
    rows, cols = shape
    g = torch.Generator().manual_seed(rows * 1000 + cols + rank)
    diffs, total = {}, {}
    for bd in DTYPES:
        for fd in DTYPES:
            base = (torch.randn(rows, cols, generator=g) * 0.02).to(bd)
            # s * B @ A about the size of the base (the hard case for rounding)
            a = (torch.randn(rank, cols, generator=g) * 0.1).to(fd)
            b = (torch.randn(rows, rank, generator=g) * 0.1).to(fd)
            s = 0.02 / (0.01 * math.sqrt(rank))
            out = emul.lora_apply(base, a, b, s)
            assert out.dtype == bd and out.shape == base.shape
            assert torch.equal(out, emul.lora_apply(base, a, b, s))
            e = _ref(base, a, b, s)
            if bd == torch.float32:
                sf = float(torch.tensor(s, dtype=torch.float32))
                bound = 2.0 ** -24 * e.abs() + (rank + 2) * 2.0 ** -24 * sf * (b.double().abs() @ a.double().abs())
                assert ((out.double() - e).abs() <= bound).all(), (bd, fd)
            else:
                acc_err = 0.0 if fd == torch.float32 else (rank + 2) * 2.0 ** -24 * s * (b.double().abs() @ a.double().abs())
                ulps, n = _ulp_diff(out, e, bd, acc_err)
                assert ulps <= 1.0 + 1e-9, (bd, fd, ulps)
                diffs[bd] = diffs.get(bd, 0) + n
                total[bd] = total.get(bd, 0) + out.numel() * 3
    for bd in diffs:                                          # over the three factor dtypes
        assert diffs[bd] <= max(1, 1e-3 * total[bd]) * 3, (bd, diffs[bd], total[bd])


def test_lora_apply_unaligned_inputs_and_bad_arguments(emul):
    buf = torch.randn(1 + 37 * 53) * 0.02
    base = buf[1:].view(37, 53)                            # 4-byte offset: no 16-byte alignment
    a, b = torch.randn(7, 53).to(torch.bfloat16), torch.randn(37, 7).to(torch.bfloat16)
    out = emul.lora_apply(base, a, b, 0.5)
    assert torch.equal(out, emul.lora_apply(base.clone(), a, b, 0.5))
    with pytest.raises(ValueError):
        emul.lora_apply(base, a[:, :50], b, 0.5)
    from shardmerge_amd._lib import SmhipError
    with pytest.raises(SmhipError, match="rank"):
        emul.lora_apply(torch.zeros(4, 4), torch.zeros(513, 4), torch.zeros(4, 513), 1.0)


# ---- the CLI end to end --------------------------------------------------------------------------------------
@pytest.mark.parametrize("operator", [None, "addition"])
def test_cli_adapter_entry_equals_materialised_checkpoint(tmp_path, emul, operator):
    base, factors, full = lf.setup_k3(tmp_path, emul)
    assert any(not torch.equal(full[n], base[n]) for n in full)
    cfg_a = lf.write_config(tmp_path, lf.k3_models("org/lora"), "merged_adapter", operator)
    cfg_f = lf.write_config(tmp_path, lf.k3_models("org/lora_full"), "merged_full", operator)
    res = _run_cli(cfg_a)
    assert res.exit_code == 0, res.output
    res = _run_cli(cfg_f)
    assert res.exit_code == 0, res.output
    lf.assert_same_outputs(tmp_path / "merged_adapter", tmp_path / "merged_full")
    assert (json.loads((tmp_path / "merged_adapter" / "model.safetensors.index.json").read_text()) ==
            json.loads((tmp_path / "merged_full" / "model.safetensors.index.json").read_text()))


def test_untargeted_tensors_are_the_base_itself(tmp_path, emul):
    base, factors, full = lf.setup_k3(tmp_path, emul)
    cfg = MergeConfig.from_yaml(lf.write_config(tmp_path, lf.k3_models("org/lora"), "merged"))
    from shardmerge_amd.merge.fast_fourier import FourierMerge
    merger = FourierMerge(config=cfg, index_manager=LocalModelIndex(cfg.storage_path), engine=emul)
    asyncio.run(merger.initialize())
    m = cfg.finetune_merge[2]
    for name, _ in lf.TENSORS:
        base_t = merger.index_manager.load_tensor("org/base", name)
        calls = []

        async def fetch(uri, tname):
            calls.append((uri, tname))
            return base_t if (uri, tname) == ("org/base", name) else merger.index_manager.load_tensor(uri, tname)
        ft = asyncio.run(merger.finetune_tensor(m, name, "cpu", fetch))
        targeted = any(f".{t}." in name for t in lf.TARGETS)
        if not targeted:
            assert ft is base_t and calls == [("org/base", name)]
        else:
            assert len(calls) == 3 and set(calls) == set(merger._finetune_requests(m, name))


def test_zero_b_adapter_yields_the_base_and_merges_as_an_unchanged_finetune(tmp_path, emul):
    base, factors, full = lf.setup_k3(tmp_path, emul, zero_b=True)
    for n in base:
        assert torch.equal(full[n].view(torch.uint8), base[n].view(torch.uint8)), n
    lf.write_model(tmp_path / "storage", "org/base_copy", base)
    res = _run_cli(lf.write_config(tmp_path, lf.k3_models("org/lora"), "merged_adapter"))
    assert res.exit_code == 0, res.output
    res = _run_cli(lf.write_config(tmp_path, lf.k3_models("org/base_copy"), "merged_copy"))
    assert res.exit_code == 0, res.output
    lf.assert_same_outputs(tmp_path / "merged_adapter", tmp_path / "merged_copy")


def test_config_stamp_follows_the_adapter_files(tmp_path, emul):
    lf.setup_k3(tmp_path, emul)
    cfg_path = lf.write_config(tmp_path, lf.k3_models("org/lora"), "merged")
    s0 = distributed.config_stamp(MergeConfig.from_yaml(cfg_path))
    assert s0 == distributed.config_stamp(MergeConfig.from_yaml(cfg_path))
    d = tmp_path / "storage" / "org/lora"
    cfg = json.loads((d / "adapter_config.json").read_text())
    cfg["lora_alpha"] = 8
    (d / "adapter_config.json").write_text(json.dumps(cfg))
    s1 = distributed.config_stamp(MergeConfig.from_yaml(cfg_path))
    assert s1 != s0
    f = lf.adapter_factors(16)                                     # another rank: another header
    lf.write_adapter(tmp_path / "storage", "org/lora", f, lf.adapter_config(16, 16))
    s2 = distributed.config_stamp(MergeConfig.from_yaml(cfg_path))
    assert s2 not in (s0, s1)
    # configs without adapters keep their stamp's definition
    full_cfg = MergeConfig.from_yaml(lf.write_config(tmp_path, lf.k3_models("org/lora_full"), "merged_full"))
    from dataclasses import asdict
    import hashlib
    from shardmerge_amd.constants import DEFAULT_NORM_MODE
    doc = {"output_base_model": full_cfg.output_base_model, "output_dtype": full_cfg.output_dtype,
           "finetune_merge": [asdict(m) for m in full_cfg.finetune_merge], "merge_options": {},
           "operator": "fourier", "norm_mode": DEFAULT_NORM_MODE}
    assert distributed.config_stamp(full_cfg) == hashlib.sha256(json.dumps(doc, sort_keys=True, default=str).encode()).hexdigest()[:16]


def test_inplace_resume_rewrites_shards_after_the_adapter_changes(tmp_path, emul, monkeypatch):
    monkeypatch.setenv("SHARDMERGE_INPLACE", "1")
    monkeypatch.setattr(distributed, "ENGINE_FACTORY", lambda: emul)
    lf.setup_k3(tmp_path, emul)
    cfg_path = lf.write_config(tmp_path, lf.k3_models("org/lora"), "merged")
    res = _run_cli(cfg_path)
    assert res.exit_code == 0, res.output
    out = tmp_path / "merged"
    first = lf.read_outputs(out)
    # the same adapter again: every shard is complete and stamped, nothing is rewritten
    mtimes = {s: (out / s).stat().st_mtime_ns for s in lf.SHARDS}
    res = _run_cli(cfg_path)
    assert res.exit_code == 0, res.output
    assert {s: (out / s).stat().st_mtime_ns for s in lf.SHARDS} == mtimes
    # another adapter under the same name: the resumed run must not keep the old shards
    d = tmp_path / "storage" / "org/lora"
    f = lf.adapter_factors(8, seed=991)
    cfg = lf.adapter_config(8, 32)
    lf.write_adapter(tmp_path / "storage", "org/lora", f, cfg)
    base = lf.model_tensors(0)
    lf.materialise(emul, tmp_path / "storage", "org/lora2_full", base, f, 32 / 8)
    res = _run_cli(cfg_path)
    assert res.exit_code == 0, res.output
    second = lf.read_outputs(out)
    assert any(not torch.equal(first[k], second[k]) for k in first)
    res = _run_cli(lf.write_config(tmp_path, lf.k3_models("org/lora2_full"), "merged_full"))
    assert res.exit_code == 0, res.output
    lf.assert_same_outputs(out, tmp_path / "merged_full", file_bytes=False)
