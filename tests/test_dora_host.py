"""DoRA and embedding-LoRA adapters as finetunes, CPU tier: key parsing and the rejection rules, smhip_adapter_apply
through the CPU work-group emulator against fp64, and the CLI end to end with a DoRA + embedding adapter entry."""
import asyncio
import json
import math

import pytest
import torch
from click.testing import CliRunner

from shardmerge_amd import distributed
from shardmerge_amd.adapter import AdapterError, LoraAdapter
from shardmerge_amd.config import MergeConfig
from shardmerge_amd.index import LocalModelIndex
from tests import dora_fixtures as df
from tests import lora_fixtures as lf
from tests.harness import emul  # noqa: F401

DTYPES = (torch.bfloat16, torch.float16, torch.float32)
Q0 = "base_model.model.model.layers.0.self_attn.q_proj"
EMB = "base_model.model.model.embed_tokens"


def _run_cli(cfg_path):
    from shardmerge_amd.__main__ import cli
    return CliRunner().invoke(cli, ["merge", str(cfg_path)])


# ---- adapter_config.json and keys ----------------------------------------------------------------------------
def _adapter(tmp_path, factors, config):
    storage = tmp_path / "storage"
    lf.write_adapter(storage, "org/dora", factors, config)
    return LoraAdapter("org/dora", storage / "org/dora")


def test_dora_and_embedding_adapter_is_accepted(tmp_path):
    ad = _adapter(tmp_path, df.dora_factors(8), df.dora_config(8, 16, alpha_pattern={"embed_tokens": 4},
                                                                 rank_pattern={}))
    assert len(ad.pairs) == 5
    q = ad.pairs["model.layers.0.self_attn.q_proj.weight"]
    assert (q.kind, q.a_key, q.b_key, q.m_key) == ("linear", f"{Q0}.lora_A.weight", f"{Q0}.lora_B.weight",
                                                   f"{Q0}.lora_magnitude_vector")
    assert q.scale == 2.0 and q.rank == 8
    e = ad.pairs["model.embed_tokens.weight"]
    assert (e.kind, e.a_key, e.b_key, e.m_key) == ("embedding", f"{EMB}.lora_embedding_A", f"{EMB}.lora_embedding_B", None)
    assert e.scale == 4 / 8
    ad = _adapter(tmp_path, df.dora_factors(8), df.dora_config(8, 16, use_rslora=True))
    assert ad.pairs["model.embed_tokens.weight"].scale == 16 / math.sqrt(8)
    # embedding LoRA without DoRA
    f = {k: v for k, v in df.dora_factors(8).items() if "magnitude" not in k}
    ad = _adapter(tmp_path, f, lf.adapter_config(8, 16))
    assert ad.pairs["model.embed_tokens.weight"].kind == "embedding"
    assert all(p.m_key is None for p in ad.pairs.values())


def test_embedding_rank_pattern(tmp_path):
    f = df.dora_factors(8)
    f[f"{EMB}.lora_embedding_A"] = f[f"{EMB}.lora_embedding_A"][:4].clone()
    f[f"{EMB}.lora_embedding_B"] = f[f"{EMB}.lora_embedding_B"][:, :4].clone()
    ad = _adapter(tmp_path, f, df.dora_config(8, 16, rank_pattern={"embed_tokens": 4}))
    assert ad.pairs["model.embed_tokens.weight"].rank == 4 and ad.pairs["model.embed_tokens.weight"].scale == 4.0
    with pytest.raises(AdapterError, match=r"lora_embedding_A has rank 4, r says 8"):
        _adapter(tmp_path, f, df.dora_config(8, 16))


def _bad(kind):
    f = df.dora_factors(8)
    cfg = df.dora_config(8, 16)
    if kind == "dora_embedding":
        f[f"{EMB}.lora_magnitude_vector"] = torch.ones(64, dtype=torch.bfloat16)
    elif kind == "no_magnitude":
        del f[f"{Q0}.lora_magnitude_vector"]
    elif kind == "magnitude_without_dora":
        cfg["use_dora"] = False
    elif kind == "magnitude_shape":
        f[f"{Q0}.lora_magnitude_vector"] = torch.ones(127, dtype=torch.bfloat16)
    elif kind == "magnitude_2d":
        f[f"{Q0}.lora_magnitude_vector"] = torch.ones(128, 1, dtype=torch.bfloat16)
    elif kind == "magnitude_dtype":
        f[f"{Q0}.lora_magnitude_vector"] = torch.ones(128, dtype=torch.float64)
    elif kind == "lone_embedding_B":
        del f[f"{EMB}.lora_embedding_A"]
    elif kind == "embedding_shape":
        f[f"{EMB}.lora_embedding_A"] = torch.zeros(8, 65, dtype=torch.bfloat16)
    elif kind == "embedding_rank":
        f[f"{EMB}.lora_embedding_B"] = torch.zeros(128, 7, dtype=torch.bfloat16)
    elif kind == "magnitude_alone":
        f["base_model.model.model.layers.0.self_attn.k_proj.lora_magnitude_vector"] = torch.ones(64)
    elif kind == "modules_to_save":
        cfg["modules_to_save"] = ["lm_head"]
    elif kind == "fan_in_fan_out":
        cfg["fan_in_fan_out"] = True
    elif kind == "bias":
        f[f"{Q0}.lora_B.bias"] = torch.zeros(128, dtype=torch.bfloat16)
    return f, cfg


@pytest.mark.parametrize("kind,words", [
    ("dora_embedding", ["DoRA", "embed_tokens", "lora_magnitude_vector"]),
    ("no_magnitude", ["use_dora", "q_proj"]),
    ("magnitude_without_dora", ["lora_magnitude_vector", "use_dora"]),
    ("magnitude_shape", ["q_proj.lora_magnitude_vector", "127"]),
    ("magnitude_2d", ["q_proj.lora_magnitude_vector"]),
    ("magnitude_dtype", ["q_proj.lora_magnitude_vector", "F64"]),
    ("lone_embedding_B", ["lora_embedding_B", "lora_embedding_A"]),
    ("embedding_shape", ["lora_embedding_A", "embed_tokens.weight"]),
    ("embedding_rank", ["lora_embedding_B", "ranks differ"]),
    ("magnitude_alone", ["k_proj.lora_magnitude_vector"]),
    ("modules_to_save", ["modules_to_save"]),
    ("fan_in_fan_out", ["fan_in_fan_out"]),
    ("bias", ["q_proj.lora_B.bias"])])
def test_rejections_fail_before_any_output(tmp_path, emul, caplog, kind, words):
    base, _, _ = df.setup_k3(tmp_path, emul)
    f, cfg = _bad(kind)
    lf.write_adapter(tmp_path / "storage", "org/dora", f, cfg)
    res = _run_cli(lf.write_config(tmp_path, df.k3_models_input("org/dora"), "merged"))
    assert res.exit_code != 0
    errors = [r.getMessage() for r in caplog.records if "LoRA adapter org/dora" in r.getMessage()]
    assert errors and all(w in errors[0] for w in words), (errors, words)
    assert not (tmp_path / "merged").exists()


# ---- smhip_adapter_apply on the emulator ---------------------------------------------------------------------
def _spacing(r):
    mant, tiny = (7, 2.0 ** -133) if r.dtype == torch.bfloat16 else (10, 2.0 ** -24)
    _, e = torch.frexp(r.double())
    return torch.ldexp(torch.ones_like(r, dtype=torch.float64), e - 1 - mant).clamp_min(tiny)


def check_against_fp64(out, e, slack, bd):
    """the bars: fp32 |out - e| <= 4 2^-24 |e| + slack; 16-bit: 1 ulp of round(e) beyond the slack.  Returns the
    number of elements that differ from round(e)."""
    if bd == torch.float32:
        assert ((out.double() - e).abs() <= 4 * 2.0 ** -24 * e.abs() + slack).all()
        return 0
    r = e.to(bd)
    ulps = (((out.double() - r.double()).abs() - slack).clamp_min(0) / _spacing(r)).max().item()
    assert ulps <= 1.0 + 1e-9, ulps
    return (out != r).sum().item()


def dora_slack(a, b, s, fd, f, embedding=False):
    """what the fp32 sum of 16-bit factor products may lose, scaled by |m| / ||V|| for DoRA"""
    if fd == torch.float32:
        return 0.0
    rank = a.shape[0]
    s32 = float(torch.tensor(s, dtype=torch.float32))
    absprod = (a.double().abs().T @ b.double().abs().T) if embedding else (b.double().abs() @ a.double().abs())
    acc = (rank + 2) * 2.0 ** -24 * s32 * absprod
    return acc if f is None else acc * f.abs()[:, None]


@pytest.mark.parametrize("shape", [(1, 4096), (37, 53), (96, 160), (300, 7), (3, 5)])
@pytest.mark.parametrize("rank", [1, 7, 64])
def test_dora_emulator_against_fp64(emul, shape, rank):
    rows, cols = shape
    g = torch.Generator().manual_seed(rows * 1000 + cols + rank)
    diffs = total = 0
    for bd in DTYPES:
        for fd in DTYPES:
            for md in (torch.float32, torch.bfloat16):
                base = (torch.randn(rows, cols, generator=g) * 0.02).to(bd)
                a = (torch.randn(rank, cols, generator=g) * 0.1).to(fd)
                b = (torch.randn(rows, rank, generator=g) * 0.1).to(fd)
                m = (torch.rand(rows, generator=g) + 0.5).to(md)
                s = 0.02 / (0.01 * math.sqrt(rank))
                out = emul.lora_apply(base, a, b, s, magnitude=m)
                assert out.dtype == bd and out.shape == base.shape
                assert torch.equal(out, emul.lora_apply(base, a, b, s, magnitude=m))
                e, f = df.dora_ref(base, a, b, s, m)
                n = check_against_fp64(out, e, dora_slack(a, b, s, fd, f), bd)
                if bd != torch.float32:
                    diffs += n
                    total += out.numel()
    assert diffs <= max(2, 1e-3 * total) if total >= 4096 * 30 else True, (diffs, total)


@pytest.mark.parametrize("shape", [(64, 128), (1000, 96)])
@pytest.mark.parametrize("rank", [1, 16])
def test_embedding_emulator_against_fp64(emul, shape, rank):
    rows, cols = shape
    g = torch.Generator().manual_seed(rows + cols + rank)
    for bd in DTYPES:
        for fd in DTYPES:
            base = (torch.randn(rows, cols, generator=g) * 0.02).to(bd)
            a = (torch.randn(rank, rows, generator=g) * 0.1).to(fd)          # lora_embedding_A [r, num_embeddings]
            b = (torch.randn(cols, rank, generator=g) * 0.1).to(fd)          # lora_embedding_B [dim, r]
            s = 0.02 / (0.01 * math.sqrt(rank))
            out = emul.lora_apply(base, a, b, s, embedding=True)
            assert torch.equal(out, emul.lora_apply(base, a, b, s, embedding=True))
            e, _ = df.dora_ref(base, a, b, s, None, embedding=True)
            check_against_fp64(out, e, dora_slack(a, b, s, fd, None, embedding=True), bd)
            # the same as plain LoRA with the factors transposed by hand
            assert torch.equal(out, emul.lora_apply(base, b.T.contiguous(), a.T.contiguous(), s))


def test_no_magnitude_through_the_new_entry_equals_lora_apply(emul):
    g = torch.Generator().manual_seed(5)
    for bd in DTYPES:
        for fd in DTYPES:
            base = (torch.randn(37, 53, generator=g) * 0.02).to(bd)
            a, b = (torch.randn(7, 53, generator=g) * 0.1).to(fd), (torch.randn(37, 7, generator=g) * 0.1).to(fd)
            assert torch.equal(emul.adapter_apply(base, a, b, 0.7).view(torch.uint8),
                               emul.lora_apply(base, a, b, 0.7).view(torch.uint8))


def test_zero_norm_rows_and_bad_magnitudes_raise_naming_the_row(emul):
    from shardmerge_amd._lib import ERR_ROW_NORM, SmhipError
    base = torch.randn(40, 24) * 0.02
    a, b = torch.randn(4, 24) * 0.1, torch.randn(40, 4) * 0.1
    b[17] = 0
    base[17] = 0
    with pytest.raises(SmhipError, match=r"row 17 .*\(1 of 40 rows\)") as ei:
        emul.lora_apply(base, a, b, 1.0, magnitude=torch.ones(40))
    assert ei.value.code == ERR_ROW_NORM
    base[17] = 1.0
    for bad in (float("nan"), float("inf")):
        m = torch.ones(40)
        m[33] = bad
        m[35] = bad
        with pytest.raises(SmhipError, match=r"row 33 .*\(2 of 40 rows\)"):
            emul.lora_apply(base, a, b, 1.0, magnitude=m)
    with pytest.raises(ValueError, match="Linear"):
        emul.lora_apply(base, torch.randn(4, 40), torch.randn(24, 4), 1.0, magnitude=torch.ones(40), embedding=True)


def test_zero_norm_row_fails_the_merge_naming_adapter_tensor_and_row(tmp_path, emul, caplog):
    base, f, _ = df.setup_k3(tmp_path, emul)
    f[f"{Q0}.lora_magnitude_vector"][5] = float("nan")
    lf.write_adapter(tmp_path / "storage", "org/dora", f, df.dora_config(8, 16))
    res = _run_cli(lf.write_config(tmp_path, df.k3_models_input("org/dora"), "merged"))
    assert res.exit_code != 0
    errors = [r.getMessage() for r in caplog.records if "LoRA adapter org/dora" in r.getMessage()]
    assert errors and "model.layers.0.self_attn.q_proj.weight" in errors[0] and "row 5" in errors[0], errors


# ---- the CLI and the merge path ------------------------------------------------------------------------------
@pytest.mark.parametrize("operator", [None, "addition"])
def test_cli_dora_adapter_entry_equals_materialised_checkpoint(tmp_path, emul, operator):
    base, factors, full = df.setup_k3(tmp_path, emul)
    changed = {n for n in full if not torch.equal(full[n], base[n])}
    assert "model.embed_tokens.weight" in changed and "model.layers.1.self_attn.v_proj.weight" in changed
    for adapter, out in (("org/dora", "merged_adapter"), ("org/dora_full", "merged_full")):
        res = _run_cli(lf.write_config(tmp_path, df.k3_models_input(adapter), out, operator))
        assert res.exit_code == 0, res.output
    lf.assert_same_outputs(tmp_path / "merged_adapter", tmp_path / "merged_full")


def test_finetune_tensor_reads_base_factors_and_magnitude(tmp_path, emul):
    df.setup_k3(tmp_path, emul)
    cfg = MergeConfig.from_yaml(lf.write_config(tmp_path, df.k3_models_input("org/dora"), "merged"))
    from shardmerge_amd.merge.fast_fourier import FourierMerge
    merger = FourierMerge(config=cfg, index_manager=LocalModelIndex(cfg.storage_path), engine=emul)
    asyncio.run(merger.initialize())
    m = cfg.finetune_merge[0]
    for name, want in (("model.layers.0.self_attn.q_proj.weight",
                        [("org/base", None), ("org/dora", "lora_A.weight"), ("org/dora", "lora_B.weight"),
                         ("org/dora", "lora_magnitude_vector")]),
                       ("model.embed_tokens.weight",
                        [("org/base", None), ("org/dora", "lora_embedding_A"), ("org/dora", "lora_embedding_B")])):
        calls = []

        async def fetch(uri, tname):
            calls.append((uri, tname))
            return merger.index_manager.load_tensor(uri, tname)
        asyncio.run(merger.finetune_tensor(m, name, "cpu", fetch))
        assert len(calls) == len(want) and calls == merger._finetune_requests(m, name)
        for (uri, tname), (wu, suffix) in zip(calls, want):
            assert uri == wu and (tname == name if suffix is None else tname.endswith(suffix)), (calls, want)


def test_config_stamp_changes_when_use_dora_flips(tmp_path, emul):
    df.setup_k3(tmp_path, emul)
    cfg_path = lf.write_config(tmp_path, df.k3_models_input("org/dora"), "merged")
    s0 = distributed.config_stamp(MergeConfig.from_yaml(cfg_path))
    d = tmp_path / "storage" / "org/dora"
    cfg = json.loads((d / "adapter_config.json").read_text())
    cfg["use_dora"] = False
    (d / "adapter_config.json").write_text(json.dumps(cfg))
    assert distributed.config_stamp(MergeConfig.from_yaml(cfg_path)) != s0
