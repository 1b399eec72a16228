"""The one checkpoint-format interface (shardmerge_amd/quantformat.py) on the CPU work-group emulator: every command on
every format's checkpoint, the resume stamp restated, one header read per shard, two claims, and the commands' --help."""
import hashlib
import json
import shutil
from dataclasses import asdict
from pathlib import Path

import pytest
from click.testing import CliRunner

from tests import harness, lora_fixtures as lf
from tests.harness import emul  # noqa: F401

FORMATS = {"fp8": "fp8", "mxfp4": "mx4", "nvfp4": "nv4", "gptq": "gptq"}       # command suffix -> key
NAMES = {"fp8": "FP8", "mxfp4": "MXFP4", "nvfp4": "NVFP4", "gptq": "GPTQ"}
COMMANDS = [f"{verb}-{suffix}" for suffix in FORMATS for verb in ("quantize", "dequantize")]
HELP_DIR = Path(__file__).parent / "golden" / "quant_help"


def run_cli(args):
    from shardmerge_amd.__main__ import cli
    return CliRunner().invoke(cli, [str(a) for a in args])


@pytest.fixture(scope="module")
def storage(tmp_path_factory):
    """the on-disk model of tests/lora_fixtures.py and org/ft1 as a checkpoint of each format, org/ft1-<suffix>; shared,
    and left as it is by every test"""
    from shardmerge_amd import engine as engine_mod
    from tests.emul.loader import emul_engine
    root = tmp_path_factory.mktemp("quantformat")
    eng = emul_engine()
    lf.setup_k3(root, eng)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(engine_mod, "get_engine", lambda device=None: eng)
        for suffix in FORMATS:
            res = run_cli([f"quantize-{suffix}", "org/ft1", "--out", root / "storage" / f"org/ft1-{suffix}",
                           "--storage-dir", root / "storage", "--device", "cpu"])
            assert res.exit_code == 0, res.output
    return root / "storage"


@pytest.mark.parametrize("held", [None] + list(FORMATS), ids=lambda s: s or "plain")
def test_rejection_matrix(tmp_path, emul, storage, caplog, held):
    """all eight commands on org/ft1 (held = None) or on its checkpoint of the format `held`: the own dequantize
    succeeds, the own quantize says "already", every other format's command names the dequantize that undoes the
    checkpoint, every dequantize of the plain model fails; no output directory exists after a failure"""
    model = "org/ft1" if held is None else f"org/ft1-{held}"
    for command in COMMANDS:
        verb, suffix = command.split("-")
        out = tmp_path / command
        caplog.clear()
        res = run_cli([command, model, "--out", out, "--storage-dir", storage, "--device", "cpu"])
        errors = [r.getMessage() for r in caplog.records if r.getMessage().startswith(f"Error during {command}: {command}: {model} ")]
        if (held is None and verb == "quantize") or (held == suffix and verb == "dequantize"):
            assert res.exit_code == 0 and not errors and (out / "model.safetensors.index.json").exists(), (command, res.output)
            continue
        assert res.exit_code != 0 and len(errors) == 1 and not out.exists(), (command, res.output)
        if held is None:
            assert NAMES[suffix] in errors[0] and "expected" in errors[0], errors[0]
        elif held == suffix:
            assert errors[0].endswith(f"{NAMES[suffix]} checkpoint already"), errors[0]
        else:
            assert errors[0].endswith(f"{NAMES[held]} checkpoint; `dequantize-{held}` first"), errors[0]


def test_stamp_restated(tmp_path, storage):
    """config_stamp of one entry of each format is the hash of the plain fields and, per format, {"<key>_models": {uri:
    {"<key>_headers": sha256 over the sorted shards of name + "\\0" + raw header}}} - the document of the commit before
    the formats shared an interface, so that a partly written output directory resumes"""
    from shardmerge_amd import distributed
    from shardmerge_amd.config import MergeConfig
    models = [{"model": f"org/ft1-{s}", "base": "org/base", "alpha": 0.5, "is_input": True, "is_output": True} for s in FORMATS]
    path = harness.write_config(tmp_path, models, "stamp", {"operator": "ties", "density": 0.3}, "cpu")
    path.write_text(path.read_text().replace(str(tmp_path / "storage"), str(storage)))
    cfg = MergeConfig.from_yaml(path)
    doc = {"output_base_model": cfg.output_base_model, "output_dtype": cfg.output_dtype,
           "finetune_merge": [asdict(m) for m in cfg.finetune_merge], "merge_options": dict(sorted(cfg.merge_options.items())),
           "operator": "ties", "norm_mode": getattr(cfg, "norm_mode", None) or distributed.DEFAULT_NORM_MODE}
    for suffix, key in FORMATS.items():
        uri = f"org/ft1-{suffix}"
        sha = hashlib.sha256()
        for shard in sorted((storage / uri).glob("*.safetensors")):
            data = shard.read_bytes()
            sha.update(shard.name.encode() + b"\0" + data[8:8 + int.from_bytes(data[:8], "little")])
        doc[f"{key}_models"] = {uri: {f"{key}_headers": sha.hexdigest()}}
    assert distributed.config_stamp(cfg) == hashlib.sha256(json.dumps(doc, sort_keys=True, default=str).encode()).hexdigest()[:16]


def test_one_header_read(tmp_path, storage, monkeypatch):
    """`add_model` of a checkpoint of each format reads each shard's header at most once, and so does `config_stamp` per entry"""
    import asyncio
    from shardmerge_amd import adapter, distributed, quantformat
    from shardmerge_amd.config import MergeConfig
    from shardmerge_amd.index import LocalModelIndex
    reads = []
    real = adapter.read_header

    def counted(path):
        reads.append(Path(path))
        return real(path)
    for module in (adapter, distributed, quantformat):
        monkeypatch.setattr(module, "read_header", counted)
    for suffix, key in FORMATS.items():
        uri = f"org/ft1-{suffix}"
        shards = sorted((storage / uri).glob("*.safetensors"))
        assert len(shards) > 1
        reads.clear()
        index = LocalModelIndex(storage_path=storage)
        asyncio.run(index.add_model(uri))
        assert index.quant(uri) is getattr(index, key)(uri) is not None and sorted(reads) == shards, (uri, reads)
        models = [{"model": uri, "base": "org/base", "alpha": 0.5, "is_input": True, "is_output": True}]
        path = harness.write_config(tmp_path, models, f"stamp-{suffix}", {"operator": "ties", "density": 0.3}, "cpu")
        path.write_text(path.read_text().replace(str(tmp_path / "storage"), str(storage)))
        reads.clear()
        distributed.config_stamp(MergeConfig.from_yaml(path))
        assert sorted(reads) == shards, (uri, reads)


def test_two_claims(tmp_path, storage, monkeypatch):
    """a directory whose hf_quant_config.json says NVFP4 and whose config.json says gptq, with both kinds of tensor, is
    rejected (here by the NVFP4 test, which reads a group size in both files); so is, naming both, any directory that two
    formats of the registry claim"""
    import asyncio
    from safetensors.torch import load_file, save_file
    from shardmerge_amd import quantformat
    from shardmerge_amd.gptqmodel import GptqModel
    from shardmerge_amd.index import LocalModelIndex
    both = tmp_path / "storage" / "org/both"
    shutil.copytree(storage / "org/ft1-nvfp4", both)
    config = json.loads((both / "config.json").read_text())
    (both / "hf_quant_config.json").write_text(json.dumps({"quantization": config["quantization_config"]}))
    config["quantization_config"] = json.loads((storage / "org/ft1-gptq" / "config.json").read_text())["quantization_config"]
    (both / "config.json").write_text(json.dumps(config))
    shard = sorted(both.glob("*.safetensors"))[0]
    gptq = load_file(str(sorted((storage / "org/ft1-gptq").glob("*.safetensors"))[0]))
    stem = next(n for n in gptq if n.endswith(".qweight"))[: -len("qweight")]
    extra = {"extra." + k: gptq[stem + k] for k in ("qweight", "qzeros", "scales", "g_idx")}
    save_file({**load_file(str(shard)), **extra}, str(shard), metadata={"format": "pt"})
    index = both / "model.safetensors.index.json"
    doc = json.loads(index.read_text())
    doc["weight_map"].update({k: shard.name for k in extra})
    index.write_text(json.dumps(doc))
    with pytest.raises(ValueError, match=r"org/both"):
        asyncio.run(LocalModelIndex(storage_path=tmp_path / "storage").add_model("org/both"))
    assert quantformat.identity_of(both) is None

    class Twin(GptqModel):
        KEY, A_LABEL = "twin", "a twin"
    monkeypatch.setattr(quantformat, "formats", lambda: (GptqModel, Twin))
    with pytest.raises(ValueError, match=r"org/ft1-gptq is a GPTQ checkpoint and a twin checkpoint at once"):
        asyncio.run(LocalModelIndex(storage_path=storage).add_model("org/ft1-gptq"))


@pytest.mark.parametrize("command", COMMANDS)
def test_help(command):
    """--help of the eight commands, which are registered from the formats, is the text recorded before they were"""
    assert run_cli([command, "--help"]).output == (HELP_DIR / f"{command}.txt").read_text()
