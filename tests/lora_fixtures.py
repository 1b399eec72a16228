"""Synthetic on-disk models and LoRA adapters for tests/test_lora_host.py and tests/test_lora_gpu.py.

storage/org/base, org/ft1, org/ft2: full checkpoints (two shards + index); org/lora: a PEFT-layout adapter of
org/base that targets q_proj and v_proj; every tensor is drawn from a fixed seed."""
import json
from pathlib import Path
from typing import Dict, Optional

import torch
import yaml
from safetensors.torch import save_file

HIDDEN = 128
TENSORS = [
    ("model.embed_tokens.weight", (64, HIDDEN)),
    ("model.layers.0.self_attn.q_proj.weight", (128, HIDDEN)),
    ("model.layers.0.self_attn.k_proj.weight", (64, HIDDEN)),
    ("model.layers.0.self_attn.v_proj.weight", (64, HIDDEN)),
    ("model.layers.0.input_layernorm.weight", (HIDDEN,)),
    ("model.layers.1.self_attn.q_proj.weight", (128, HIDDEN)),
    ("model.layers.1.self_attn.k_proj.weight", (64, HIDDEN)),
    ("model.layers.1.self_attn.v_proj.weight", (64, HIDDEN)),
    ("model.layers.1.input_layernorm.weight", (HIDDEN,)),
    ("model.norm.weight", (HIDDEN,)),
    ("lm_head.weight", (64, HIDDEN)),
]
SHARDS = {"model-00001-of-00002.safetensors": TENSORS[:5], "model-00002-of-00002.safetensors": TENSORS[5:]}
TARGETS = ("q_proj", "v_proj")


def randn(shape, seed, scale):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def model_tensors(which: int) -> Dict[str, torch.Tensor]:
    """which = 0: the base; 1, 2: full finetunes of it"""
    out = {}
    for ti, (name, shape) in enumerate(TENSORS):
        base = randn(shape, 500 + ti, 0.02)
        if which:
            base = base + randn(shape, 500 + 50 * which + ti, 0.003)
        out[name] = base.to(torch.bfloat16)
    return out


def write_model(storage: Path, uri: str, tensors: Dict[str, torch.Tensor]):
    d = storage / uri
    d.mkdir(parents=True, exist_ok=True)
    weight_map = {}
    for shard, items in SHARDS.items():
        save_file({n: tensors[n].contiguous() for n, _ in items}, str(d / shard), metadata={"format": "pt"})
        weight_map.update({n: shard for n, _ in items})
    with open(d / "model.safetensors.index.json", "w") as f:
        json.dump({"metadata": {"total_size": 0}, "weight_map": weight_map}, f)


def adapter_factors(rank: int = 8, seed: int = 77, dtype=torch.bfloat16, zero_b: bool = False, targets=TARGETS,
                    scale: float = 0.05) -> Dict[str, torch.Tensor]:
    """PEFT keys -> factors for every targeted module of TENSORS"""
    out = {}
    for ti, (name, shape) in enumerate(TENSORS):
        if len(shape) != 2 or not any(name.endswith(f".{t}.weight") for t in targets):
            continue
        module = name[: -len(".weight")]
        out[f"base_model.model.{module}.lora_A.weight"] = randn((rank, shape[1]), seed + 2 * ti, scale).to(dtype)
        b = randn((shape[0], rank), seed + 2 * ti + 1, scale).to(dtype)
        out[f"base_model.model.{module}.lora_B.weight"] = torch.zeros_like(b) if zero_b else b
    return out


def adapter_config(rank: int = 8, alpha: float = 16, **extra) -> dict:
    cfg = {"peft_type": "LORA", "task_type": "CAUSAL_LM", "r": rank, "lora_alpha": alpha, "lora_dropout": 0.0,
           "target_modules": list(TARGETS), "bias": "none", "fan_in_fan_out": False, "use_rslora": False,
           "use_dora": False, "modules_to_save": None, "rank_pattern": {}, "alpha_pattern": {},
           "base_model_name_or_path": "org/base"}
    cfg.update(extra)
    return cfg


def write_adapter(storage: Path, uri: str, factors: Dict[str, torch.Tensor], config: dict):
    d = storage / uri
    d.mkdir(parents=True, exist_ok=True)
    save_file({k: v.contiguous() for k, v in factors.items()}, str(d / "adapter_model.safetensors"),
              metadata={"format": "pt"})
    (d / "adapter_config.json").write_text(json.dumps(config, indent=2))


def materialise(engine, storage: Path, uri: str, base: Dict[str, torch.Tensor], factors: Dict[str, torch.Tensor],
                scale: float) -> Dict[str, torch.Tensor]:
    """the full checkpoint the adapter stands for, written from Engine.lora_apply's own output"""
    out = {}
    for name, t in base.items():
        module = name[: -len(".weight")]
        a = factors.get(f"base_model.model.{module}.lora_A.weight")
        if a is None:
            out[name] = t
        else:
            out[name] = engine.lora_apply(t, a, factors[f"base_model.model.{module}.lora_B.weight"], scale).cpu()
    write_model(storage, uri, out)
    return out


def write_config(root: Path, models, out_dir: str, operator: Optional[str] = None) -> Path:
    cfg = {"output_base_model": "org/base", "finetune_merge": models, "output_dir": str(root / out_dir),
           "output_dtype": "bfloat16", "cache_dir": str(root / "cache"), "storage_dir": str(root / "storage")}
    if operator:
        cfg["merge_options"] = {"operator": operator}
    p = root / f"{out_dir}.yaml"
    p.write_text(yaml.safe_dump(cfg))
    return p


def k3_models(third: str):
    """two full finetunes and `third` (an adapter or its materialised checkpoint), which provides the output layers"""
    return [{"model": "org/ft1", "base": "org/base", "alpha": 0.5, "is_input": True},
            {"model": "org/ft2", "base": "org/base", "alpha": 0.3},
            {"model": third, "base": "org/base", "alpha": 0.4, "is_output": True}]


def setup_k3(root: Path, engine, rank: int = 8, alpha: float = 16, zero_b: bool = False):
    """base, ft1, ft2, the adapter org/lora and its checkpoint org/lora_full under root/storage"""
    storage = root / "storage"
    base = model_tensors(0)
    write_model(storage, "org/base", base)
    write_model(storage, "org/ft1", model_tensors(1))
    write_model(storage, "org/ft2", model_tensors(2))
    factors = adapter_factors(rank, zero_b=zero_b)
    write_adapter(storage, "org/lora", factors, adapter_config(rank, alpha))
    full = materialise(engine, storage, "org/lora_full", base, factors, alpha / rank)
    return base, factors, full


def read_outputs(out_dir: Path) -> Dict[str, torch.Tensor]:
    from safetensors import safe_open
    out = {}
    for shard in SHARDS:
        with safe_open(str(out_dir / shard), framework="pt") as f:
            for k in f.keys():
                out[k] = f.get_tensor(k)
    return out


def assert_same_outputs(a: Path, b: Path, file_bytes: bool = True):
    """every output tensor bit-equal (and, file_bytes, every shard file byte-identical)"""
    ta, tb = read_outputs(a), read_outputs(b)
    assert sorted(ta) == sorted(tb) == sorted(n for n, _ in TENSORS)
    for k in ta:
        assert ta[k].dtype == tb[k].dtype and ta[k].shape == tb[k].shape, k
        assert torch.equal(ta[k].view(torch.uint8), tb[k].view(torch.uint8)), k
    if file_bytes:
        for shard in SHARDS:
            assert (a / shard).read_bytes() == (b / shard).read_bytes(), shard
