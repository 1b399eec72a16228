"""DoRA and embedding-LoRA adapters in PEFT's saved layout for the synthetic models of tests/lora_fixtures.py, for
tests/test_dora_host.py and tests/test_dora_gpu.py.

org/dora: DoRA on q_proj / v_proj (lora_A, lora_B and lora_magnitude_vector per module) plus plain embedding LoRA on
embed_tokens (lora_embedding_A / lora_embedding_B); org/dora_full: the checkpoint it stands for, written from
Engine.lora_apply's own output."""
from pathlib import Path
from typing import Dict

import torch

from tests import lora_fixtures as lf

EMBED = "model.embed_tokens"
TARGETS = ("q_proj", "v_proj", "embed_tokens")


def dora_factors(rank: int = 8, seed: int = 91, dtype=torch.bfloat16, mag_dtype=torch.bfloat16,
                 embedding: bool = True) -> Dict[str, torch.Tensor]:
    """PEFT keys -> tensors: lf.adapter_factors for q_proj / v_proj, a magnitude per such module (about the base rows'
    norms, so the merged rows keep their size) and, with `embedding`, embedding factors for embed_tokens"""
    out = lf.adapter_factors(rank, seed=seed, dtype=dtype)
    base = lf.model_tensors(0)
    for ti, (name, shape) in enumerate(lf.TENSORS):
        module = name[: -len(".weight")]
        if f"base_model.model.{module}.lora_A.weight" in out:
            norms = base[name].float().norm(dim=1)
            out[f"base_model.model.{module}.lora_magnitude_vector"] = \
                (norms * (1 + 0.2 * lf.randn((shape[0],), seed + 1000 + ti, 1.0))).to(mag_dtype)
        if embedding and module == EMBED:
            out[f"base_model.model.{module}.lora_embedding_A"] = lf.randn((rank, shape[0]), seed + 2000, 0.05).to(dtype)
            out[f"base_model.model.{module}.lora_embedding_B"] = lf.randn((shape[1], rank), seed + 2001, 0.05).to(dtype)
    return out


def dora_config(rank: int = 8, alpha: float = 16, **extra) -> dict:
    cfg = lf.adapter_config(rank, alpha, use_dora=True, target_modules=list(TARGETS))
    cfg.update(extra)
    return cfg


def materialise(engine, storage: Path, uri: str, base: Dict[str, torch.Tensor], factors: Dict[str, torch.Tensor],
                scale: float) -> Dict[str, torch.Tensor]:
    """the full checkpoint a DoRA / embedding / LoRA adapter stands for, written from Engine.lora_apply's own output"""
    out = {}
    for name, t in base.items():
        k = f"base_model.model.{name[: -len('.weight')]}"
        if f"{k}.lora_A.weight" in factors:
            out[name] = engine.lora_apply(t, factors[f"{k}.lora_A.weight"], factors[f"{k}.lora_B.weight"], scale,
                                          magnitude=factors.get(f"{k}.lora_magnitude_vector")).cpu()
        elif f"{k}.lora_embedding_A" in factors:
            out[name] = engine.lora_apply(t, factors[f"{k}.lora_embedding_A"], factors[f"{k}.lora_embedding_B"], scale,
                                          embedding=True).cpu()
        else:
            out[name] = t
    lf.write_model(storage, uri, out)
    return out


def setup_k3(root: Path, engine, rank: int = 8, alpha: float = 16):
    """base, ft1, ft2, the adapter org/dora and its checkpoint org/dora_full under root/storage"""
    storage = root / "storage"
    base = lf.model_tensors(0)
    lf.write_model(storage, "org/base", base)
    lf.write_model(storage, "org/ft1", lf.model_tensors(1))
    lf.write_model(storage, "org/ft2", lf.model_tensors(2))
    factors = dora_factors(rank)
    lf.write_adapter(storage, "org/dora", factors, dora_config(rank, alpha))
    full = materialise(engine, storage, "org/dora_full", base, factors, alpha / rank)
    return base, factors, full


def k3_models_input(adapter: str):
    """the adapter (or its checkpoint) as the is_input entry, a full finetune as the output one"""
    return [{"model": adapter, "base": "org/base", "alpha": 0.5, "is_input": True},
            {"model": "org/ft2", "base": "org/base", "alpha": 0.3},
            {"model": "org/ft1", "base": "org/base", "alpha": 0.4, "is_output": True}]


def dora_ref(base, a, b, s, m, embedding: bool = False):
    """fp64 of the contract: V = base + s32 * (B @ A) (transposed factors for embeddings), V * m / ||V|| per row"""
    s32 = float(torch.tensor(s, dtype=torch.float32))
    prod = (a.double().T @ b.double().T) if embedding else (b.double() @ a.double())
    v = base.double() + s32 * prod
    if m is None:
        return v, None
    f = m.double() / torch.linalg.norm(v, dim=1)
    return v * f[:, None], f
