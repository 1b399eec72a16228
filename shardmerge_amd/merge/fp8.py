"""The drivers of `python -m shard quantize-fp8 MODEL --out DIR` and `python -m shard dequantize-fp8 MODEL --out DIR`: a
full model turned into a block-scaled FP8 checkpoint (fp8model.py) and back.

`quantize-fp8` walks MODEL shard by shard and calls ``Engine.fp8_quant`` (``smhip_fp8_quant``; the function is stated in
include/shardmerge_hip.h) on every 2-D ``*.weight`` tensor of the modules named by ``--modules``; it writes ``X`` as
F8_E4M3 and ``X_scale_inv`` as F32 into the shard ``X`` came from and copies every other tensor as it is.  DIR receives
the shards, ``model.safetensors.index.json`` and a ``config.json`` (MODEL's, when it has one) with the
``quantization_config`` block, the untouched modules under ``modules_to_not_convert``.  `dequantize-fp8` is the inverse
through ``Engine.fp8_dequant``.  Everything is rejected before anything is read, and DIR is created only after the
last tensor has been converted."""
from __future__ import annotations

import json
import logging
from pathlib import Path
from typing import Dict, List, Optional, Sequence

import torch

from ..adapter import FULL_INDEX, base_tensor_meta, is_adapter_dir, is_bin_only_adapter_dir
from ..deltapack import is_pack_dir
from ..emrpack import is_emr_dir
from ..fp8model import FP8_DTYPE, SCALE_SUFFIX, quantization_config

logger = logging.getLogger(__name__)

DEFAULT_MODULES = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")
DTYPES = {"bf16": torch.bfloat16, "bfloat16": torch.bfloat16, "f16": torch.float16, "float16": torch.float16,
          "f32": torch.float32, "float32": torch.float32}
_QUANTISABLE = ("BF16", "F16", "F32")


class Fp8Conversion:
    QUANTISE = "quantize-fp8"                           # the command that writes quantization_config (merge/mx4.py: its own)
    quantization_config = staticmethod(quantization_config)
    def __init__(self, command: str, model: str, out_dir: Path, storage_dir: Path, modules: Optional[Sequence[str]] = None,
                 dtype: str = "bf16", index_manager=None, engine=None):
        self.command, self.model, self.out_dir, self.storage_dir = command, model, Path(out_dir), Path(storage_dir)
        self.modules = list(modules) if modules else list(DEFAULT_MODULES)
        self.dtype = dtype
        self.index_manager, self._engine = index_manager, engine

    def engine(self, device):
        if self._engine is None:
            from ..engine import get_engine
            self._engine = get_engine(device)
        return self._engine

    async def preflight(self) -> Dict[str, tuple]:
        """the checks, on the arguments and the shard headers alone; returns MODEL's name -> (shape, dtype)"""
        from .. import distributed
        cmd = self.command
        if self.dtype not in DTYPES:
            raise ValueError(f"{cmd}: --dtype {self.dtype!r} is not one of bf16, f16, f32")
        if distributed.world_size() > 1:
            raise ValueError(f"{cmd} runs in a single process (run it without torchrun)")
        path = self.storage_dir / self.model
        for test, what in ((is_adapter_dir, "an adapter"), (is_bin_only_adapter_dir, "an adapter"), (is_pack_dir, "a delta pack"),
                           (is_emr_dir, "an EMR pack")):
            if test(path):
                raise ValueError(f"{cmd}: {self.model} is {what} directory; a full model is expected")
        if self.out_dir.exists() and any(self.out_dir.iterdir()):
            raise ValueError(f"{cmd}: {self.out_dir} exists and is not empty; it is not overwritten")
        if self.index_manager is None:
            from ..index import LocalModelIndex
            self.index_manager = LocalModelIndex(storage_path=self.storage_dir)
        await self.index_manager.add_model(self.model)
        is_fp8 = self.index_manager.fp8(self.model) is not None
        if cmd == "quantize-fp8" and is_fp8:
            raise ValueError(f"{cmd}: {self.model} is an FP8 checkpoint already")
        if cmd == "dequantize-fp8" and not is_fp8:
            raise ValueError(f"{cmd}: {self.model} holds no {FP8_DTYPE} tensor; an FP8 checkpoint is expected")
        return base_tensor_meta(self.index_manager, self.model)

    def quantised(self, name: str, shape, dtype: str) -> bool:
        if len(shape) != 2 or dtype not in _QUANTISABLE or not name.endswith(".weight"):
            return False
        module = name[: -len(".weight")]
        return any(module == m or module.endswith("." + m) for m in self.modules)

    async def run(self, device: str) -> dict:
        from safetensors import safe_open
        meta = await self.preflight()
        eng = self.engine(device)
        weight_map = self.index_manager.model_indexes[self.model]["weight_map"]
        fp8 = self.index_manager.fp8(self.model)
        scale_names = fp8.scale_names if fp8 is not None else set()
        shards: Dict[str, Dict[str, torch.Tensor]] = {}
        tensors: List[dict] = []
        untouched = set()
        for shard in sorted(set(weight_map.values())):
            out = shards[shard] = {}
            with safe_open(str(self.storage_dir / self.model / shard), framework="pt") as fh:
                for name in sorted(n for n, s in weight_map.items() if s == shard and n not in scale_names):
                    shape, dtype = meta[name]
                    t = fh.get_tensor(name)
                    if self.command == "quantize-fp8" and self.quantised(name, shape, dtype):
                        codes, scale, rep = eng.fp8_quant(t, name=name)
                        out[name], out[name + SCALE_SUFFIX] = codes.cpu(), scale.cpu()
                        logger.info(f"Quantised {name}: {rep.blocks} blocks ({rep.zero_blocks} of zeros), amax {rep.amax:.6g}")
                        tensors.append({"name": name, "shape": list(shape), "blocks": rep.blocks, "zero_blocks": rep.zero_blocks,
                                        "amax": rep.amax})
                    elif fp8 is not None and name in fp8.scale_keys:
                        out[name] = eng.fp8_dequant(t, fh.get_tensor(fp8.scale_keys[name]), DTYPES[self.dtype], name=name).cpu()
                        logger.info(f"Dequantised {name} to {self.dtype}")
                        tensors.append({"name": name, "shape": list(shape)})
                    else:
                        out[name] = t
                        untouched.add(name.rsplit(".", 1)[0])
        if not tensors:
            raise ValueError(f"{self.command}: no tensor of {self.model} belongs to the modules {', '.join(self.modules)}; nothing to write")
        self.write(shards, untouched)
        return {"model": self.model, "command": self.command, "tensors": tensors, "copied": sorted(untouched)}

    def write(self, shards: Dict[str, Dict[str, torch.Tensor]], untouched):
        from safetensors.torch import save_file
        src = self.storage_dir / self.model
        self.out_dir.mkdir(parents=True, exist_ok=True)
        weight_map, total = {}, 0
        for shard, tensors in shards.items():
            save_file({k: tensors[k].contiguous() for k in sorted(tensors)}, str(self.out_dir / shard), metadata={"format": "pt"})
            weight_map.update({k: shard for k in tensors})
            total += sum(t.numel() * t.element_size() for t in tensors.values())
        (self.out_dir / FULL_INDEX).write_text(json.dumps({"metadata": {"total_size": total}, "weight_map": dict(sorted(weight_map.items()))}, indent=2))
        config = json.loads((src / "config.json").read_bytes()) if (src / "config.json").exists() else {}
        if self.command == self.QUANTISE:
            config["quantization_config"] = self.quantization_config(untouched)
        else:
            config.pop("quantization_config", None)
            config["torch_dtype"] = str(DTYPES[self.dtype]).replace("torch.", "")
        (self.out_dir / "config.json").write_text(json.dumps(config, indent=2))


def format_table(report: dict) -> str:
    lines = [f"{report['command']}: {len(report['tensors'])} tensor(s) converted, {len(report['copied'])} module(s) copied as they are"]
    for t in report["tensors"]:
        shape = "x".join(map(str, t["shape"]))
        more = f" {t['blocks']:8d} blocks  amax {t['amax']:.6g}" if "blocks" in t else ""
        lines.append(f"{t['name'][-64:]:64s} {shape:>14s}{more}")
    return "\n".join(lines)


async def run_fp8(command: str, model: str, out_dir: Path, storage_dir: Path, modules=None, dtype: str = "bf16",
                  device: str = "cuda") -> dict:
    return await Fp8Conversion(command, model, out_dir, storage_dir, modules, dtype).run(device)
