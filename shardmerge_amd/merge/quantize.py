"""The driver of `python -m shard quantize-SUFFIX MODEL --out DIR` and `python -m shard dequantize-SUFFIX MODEL --out DIR`
for every checkpoint format of quantformat.py: a full model turned into a quantised checkpoint and back.

`quantize-SUFFIX` walks MODEL shard by shard and calls the format's `quant` (its ``Engine.*_quant``; the functions are
stated in include/shardmerge_hip.h) on every 2-D ``*.weight`` tensor of the modules named by ``--modules`` that the
format `fits`; it writes the stored tensors into the shard the weight came from and copies every other tensor as it is
- a named module's weight that does not fit too, which is then listed as not converted with the rest.  DIR receives the
shards, ``model.safetensors.index.json`` and a ``config.json`` (MODEL's, when it has one) with the format's
``quantization_config`` block.  `dequantize-SUFFIX` is the inverse through the format's `dequant`.  A MODEL that is a
checkpoint of another format is rejected.  Everything is rejected before anything is read, and DIR is created only
after the last tensor has been converted."""
from __future__ import annotations

import json
import logging
from pathlib import Path
from typing import Dict, List, Optional, Sequence

import torch

from ..adapter import FULL_INDEX, base_tensor_meta, is_adapter_dir, is_bin_only_adapter_dir
from ..deltapack import is_pack_dir
from ..emrpack import is_emr_dir

logger = logging.getLogger(__name__)

DEFAULT_MODULES = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")
DTYPES = {"bf16": torch.bfloat16, "bfloat16": torch.bfloat16, "f16": torch.float16, "float16": torch.float16,
          "f32": torch.float32, "float32": torch.float32}
_QUANTISABLE = ("BF16", "F16", "F32")


class Conversion:
    """fmt: the format (a QuantModel subclass); verb: "quantize" or "dequantize"; options: the format's OPTIONS"""

    def __init__(self, fmt, verb: str, model: str, out_dir: Path, storage_dir: Path, modules: Optional[Sequence[str]] = None,
                 dtype: str = "bf16", index_manager=None, engine=None, **options):
        self.fmt, self.quantising, self.command, self.options = fmt, verb == "quantize", f"{verb}-{fmt.SUFFIX}", options
        self.model, self.out_dir, self.storage_dir = model, Path(out_dir), Path(storage_dir)
        self.modules = list(modules) if modules else list(DEFAULT_MODULES)
        self.dtype = dtype
        self.index_manager, self._engine = index_manager, engine

    def engine(self, device):
        if self._engine is None:
            from ..engine import get_engine
            self._engine = get_engine(device)
        return self._engine

    async def preflight(self) -> Dict[str, tuple]:
        """the checks, on the arguments and the shard headers alone; returns MODEL's stored name -> (shape, dtype)"""
        from .. import distributed
        cmd, fmt = self.command, self.fmt
        fmt.check_options(cmd, **self.options)
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
        held = self.index_manager.quant(self.model)
        if held is not None and type(held) is not fmt:
            raise ValueError(f"{cmd}: {self.model} is {held.A_LABEL} checkpoint; `dequantize-{held.SUFFIX}` first")
        if self.quantising and held is not None:
            raise ValueError(f"{cmd}: {self.model} is {fmt.A_NAME} checkpoint already")
        if not self.quantising and held is None:
            raise ValueError(f"{cmd}: {self.model} {fmt.EXPECTED}")
        return base_tensor_meta(self.index_manager, self.model)

    def quantised(self, name: str, shape, dtype: str) -> bool:
        if len(shape) != 2 or dtype not in _QUANTISABLE or not name.endswith(".weight"):
            return False
        module = name[: -len(".weight")]
        return any(module == m or module.endswith("." + m) for m in self.modules)

    async def run(self, device: str) -> dict:
        from safetensors import safe_open
        meta = await self.preflight()
        eng, fmt = self.engine(device), self.fmt
        weight_map = self.index_manager.model_indexes[self.model]["weight_map"]
        held = self.index_manager.quant(self.model)             # (dequantising: MODEL's checkpoint)
        first = {stored[0]: name for name, stored in held.keys.items()} if held is not None else {}
        extra = held.extra_names if held is not None else set()
        shards: Dict[str, Dict[str, torch.Tensor]] = {}
        tensors: List[dict] = []
        untouched = set()
        for shard in sorted(set(weight_map.values())):
            out = shards[shard] = {}
            with safe_open(str(self.storage_dir / self.model / shard), framework="pt") as fh:
                for stored in sorted(n for n, s in weight_map.items() if s == shard):
                    if stored in first:                         # the first stored tensor of a weight: read with the others
                        name = first[stored]
                        parts = [fh.get_tensor(stored)] + [self.index_manager.load_tensor(self.model, k) for k in held.keys[name][1:]]
                        out[name] = held.dequant(eng, parts, DTYPES[self.dtype], name).cpu()
                        logger.info(f"Dequantised {name} to {self.dtype}")
                        tensors.append({"name": name, "shape": held.shape(name)})
                        continue
                    if stored in extra:
                        continue
                    shape, dtype = meta[stored]
                    t = fh.get_tensor(stored)
                    named = self.quantising and self.quantised(stored, shape, dtype)
                    if named and fmt.fits(shape, **self.options):
                        written, record, line = fmt.quant(eng, t, stored, **self.options)
                        out.update(written)
                        logger.info(f"Quantised {stored}: {line}")
                        tensors.append({"name": stored, "shape": list(shape), **record})
                    else:
                        if named:
                            logger.info(f"Copied {stored}: {fmt.unfit(shape, **self.options)}")
                        out[stored] = t
                        untouched.add(stored.rsplit(".", 1)[0])
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
        if self.quantising:
            config["quantization_config"] = self.fmt.quantization_config(untouched, **self.options)
        else:
            config.pop("quantization_config", None)
            config["torch_dtype"] = str(DTYPES[self.dtype]).replace("torch.", "")
        (self.out_dir / "config.json").write_text(json.dumps(config, indent=2))


def format_table(fmt, report: dict) -> str:
    lines = [f"{report['command']}: {len(report['tensors'])} tensor(s) converted, {len(report['copied'])} module(s) copied as they are"]
    quantised = report["command"] == f"quantize-{fmt.SUFFIX}"
    for t in report["tensors"]:
        shape = "x".join(map(str, t["shape"]))
        more = fmt.columns(t) if quantised else ""
        lines.append(f"{t['name'][-64:]:64s} {shape:>14s}{more}")
    return "\n".join(lines)


async def run_conversion(fmt, verb: str, model: str, out_dir: Path, storage_dir: Path, modules=None, dtype: str = "bf16",
                         device: str = "cuda", **options) -> dict:
    return await Conversion(fmt, verb, model, out_dir, storage_dir, modules, dtype, **options).run(device)
