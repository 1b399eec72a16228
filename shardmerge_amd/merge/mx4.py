"""The drivers of `python -m shard quantize-mxfp4 MODEL --out DIR` and `python -m shard dequantize-mxfp4 MODEL --out DIR`:
a full model turned into an MXFP4 checkpoint (mx4model.py) and back.

`quantize-mxfp4` walks MODEL shard by shard and calls ``Engine.mx4_quant`` (``smhip_mx4_quant``; the function is stated
in include/shardmerge_hip.h) on every 2-D ``*.weight`` tensor of the modules named by ``--modules`` whose row length is a
multiple of 32; it writes ``X.weight`` as U8 ``[R, C / 2]`` and ``X.weight_scale`` as U8 ``[R, C / 32]`` into the shard
the weight came from and copies every other tensor as it is - a named module's weight with ``C % 32 != 0`` too, which
is then listed under ``modules_to_not_convert`` with the rest.  DIR receives the shards, ``model.safetensors.index.json``
and a ``config.json`` (MODEL's, when it has one) with the ``quantization_config`` block.  `dequantize-mxfp4` is the
inverse through ``Engine.mx4_dequant``.  Everything is rejected before anything is read, and DIR is created only after
the last tensor has been converted."""
from __future__ import annotations

import logging
from pathlib import Path
from typing import Dict, List

import torch

from ..mx4model import BLOCK, SCALE_SUFFIX, quantization_config
from .fp8 import DTYPES, Fp8Conversion

logger = logging.getLogger(__name__)


class Mx4Conversion(Fp8Conversion):
    """the arguments, the engine, the checks on MODEL and DIR and the writer are the FP8 commands' (merge/fp8.py)"""
    QUANTISE = "quantize-mxfp4"
    quantization_config = staticmethod(quantization_config)

    async def preflight(self) -> Dict[str, tuple]:
        cmd = self.command
        meta = await super().preflight()                        # (its two FP8 checks name the FP8 commands: they pass)
        if self.index_manager.fp8(self.model) is not None:
            raise ValueError(f"{cmd}: {self.model} is a block-scaled FP8 checkpoint; `dequantize-fp8` first")
        is_mx4 = self.index_manager.mx4(self.model) is not None
        if cmd == "quantize-mxfp4" and is_mx4:
            raise ValueError(f"{cmd}: {self.model} is an MXFP4 checkpoint already")
        if cmd == "dequantize-mxfp4" and not is_mx4:
            raise ValueError(f"{cmd}: {self.model} is no MXFP4 checkpoint (quantization_config.quant_method 'mxfp4' and "
                             f"U8 weights with their U8 scales are expected)")
        return meta

    async def run(self, device: str) -> dict:
        from safetensors import safe_open
        meta = await self.preflight()
        eng = self.engine(device)
        weight_map = self.index_manager.model_indexes[self.model]["weight_map"]
        mx4 = self.index_manager.mx4(self.model)
        scale_names = mx4.scale_names if mx4 is not None else set()
        shards: Dict[str, Dict[str, torch.Tensor]] = {}
        tensors: List[dict] = []
        untouched = set()
        for shard in sorted(set(weight_map.values())):
            out = shards[shard] = {}
            with safe_open(str(self.storage_dir / self.model / shard), framework="pt") as fh:
                for name in sorted(n for n, s in weight_map.items() if s == shard and n not in scale_names):
                    shape, dtype = meta[name]
                    t = fh.get_tensor(name)
                    if self.command == "quantize-mxfp4" and self.quantised(name, shape, dtype) and shape[1] % BLOCK == 0:
                        codes, scale, rep = eng.mx4_quant(t, layer_name=name)
                        out[name], out[name + SCALE_SUFFIX] = codes.cpu(), scale.cpu()
                        logger.info(f"Quantised {name}: {rep.blocks} blocks ({rep.zero_blocks} of zeros), {rep.saturated} "
                                    f"saturated, {rep.nonfinite} non-finite")
                        tensors.append({"name": name, "shape": list(shape), "blocks": rep.blocks, "zero_blocks": rep.zero_blocks,
                                        "saturated": rep.saturated})
                    elif mx4 is not None and name in mx4.scale_keys:
                        out[name] = eng.mx4_dequant(t, fh.get_tensor(mx4.scale_keys[name]), DTYPES[self.dtype], layer_name=name).cpu()
                        logger.info(f"Dequantised {name} to {self.dtype}")
                        tensors.append({"name": name, "shape": mx4.shape(name)})
                    else:
                        if self.command == "quantize-mxfp4" and self.quantised(name, shape, dtype):
                            logger.info(f"Copied {name}: its {shape[1]} columns are no multiple of {BLOCK}")
                        out[name] = t
                        untouched.add(name.rsplit(".", 1)[0])
        if not tensors:
            raise ValueError(f"{self.command}: no tensor of {self.model} belongs to the modules {', '.join(self.modules)}; nothing to write")
        self.write(shards, untouched)
        return {"model": self.model, "command": self.command, "tensors": tensors, "copied": sorted(untouched)}


def format_table(report: dict) -> str:
    lines = [f"{report['command']}: {len(report['tensors'])} tensor(s) converted, {len(report['copied'])} module(s) copied as they are"]
    for t in report["tensors"]:
        shape = "x".join(map(str, t["shape"]))
        more = f" {t['blocks']:8d} blocks  {t['saturated']:8d} saturated" if "blocks" in t else ""
        lines.append(f"{t['name'][-64:]:64s} {shape:>14s}{more}")
    return "\n".join(lines)


async def run_mx4(command: str, model: str, out_dir: Path, storage_dir: Path, modules=None, dtype: str = "bf16",
                  device: str = "cuda") -> dict:
    return await Mx4Conversion(command, model, out_dir, storage_dir, modules, dtype).run(device)
