"""The drivers of `python -m shard quantize-gptq MODEL --out DIR` and `python -m shard dequantize-gptq MODEL --out DIR`: a
full model turned into a GPTQ-layout INT4 checkpoint (gptqmodel.py) and back.

`quantize-gptq` walks MODEL shard by shard and calls ``Engine.gptq_quant`` (``smhip_gptq_quant``; the function is stated
in include/shardmerge_hip.h - round to nearest, NOT the GPTQ solver) on every 2-D ``X.weight`` of the modules named by
``--modules`` with ``R % 8 == 0`` and ``C % group_size == 0``; it writes ``X.qweight``, ``X.qzeros``, ``X.scales`` and
``X.g_idx`` into the shard the weight came from, in its place, and copies every other tensor as it is - a named
module's weight that does not fit the shape rule too.  DIR receives the shards, ``model.safetensors.index.json`` and a
``config.json`` (MODEL's, when it has one) with the ``quantization_config`` block.  `dequantize-gptq` is the inverse
through ``Engine.gptq_dequant``.  Everything is rejected before anything is read, and DIR is created only after the
last tensor has been converted."""
from __future__ import annotations

import logging
from pathlib import Path
from typing import Dict, List

import torch

from ..gptqmodel import COMPANIONS, GROUPS, QWEIGHT, WEIGHT_SUFFIX, quantization_config
from .fp8 import DTYPES, Fp8Conversion

logger = logging.getLogger(__name__)


class GptqConversion(Fp8Conversion):
    """the arguments, the engine, the checks on MODEL and DIR and the writer are the FP8 commands' (merge/fp8.py)"""
    QUANTISE = "quantize-gptq"

    def __init__(self, *args, group_size: int = 128, **kwargs):
        super().__init__(*args, **kwargs)
        self.group_size = group_size
        self.quantization_config = lambda not_converted: quantization_config(not_converted, self.group_size)

    async def preflight(self) -> Dict[str, tuple]:
        cmd = self.command
        if self.group_size not in GROUPS:
            raise ValueError(f"{cmd}: --group-size {self.group_size} is not one of {list(GROUPS)}")
        meta = await super().preflight()                        # (its two FP8 checks name the FP8 commands: they pass)
        for what, get, undo in (("a block-scaled FP8", self.index_manager.fp8, "dequantize-fp8"),
                                ("an MXFP4", self.index_manager.mx4, "dequantize-mxfp4"),
                                ("an NVFP4", self.index_manager.nv4, "dequantize-nvfp4")):
            if get(self.model) is not None:
                raise ValueError(f"{cmd}: {self.model} is {what} checkpoint; `{undo}` first")
        is_gptq = self.index_manager.gptq(self.model) is not None
        if cmd == "quantize-gptq" and is_gptq:
            raise ValueError(f"{cmd}: {self.model} is a GPTQ checkpoint already")
        if cmd == "dequantize-gptq" and not is_gptq:
            raise ValueError(f"{cmd}: {self.model} is no GPTQ checkpoint (quant_method 'gptq' in config.json and I32 "
                             f"qweight tensors with their qzeros, scales and g_idx are expected)")
        return meta

    def fits(self, shape) -> bool:
        return shape[0] % 8 == 0 and shape[1] % self.group_size == 0

    async def run(self, device: str) -> dict:
        from safetensors import safe_open
        meta = await self.preflight()
        eng = self.engine(device)
        weight_map = self.index_manager.model_indexes[self.model]["weight_map"]
        gptq = self.index_manager.gptq(self.model)
        stored = gptq.stored_names if gptq is not None else set()
        shards: Dict[str, Dict[str, torch.Tensor]] = {}
        tensors: List[dict] = []
        untouched = set()
        for shard in sorted(set(weight_map.values())):
            out = shards[shard] = {}
            with safe_open(str(self.storage_dir / self.model / shard), framework="pt") as fh:
                for name in sorted(n for n, s in weight_map.items() if s == shard):
                    shape, dtype = meta[name]
                    if name in stored:
                        if not name.endswith(QWEIGHT):
                            continue                            # (a companion: read with its qweight)
                        stem = name[: -len(QWEIGHT)]
                        four = [fh.get_tensor(name)] + [await self.index_manager.get_tensor(self.model, stem + c, device="cpu").get()
                                                        for c in COMPANIONS]
                        out[stem + WEIGHT_SUFFIX] = eng.gptq_dequant(*four, DTYPES[self.dtype], layer_name=stem + WEIGHT_SUFFIX).cpu()
                        logger.info(f"Dequantised {stem + WEIGHT_SUFFIX} to {self.dtype}")
                        tensors.append({"name": stem + WEIGHT_SUFFIX, "shape": gptq.shape(stem + WEIGHT_SUFFIX)})
                        continue
                    t = fh.get_tensor(name)
                    if self.command == "quantize-gptq" and self.quantised(name, shape, dtype) and self.fits(shape):
                        stem = name[: -len(WEIGHT_SUFFIX)]
                        *four, rep = eng.gptq_quant(t, self.group_size, layer_name=name)
                        for suffix, v in zip((QWEIGHT,) + COMPANIONS, four):
                            out[stem + suffix] = v.cpu()
                        logger.info(f"Quantised {name}: {rep.groups} groups of {self.group_size} ({rep.zero_groups} of zeros, "
                                    f"{rep.scale_clamped} with a clamped scale), {rep.clipped} clipped, {rep.nonfinite} non-finite")
                        tensors.append({"name": name, "shape": list(shape), "groups": rep.groups, "zero_groups": rep.zero_groups,
                                        "scale_clamped": rep.scale_clamped, "clipped": rep.clipped})
                    else:
                        if self.command == "quantize-gptq" and self.quantised(name, shape, dtype):
                            logger.info(f"Copied {name}: {list(shape)} is not rows a multiple of 8 by columns a multiple of {self.group_size}")
                        out[name] = t
                        untouched.add(name.rsplit(".", 1)[0])
        if not tensors:
            raise ValueError(f"{self.command}: no tensor of {self.model} belongs to the modules {', '.join(self.modules)}; nothing to write")
        self.write(shards, untouched)
        return {"model": self.model, "command": self.command, "tensors": tensors, "copied": sorted(untouched)}


async def run_gptq(command: str, model: str, out_dir: Path, storage_dir: Path, modules=None, dtype: str = "bf16",
                   device: str = "cuda", group_size: int = 128) -> dict:
    return await GptqConversion(command, model, out_dir, storage_dir, modules, dtype, group_size=group_size).run(device)
