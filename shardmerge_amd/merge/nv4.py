"""The drivers of `python -m shard quantize-nvfp4 MODEL --out DIR` and `python -m shard dequantize-nvfp4 MODEL --out DIR`:
a full model turned into an NVFP4 checkpoint (nv4model.py) and back.

`quantize-nvfp4` walks MODEL shard by shard and calls ``Engine.nv4_quant`` (``smhip_nv4_quant``; the function is stated
in include/shardmerge_hip.h) on every 2-D ``*.weight`` tensor of the modules named by ``--modules`` whose row length is a
multiple of 16; it writes ``X.weight`` as U8 ``[R, C / 2]``, ``X.weight_scale`` as F8_E4M3 ``[R, C / 16]`` and
``X.weight_scale_2`` as one F32 into the shard the weight came from and copies every other tensor as it is - a named
module's weight with ``C % 16 != 0`` too, which is then listed under ``ignore`` with the rest.  DIR receives the shards,
``model.safetensors.index.json`` and a ``config.json`` (MODEL's, when it has one) with the ``quantization_config`` block.
`dequantize-nvfp4` is the inverse through ``Engine.nv4_dequant``; an ``X.input_scale`` is dropped.  Everything is
rejected before anything is read, and DIR is created only after the last tensor has been converted."""
from __future__ import annotations

import logging
from pathlib import Path
from typing import Dict, List

import torch

from ..nv4model import BLOCK, GLOBAL_SUFFIX, SCALE_SUFFIX, quantization_config
from .fp8 import DTYPES, Fp8Conversion

logger = logging.getLogger(__name__)


class Nv4Conversion(Fp8Conversion):
    """the arguments, the engine, the checks on MODEL and DIR and the writer are the FP8 commands' (merge/fp8.py)"""
    QUANTISE = "quantize-nvfp4"
    quantization_config = staticmethod(quantization_config)

    async def preflight(self) -> Dict[str, tuple]:
        cmd = self.command
        meta = await super().preflight()                        # (its two FP8 checks name the FP8 commands: they pass)
        if self.index_manager.fp8(self.model) is not None:
            raise ValueError(f"{cmd}: {self.model} is a block-scaled FP8 checkpoint; `dequantize-fp8` first")
        if self.index_manager.mx4(self.model) is not None:
            raise ValueError(f"{cmd}: {self.model} is an MXFP4 checkpoint; `dequantize-mxfp4` first")
        is_nv4 = self.index_manager.nv4(self.model) is not None
        if cmd == "quantize-nvfp4" and is_nv4:
            raise ValueError(f"{cmd}: {self.model} is an NVFP4 checkpoint already")
        if cmd == "dequantize-nvfp4" and not is_nv4:
            raise ValueError(f"{cmd}: {self.model} is no NVFP4 checkpoint (quant_algo 'NVFP4' in config.json or "
                             f"hf_quant_config.json and U8 weights with their F8_E4M3 and F32 scales are expected)")
        return meta

    async def run(self, device: str) -> dict:
        from safetensors import safe_open
        meta = await self.preflight()
        eng = self.engine(device)
        weight_map = self.index_manager.model_indexes[self.model]["weight_map"]
        nv4 = self.index_manager.nv4(self.model)
        scale_names = nv4.scale_names if nv4 is not None else set()
        shards: Dict[str, Dict[str, torch.Tensor]] = {}
        tensors: List[dict] = []
        untouched = set()
        for shard in sorted(set(weight_map.values())):
            out = shards[shard] = {}
            with safe_open(str(self.storage_dir / self.model / shard), framework="pt") as fh:
                for name in sorted(n for n, s in weight_map.items() if s == shard and n not in scale_names):
                    shape, dtype = meta[name]
                    t = fh.get_tensor(name)
                    if self.command == "quantize-nvfp4" and self.quantised(name, shape, dtype) and shape[1] % BLOCK == 0:
                        codes, scale, g, rep = eng.nv4_quant(t, layer_name=name)
                        out[name], out[name + SCALE_SUFFIX], out[name + GLOBAL_SUFFIX] = codes.cpu(), scale.cpu(), g
                        logger.info(f"Quantised {name}: {rep.blocks} blocks ({rep.zero_blocks} of zeros, {rep.zero_scale_blocks} "
                                    f"below their scale), {rep.saturated} saturated, {rep.nonfinite} non-finite")
                        tensors.append({"name": name, "shape": list(shape), "blocks": rep.blocks, "zero_blocks": rep.zero_blocks,
                                        "zero_scale_blocks": rep.zero_scale_blocks, "saturated": rep.saturated})
                    elif nv4 is not None and name in nv4.scale_keys:
                        out[name] = eng.nv4_dequant(t, fh.get_tensor(nv4.scale_keys[name]), fh.get_tensor(nv4.global_keys[name]),
                                                    DTYPES[self.dtype], layer_name=name).cpu()
                        logger.info(f"Dequantised {name} to {self.dtype}")
                        tensors.append({"name": name, "shape": nv4.shape(name)})
                    else:
                        if self.command == "quantize-nvfp4" and self.quantised(name, shape, dtype):
                            logger.info(f"Copied {name}: its {shape[1]} columns are no multiple of {BLOCK}")
                        out[name] = t
                        untouched.add(name.rsplit(".", 1)[0])
        if not tensors:
            raise ValueError(f"{self.command}: no tensor of {self.model} belongs to the modules {', '.join(self.modules)}; nothing to write")
        self.write(shards, untouched)
        return {"model": self.model, "command": self.command, "tensors": tensors, "copied": sorted(untouched)}


async def run_nv4(command: str, model: str, out_dir: Path, storage_dir: Path, modules=None, dtype: str = "bf16",
                  device: str = "cuda") -> dict:
    return await Nv4Conversion(command, model, out_dir, storage_dir, modules, dtype).run(device)
