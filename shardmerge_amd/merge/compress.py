"""DeltaCompression: the driver of `python -m shard compress-delta MODEL --base BASE --out DIR` - a full finetune turned
into a delta pack (deltapack.py), one or two bits per weight on top of its base.

It walks MODEL and BASE tensor by tensor through ``LocalModelIndex`` and the prefetching loader, as ``extract-lora``
does, and calls ``Engine.delta_pack`` (``smhip_dpack_pack``; the function is stated in include/shardmerge_hip.h) on every
tensor of at least two dimensions that differs from the base (``--modules``: only the modules whose name ends in one of
the given suffixes).  Every other tensor that differs is stored whole (``<T>.full``); a tensor equal to the base is
omitted.  Everything is rejected before anything is read, and DIR is created only after the last tensor has been packed."""
from __future__ import annotations

import json
import logging
import math
import os
from pathlib import Path
from typing import Dict, List, Optional, Sequence

import torch

from ..adapter import base_tensor_meta, is_adapter_dir, is_bin_only_adapter_dir
from ..deltapack import FORMAT, PACK_CONFIG, PACK_WEIGHTS, SCALES, VERSION, is_pack_dir
from ..emrpack import is_emr_dir

logger = logging.getLogger(__name__)

REPORT = "compression.json"
_ST_DTYPES = ("BF16", "F16", "F32")


class DeltaCompression:
    def __init__(self, model: str, base: str, out_dir: Path, storage_dir: Path, bits: int = 1, density: Optional[float] = None,
                 scale: str = "row", modules: Optional[Sequence[str]] = None, index_manager=None, engine=None):
        self.model, self.base, self.out_dir, self.storage_dir = model, base, Path(out_dir), Path(storage_dir)
        self.bits, self.density, self.scale = bits, density, scale
        self.modules = list(modules) if modules else None
        self.index_manager, self._engine = index_manager, engine
        self._loader = None

    def engine(self, device):
        if self._engine is None:
            from ..engine import get_engine
            self._engine = get_engine(device)
        return self._engine

    # ---- what is rejected before anything is read ------------------------------------------------------------------
    async def preflight(self) -> Dict[str, tuple]:
        """the checks, on the arguments and the shard headers alone; returns MODEL's name -> (shape, dtype)"""
        from .. import distributed
        if isinstance(self.bits, bool) or self.bits not in (1, 2):
            raise ValueError(f"compress-delta: --bits {self.bits!r} is not 1 or 2")
        if self.bits == 2 and self.density is None:
            raise ValueError("compress-delta: --bits 2 needs --density, the share of the largest deltas to keep")
        if self.density is None:
            self.density = 1.0
        if isinstance(self.density, bool) or not isinstance(self.density, (int, float)) or not (0.0 < float(self.density) <= 1.0):
            raise ValueError(f"compress-delta: --density {self.density!r} is not in (0, 1]")
        if self.bits == 1 and float(self.density) != 1.0:
            raise ValueError(f"compress-delta: --bits 1 keeps every sign, --density {self.density!r} must be 1 (or left out)")
        if self.scale not in SCALES:
            raise ValueError(f"compress-delta: --scale {self.scale!r} is not 'row' or 'tensor'")
        if distributed.world_size() > 1:
            raise ValueError("compress-delta runs in a single process: packing on more than one rank is not supported (run it without torchrun)")
        if self.model == self.base:
            raise ValueError(f"compress-delta: MODEL and --base are both {self.model}")
        for uri in (self.model, self.base):
            path = self.storage_dir / uri
            if is_adapter_dir(path) or is_bin_only_adapter_dir(path):
                raise ValueError(f"compress-delta: {uri} is an adapter directory; a full model is expected")
            if is_pack_dir(path):
                raise ValueError(f"compress-delta: {uri} is itself a delta pack directory; a full model is expected")
            if is_emr_dir(path):
                raise ValueError(f"compress-delta: {uri} is an EMR pack directory; a full model is expected")
        if (self.out_dir / PACK_WEIGHTS).exists() or (self.out_dir / PACK_CONFIG).exists():
            raise ValueError(f"compress-delta: {self.out_dir} already holds a delta pack; it is not overwritten")
        if self.index_manager is None:
            from ..index import LocalModelIndex
            self.index_manager = LocalModelIndex(storage_path=self.storage_dir)
        await self.index_manager.add_model(self.model)
        await self.index_manager.add_model(self.base)
        meta, base_meta = base_tensor_meta(self.index_manager, self.model), base_tensor_meta(self.index_manager, self.base)
        if set(meta) != set(base_meta):
            odd = sorted(set(meta) ^ set(base_meta))
            raise ValueError(f"compress-delta: {self.model} and {self.base} do not hold the same tensors ({', '.join(odd[:4])}{' ...' if len(odd) > 4 else ''})")
        for name, (shape, dtype) in meta.items():
            bshape, bdtype = base_meta[name]
            if list(shape) != list(bshape) or dtype != bdtype:
                raise ValueError(f"compress-delta: tensor {name} is {list(shape)} {dtype} in {self.model} and {list(bshape)} {bdtype} in {self.base}")
        return meta

    def packed(self, name: str, shape, dtype: str) -> bool:
        """a tensor that is packed when it differs: at least two dimensions, a supported dtype (and of --modules)"""
        if len(shape) < 2 or dtype not in _ST_DTYPES:
            return False
        if self.modules is None:
            return True
        module = name[: -len(".weight")] if name.endswith(".weight") else name
        return any(module == m or module.endswith("." + m) for m in self.modules)

    async def _fetch(self, uri: str, name: str, device: str) -> torch.Tensor:
        if self._loader is not None:
            t = self._loader.take(uri, name)
            if t is not None:
                return t
        return await self.index_manager.get_tensor(uri, name, device=device).get()

    # ---- the walk ----------------------------------------------------------------------------------------------------
    async def compress(self, device: str) -> dict:
        meta = await self.preflight()
        eng = self.engine(device)
        dev = str(eng.device)
        order = list(self.index_manager.get_layer_order(self.model))
        schedule = [[(self.model, n), (self.base, n)] for n in order]
        if os.environ.get("SHARDMERGE_PREFETCH", "1") != "0" and schedule:
            from ..loader import PrefetchLoader
            self._loader = PrefetchLoader(self.index_manager, dev)
            self._loader.start(schedule)
        stored: Dict[str, torch.Tensor] = {}
        declared: Dict[str, dict] = {}
        tensors, unchanged = [], []
        nbytes = lambda *ts: sum(t.numel() * t.element_size() for t in ts if t is not None)
        try:
            for pos, name in enumerate(order):
                if self._loader is not None:
                    self._loader.begin_layer(pos)
                ft = await self._fetch(self.model, name, dev)
                bs = await self._fetch(self.base, name, dev)
                if torch.equal(ft.reshape(-1).view(torch.uint8), bs.reshape(-1).view(torch.uint8)):       # bit for bit
                    unchanged.append(name)
                    continue
                shape, dtype = meta[name]
                declared[name] = {"shape": [int(s) for s in shape], "dtype": dtype}
                if not self.packed(name, shape, dtype):
                    stored[f"{name}.full"] = ft.cpu()
                    tensors.append({"name": name, "shape": list(ft.shape), "stored": "full", "bytes": nbytes(ft),
                                    "full_bytes": nbytes(ft)})
                    continue
                sign, mask, scale, rep = eng.delta_pack(ft, bs, bits=self.bits, density=float(self.density), scale=self.scale, name=name)
                stored[f"{name}.sign"], stored[f"{name}.scale"] = sign.cpu(), scale.cpu()
                if mask is not None:
                    stored[f"{name}.mask"] = mask.cpu()
                logger.info(f"Packed {name}: kept {rep.kept} of {ft.numel()}, relative residual {rep.rel_residual:.4f}")
                tensors.append({"name": name, "shape": list(ft.shape), "stored": "packed", "rows": rep.rows, "cols": rep.cols,
                                "k_keep": rep.k_keep, "kept": rep.kept, "nonzero": rep.nonzero, "threshold": rep.threshold,
                                "delta_sq": rep.delta_sq, "resid_sq": rep.resid_sq, "relative_residual": rep.rel_residual,
                                "bytes": nbytes(sign, mask, scale), "full_bytes": nbytes(ft)})
        finally:
            if self._loader is not None:
                self._loader.close()
                self._loader = None
        if not stored:
            raise ValueError(f"compress-delta: no tensor of {self.model} differs from {self.base}; nothing to write")
        config = {"format": FORMAT, "version": VERSION, "base_model_name_or_path": self.base, "bits": self.bits,
                  "density": float(self.density), "scale": self.scale, "tensors": declared}
        packed = [t for t in tensors if t["stored"] == "packed"]
        dsq, rsq = math.fsum(t["delta_sq"] for t in packed), math.fsum(t["resid_sq"] for t in packed)
        report = {"model": self.model, "base": self.base, "bits": self.bits, "density": float(self.density), "scale": self.scale,
                  "modules": self.modules, "tensors": tensors, "unchanged": unchanged,
                  "totals": {"packed": len(packed), "full": len(tensors) - len(packed), "unchanged": len(unchanged),
                             "bytes": sum(t["bytes"] for t in tensors), "full_bytes": sum(t["full_bytes"] for t in tensors),
                             "kept": sum(t["kept"] for t in packed), "elements": sum(t["rows"] * t["cols"] for t in packed),
                             "relative_residual": math.sqrt(rsq / dsq) if dsq > 0 else 0.0}}
        self.write(stored, config, report)
        return report

    def write(self, stored: Dict[str, torch.Tensor], config: dict, report: dict):
        from safetensors.torch import save_file
        self.out_dir.mkdir(parents=True, exist_ok=True)
        save_file({k: stored[k].contiguous() for k in sorted(stored)}, str(self.out_dir / PACK_WEIGHTS), metadata={"format": "pt"})
        (self.out_dir / PACK_CONFIG).write_text(json.dumps(config, indent=2))
        (self.out_dir / REPORT).write_text(json.dumps(report, indent=1))


def format_table(report: dict) -> str:
    tot = report["totals"]
    lines = [f"{tot['packed']} tensor(s) packed at {report['bits']} bit(s), density {report['density']}, scale per {report['scale']}; "
             f"{tot['full']} stored whole, {tot['unchanged']} unchanged",
             f"{'tensor':56s} {'shape':>14s} {'kept':>12s} {'threshold':>10s} {'residual':>9s} {'bytes':>12s}"]
    for t in report["tensors"]:
        shape = "x".join(map(str, t["shape"]))
        if t["stored"] == "full":
            lines.append(f"{t['name'][-56:]:56s} {shape:>14s} {'whole':>12s} {'':>10s} {'':>9s} {t['bytes']:12d}")
        else:
            lines.append(f"{t['name'][-56:]:56s} {shape:>14s} {t['kept']:12d} {t['threshold']:10.3e} {t['relative_residual']:9.4f} {t['bytes']:12d}")
    ratio = tot["full_bytes"] / tot["bytes"] if tot["bytes"] else 0.0
    lines.append(f"total: {tot['bytes']} bytes for {tot['full_bytes']} ({ratio:.1f} x smaller), relative residual {tot['relative_residual']:.4f}")
    return "\n".join(lines)


async def run_compression(model: str, base: str, out_dir: Path, storage_dir: Path, bits: int = 1, density: Optional[float] = None,
                          scale: str = "row", modules=None, device: str = "cuda") -> dict:
    return await DeltaCompression(model, base, out_dir, storage_dir, bits, density, scale, modules).compress(device)
