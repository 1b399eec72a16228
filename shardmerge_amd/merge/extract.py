"""LoraExtraction: the driver of `python -m shard extract-lora MODEL --base BASE --rank R --out DIR` - a full finetune
turned into a PEFT LoRA adapter, the other direction of adapter.py.

It walks MODEL and BASE tensor by tensor through ``LocalModelIndex`` and the prefetching loader, as ``analyze`` walks a
config, and calls ``Engine.lora_extract`` (``smhip_lora_extract``; the function is stated in include/shardmerge_hip.h) on
every 2-D ``<module>.weight`` that differs from the base (``--modules``: only the modules whose name ends in one of the
given suffixes).  ``embed_tokens`` becomes an embedding-LoRA pair with the roles swapped as the reader defines them
(``lora_embedding_A = B^T``, ``lora_embedding_B = A^T``).  A tensor that differs but cannot be a LoRA pair - a 1-D norm,
anything of rank > 2 - is warned about, listed under ``skipped`` with ``||delta|| / ||base||`` and NOT written:
``modules_to_save`` is what the reader rejects.  ``lora_alpha = r`` (scale 1); a module whose ``min(rows, cols) < r`` is
extracted at that rank and listed in ``rank_pattern`` and, so that its scale stays 1, in ``alpha_pattern``.  Everything
is rejected before anything is read, and DIR is created only after the last tensor has been extracted."""
from __future__ import annotations

import json
import logging
import math
import os
from pathlib import Path
from typing import Dict, List, Optional, Sequence

import torch

from ..adapter import ADAPTER_CONFIG, ADAPTER_WEIGHTS, KEY_PREFIX, base_tensor_meta, is_adapter_dir, is_bin_only_adapter_dir

logger = logging.getLogger(__name__)

MAX_RANK = 256                                      # smhip_lora_extract
REPORT = "extraction.json"
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
_ST_DTYPES = ("BF16", "F16", "F32")
EMBEDDING_MODULES = ("embed_tokens",)


def parse_modules(text: Optional[str]) -> Optional[List[str]]:
    if text is None:
        return None
    mods = [piece.strip() for piece in text.split(",") if piece.strip()]
    if not mods:
        raise ValueError(f"--modules {text!r} names no module")
    return mods


class LoraExtraction:
    def __init__(self, model: str, base: str, rank: int, out_dir: Path, storage_dir: Path, modules: Optional[Sequence[str]] = None,
                 power_iters: int = 2, factor_dtype: torch.dtype = torch.bfloat16, seed: int = 0, index_manager=None, engine=None):
        self.model, self.base, self.rank, self.out_dir = model, base, rank, Path(out_dir)
        self.storage_dir, self.modules = Path(storage_dir), list(modules) if modules else None
        self.power_iters, self.factor_dtype, self.seed = power_iters, factor_dtype, seed
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
        if isinstance(self.rank, bool) or not isinstance(self.rank, int) or not (1 <= self.rank <= MAX_RANK):
            raise ValueError(f"extract-lora: rank {self.rank!r} is not in 1..{MAX_RANK}")
        if not (0 <= self.power_iters <= 4):
            raise ValueError(f"extract-lora: power_iters {self.power_iters} is not in 0..4")
        if distributed.world_size() > 1:
            raise ValueError("extract-lora runs in a single process: multi-GPU extraction is not supported (run it without torchrun)")
        if self.model == self.base:
            raise ValueError(f"extract-lora: MODEL and --base are both {self.model}")
        for uri in (self.model, self.base):
            path = self.storage_dir / uri
            if is_adapter_dir(path) or is_bin_only_adapter_dir(path):
                raise ValueError(f"extract-lora: {uri} is itself an adapter directory; a full model is expected")
            from ..deltapack import is_pack_dir
            if is_pack_dir(path):
                raise ValueError(f"extract-lora: {uri} is a delta pack directory; a full model is expected")
            from ..emrpack import is_emr_dir
            if is_emr_dir(path):
                raise ValueError(f"extract-lora: {uri} is an EMR pack directory; a full model is expected")
        if (self.out_dir / ADAPTER_WEIGHTS).exists() or (self.out_dir / ADAPTER_CONFIG).exists():
            raise ValueError(f"extract-lora: {self.out_dir} already holds an adapter; it is not overwritten")
        if self.index_manager is None:
            from ..index import LocalModelIndex
            self.index_manager = LocalModelIndex(storage_path=self.storage_dir)
        await self.index_manager.add_model(self.model)
        await self.index_manager.add_model(self.base)
        meta, base_meta = base_tensor_meta(self.index_manager, self.model), base_tensor_meta(self.index_manager, self.base)
        if set(meta) != set(base_meta):
            odd = sorted(set(meta) ^ set(base_meta))
            raise ValueError(f"extract-lora: {self.model} and {self.base} do not hold the same tensors ({', '.join(odd[:4])}{' ...' if len(odd) > 4 else ''})")
        for name, (shape, dtype) in meta.items():
            bshape, bdtype = base_meta[name]
            if list(shape) != list(bshape) or dtype != bdtype:
                raise ValueError(f"extract-lora: tensor {name} is {list(shape)} {dtype} in {self.model} and {list(bshape)} {bdtype} in {self.base}")
        return meta

    def selected(self, name: str, shape, dtype: str) -> Optional[str]:
        """the module a tensor is extracted for: a 2-D <module>.weight of a supported dtype (and of --modules), else None"""
        if not name.endswith(".weight") or len(shape) != 2 or dtype not in _ST_DTYPES:
            return None
        module = name[: -len(".weight")]
        if self.modules is not None and not any(module == m or module.endswith("." + m) for m in self.modules):
            return None
        return module

    def unselected(self, name: str, shape, dtype: str) -> bool:
        """a Linear weight that --modules leaves out: not read at all"""
        return self.modules is not None and name.endswith(".weight") and len(shape) == 2 and dtype in _ST_DTYPES and \
            self.selected(name, shape, dtype) is None

    async def _fetch(self, uri: str, name: str, device: str) -> torch.Tensor:
        if self._loader is not None:
            t = self._loader.take(uri, name)
            if t is not None:
                return t
        return await self.index_manager.get_tensor(uri, name, device=device).get()

    # ---- the walk ----------------------------------------------------------------------------------------------------
    async def extract(self, device: str) -> dict:
        meta = await self.preflight()
        eng = self.engine(device)
        dev = str(eng.device)
        order = [n for n in self.index_manager.get_layer_order(self.model)]
        todo = [n for n in order if not self.unselected(n, *meta[n])]
        not_selected = [n for n in order if self.unselected(n, *meta[n])]
        schedule = [[(self.model, n), (self.base, n)] for n in todo]
        if os.environ.get("SHARDMERGE_PREFETCH", "1") != "0" and schedule:
            from ..loader import PrefetchLoader
            self._loader = PrefetchLoader(self.index_manager, dev)
            self._loader.start(schedule)
        factors: Dict[str, torch.Tensor] = {}
        tensors, skipped, unchanged = [], [], []
        rank_pattern: Dict[str, int] = {}
        try:
            for pos, name in enumerate(todo):
                if self._loader is not None:
                    self._loader.begin_layer(pos)
                ft = await self._fetch(self.model, name, dev)
                bs = await self._fetch(self.base, name, dev)
                if torch.equal(ft, bs):
                    unchanged.append(name)
                    continue
                module = self.selected(name, *meta[name])
                if module is None:
                    fdt = ft.dtype if ft.dtype in DTYPES.values() else torch.float32
                    dsq = eng.delta_stats([ft.to(fdt)], [bs.to(fdt)], [1.0], [1.0], layer_name=name).gram[0][0]
                    bn = eng.exact_norm(bs)
                    rel = math.sqrt(dsq) / bn if bn > 0 else float("inf")
                    logger.warning(f"{name} {list(ft.shape)} differs from the base (||delta|| / ||base|| = {rel:.3e}) and is not a "
                                   "Linear weight: it is NOT part of the adapter")
                    skipped.append({"name": name, "shape": list(ft.shape), "relative_delta": rel})
                    continue
                rows, cols = ft.shape
                r = min(self.rank, rows, cols)
                a, b, rep = eng.lora_extract(ft, bs, r, power_iters=self.power_iters, factor_dtype=self.factor_dtype,
                                             seed=self.seed, name=name)
                if r != self.rank:
                    rank_pattern[module] = r
                if module.split(".")[-1] in EMBEDDING_MODULES:
                    factors[f"{KEY_PREFIX}{module}.lora_embedding_A"] = b.t().contiguous().cpu()
                    factors[f"{KEY_PREFIX}{module}.lora_embedding_B"] = a.t().contiguous().cpu()
                else:
                    factors[f"{KEY_PREFIX}{module}.lora_A.weight"] = a.cpu()
                    factors[f"{KEY_PREFIX}{module}.lora_B.weight"] = b.cpu()
                logger.info(f"Extracted {name}: r {r}, effective rank {rep.effective_rank}, energy share {rep.share:.6f}")
                tensors.append({"name": name, "module": module, "shape": [rows, cols], "r": r, "rho": rep.effective_rank,
                                "sigma": rep.sigma, "orth_ranks": rep.orth_ranks, "delta_sq": rep.delta_sq, "share": rep.share,
                                "residual_bound": rep.residual_bound})
        finally:
            if self._loader is not None:
                self._loader.close()
                self._loader = None
        if not factors:
            raise ValueError(f"extract-lora: no Linear weight of {self.model} differs from {self.base}"
                             + (f" among the modules {self.modules}" if self.modules else "") + "; nothing to write")
        config = {"peft_type": "LORA", "task_type": "CAUSAL_LM", "r": self.rank, "lora_alpha": self.rank, "lora_dropout": 0.0,
                  "target_modules": sorted({t["module"].split(".")[-1] for t in tensors}), "bias": "none", "fan_in_fan_out": False,
                  "use_rslora": False, "use_dora": False, "modules_to_save": None, "rank_pattern": rank_pattern,
                  "alpha_pattern": dict(rank_pattern), "base_model_name_or_path": self.base}
        report = {"model": self.model, "base": self.base, "rank": self.rank, "power_iters": self.power_iters, "seed": self.seed,
                  "factor_dtype": next(k for k, v in DTYPES.items() if v == self.factor_dtype), "tensors": tensors,
                  "skipped": skipped, "unchanged": unchanged, "not_selected": not_selected}
        self.write(factors, config, report)
        return report

    def write(self, factors: Dict[str, torch.Tensor], config: dict, report: dict):
        from safetensors.torch import save_file
        self.out_dir.mkdir(parents=True, exist_ok=True)
        save_file({k: factors[k] for k in sorted(factors)}, str(self.out_dir / ADAPTER_WEIGHTS), metadata={"format": "pt"})
        (self.out_dir / ADAPTER_CONFIG).write_text(json.dumps(config, indent=2))
        (self.out_dir / REPORT).write_text(json.dumps(report, indent=1))


def format_table(report: dict) -> str:
    lines = [f"{len(report['tensors'])} tensor(s) extracted at rank {report['rank']} ({report['power_iters']} power iterations), "
             f"{len(report['unchanged'])} unchanged, {len(report['skipped'])} skipped",
             f"{'tensor':56s} {'shape':>14s} {'r':>4s} {'rho':>4s} {'share':>9s} {'residual':>9s}"]
    for t in report["tensors"]:
        lines.append(f"{t['name'][-56:]:56s} {'x'.join(map(str, t['shape'])):>14s} {t['r']:4d} {t['rho']:4d} {t['share']:9.6f} {t['residual_bound']:9.2e}")
    for s in report["skipped"]:
        lines.append(f"skipped (not in the adapter): {s['name']} {s['shape']}, ||delta|| / ||base|| = {s['relative_delta']:.3e}")
    return "\n".join(lines)


async def run_extraction(model: str, base: str, rank: int, out_dir: Path, storage_dir: Path, modules=None, power_iters: int = 2,
                         factor_dtype: torch.dtype = torch.bfloat16, seed: int = 0, device: str = "cuda") -> dict:
    return await LoraExtraction(model, base, rank, out_dir, storage_dir, modules, power_iters, factor_dtype, seed).extract(device)
