"""EmrTask: the driver of `python -m shard emr-task MODEL --base BASE --unified UNI --out DIR` - one task's modulator on
the unified model of an `operator: emr` merge, written as an EMR pack (emrpack.py): per tensor a 1-bit mask and one
rescaler.

It walks MODEL, BASE and UNI (three full models in the storage directory) tensor by tensor through ``LocalModelIndex``
and the prefetching loader, as ``compress-delta`` does.  A tensor of MODEL that equals BASE bit for bit is omitted; one
whose UNI equals BASE bit for bit (a passthrough tensor of the merge), whose name ends in one of ``--full``'s suffixes
or whose dtype is not BF16 / F16 / F32 is stored whole (``<T>.full``); every other tensor, at any rank, goes through
``Engine.emr_mask`` (``smhip_emr_mask``; the function is stated in include/shardmerge_hip.h).  ``--scale model`` (the
default) is the paper's rescaler over the whole task vector: ``fp32(sum_t A_t / sum_t B_t)`` over the masked tensors in
MODEL's layer order, the two sums in fp64 from 0.0, the same value in every ``<T>.scale``.  Everything is rejected
before anything is read, and DIR is created only after the last tensor."""
from __future__ import annotations

import json
import logging
import math
import os
from pathlib import Path
from typing import Dict, List, Optional, Sequence

import torch

from ..adapter import base_tensor_meta, is_adapter_dir, is_bin_only_adapter_dir
from ..deltapack import is_pack_dir
from ..emrpack import EMR_CONFIG, EMR_WEIGHTS, FORMAT, SCALES, VERSION, is_emr_dir

logger = logging.getLogger(__name__)

REPORT = "emr_task.json"
_ST_DTYPES = ("BF16", "F16", "F32")


def parse_suffixes(text: Optional[str]) -> Optional[List[str]]:
    if text is None:
        return None
    found = [piece.strip() for piece in text.split(",") if piece.strip()]
    if not found:
        raise ValueError(f"emr-task: --full {text!r} names no suffix")
    return found


def resid_of(D2: float, X: float, U2: float, lam: float) -> float:
    """max((D2 - 2 (lam X)) + (lam lam) U2, 0), one rounded fp64 operation at a time (Python floats never fuse)"""
    e = (D2 - 2.0 * (lam * X)) + (lam * lam) * U2
    return e if e > 0.0 else 0.0


class EmrTask:
    def __init__(self, model: str, base: str, unified: str, out_dir: Path, storage_dir: Path, scale: str = "model",
                 full: Optional[Sequence[str]] = None, index_manager=None, engine=None):
        self.model, self.base, self.unified = model, base, unified
        self.out_dir, self.storage_dir = Path(out_dir), Path(storage_dir)
        self.scale = scale
        self.full = list(full) if full else []
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
        if self.scale not in SCALES:
            raise ValueError(f"emr-task: --scale {self.scale!r} is not 'model' or 'tensor'")
        if distributed.world_size() > 1:
            raise ValueError("emr-task runs in a single process: packing on more than one rank is not supported (run it without torchrun)")
        uris = (("MODEL", self.model), ("--base", self.base), ("--unified", self.unified))
        for i, (wa, a) in enumerate(uris):
            for wb, b in uris[i + 1:]:
                if a == b:
                    raise ValueError(f"emr-task: {wa} and {wb} are both {a}")
        for _, uri in uris:
            path = self.storage_dir / uri
            if is_adapter_dir(path) or is_bin_only_adapter_dir(path):
                raise ValueError(f"emr-task: {uri} is an adapter directory; a full model is expected")
            if is_pack_dir(path):
                raise ValueError(f"emr-task: {uri} is a delta pack directory; a full model is expected")
            if is_emr_dir(path):
                raise ValueError(f"emr-task: {uri} is itself an EMR pack directory; a full model is expected")
        if (self.out_dir / EMR_WEIGHTS).exists() or (self.out_dir / EMR_CONFIG).exists():
            raise ValueError(f"emr-task: {self.out_dir} already holds an EMR pack; it is not overwritten")
        if self.index_manager is None:
            from ..index import LocalModelIndex
            self.index_manager = LocalModelIndex(storage_path=self.storage_dir)
        for _, uri in uris:
            await self.index_manager.add_model(uri)
        meta = base_tensor_meta(self.index_manager, self.model)
        for uri in (self.base, self.unified):
            other = base_tensor_meta(self.index_manager, uri)
            if set(meta) != set(other):
                odd = sorted(set(meta) ^ set(other))
                raise ValueError(f"emr-task: {self.model} and {uri} do not hold the same tensors ({', '.join(odd[:4])}{' ...' if len(odd) > 4 else ''})")
            for name, (shape, dtype) in meta.items():
                oshape, odtype = other[name]
                if list(shape) != list(oshape) or dtype != odtype:
                    raise ValueError(f"emr-task: tensor {name} is {list(shape)} {dtype} in {self.model} and {list(oshape)} {odtype} in {uri}")
        return meta

    def whole(self, name: str, dtype: str) -> bool:
        """a tensor that is stored whole whatever the unified model holds: a dtype without a mask, or one of --full"""
        return dtype not in _ST_DTYPES or any(name.endswith(s) for s in self.full)

    async def _fetch(self, uri: str, name: str, device: str) -> torch.Tensor:
        if self._loader is not None:
            t = self._loader.take(uri, name)
            if t is not None:
                return t
        return await self.index_manager.get_tensor(uri, name, device=device).get()

    # ---- the walk ----------------------------------------------------------------------------------------------------
    async def run(self, device: str) -> dict:
        meta = await self.preflight()
        eng = self.engine(device)
        dev = str(eng.device)
        order = list(self.index_manager.get_layer_order(self.model))
        schedule = [[(self.model, n), (self.base, n), (self.unified, n)] for n in order]
        if os.environ.get("SHARDMERGE_PREFETCH", "1") != "0" and schedule:
            from ..loader import PrefetchLoader
            self._loader = PrefetchLoader(self.index_manager, dev)
            self._loader.start(schedule)
        self.begin()
        try:
            for pos, name in enumerate(order):
                if self._loader is not None:
                    self._loader.begin_layer(pos)
                ft = await self._fetch(self.model, name, dev)
                bs = await self._fetch(self.base, name, dev)
                un = await self._fetch(self.unified, name, dev)
                shape, dtype = meta[name]
                kind = self.decide(name, dtype, ft, bs, un)
                if kind == "unchanged":
                    self.add_unchanged(name)
                elif kind == "full":
                    self.add_full(name, shape, dtype, ft)
                else:
                    mask, scale, rep = eng.emr_mask(ft, bs, un, name=name)
                    self.add_masked(name, shape, dtype, ft, mask, scale, rep)
        finally:
            if self._loader is not None:
                self._loader.close()
                self._loader = None
        return self.finish(order)

    # ---- the per-tensor records and the pack they end in: `run` above and the merge that writes its packs itself
    # (merge/emr_packs.py) decide, record and write through these ----------------------------------------------------
    @staticmethod
    def same(a: torch.Tensor, b: torch.Tensor) -> bool:
        """bit for bit"""
        return torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))

    def begin(self):
        self._stored: Dict[str, torch.Tensor] = {}
        self._declared: Dict[str, dict] = {}
        self._records: Dict[str, dict] = {}
        self._unchanged = set()

    def decide(self, name: str, dtype: str, ft: torch.Tensor, bs: torch.Tensor, un: torch.Tensor) -> str:
        """'unchanged': MODEL's tensor is its base's, nothing is stored; 'full': it is stored whole (the unified tensor is
        the base's, a dtype without a mask, one of --full); 'masked' otherwise"""
        if self.same(ft, bs):
            return "unchanged"
        return "full" if self.whole(name, dtype) or self.same(un, bs) else "masked"

    def add_unchanged(self, name: str):
        self._unchanged.add(name)

    def _declare(self, name: str, shape, dtype: str):
        self._declared[name] = {"shape": [int(s) for s in shape], "dtype": dtype}

    def add_full(self, name: str, shape, dtype: str, ft: torch.Tensor):
        nbytes = ft.numel() * ft.element_size()
        self._declare(name, shape, dtype)
        self._stored[f"{name}.full"] = ft.cpu()
        self._records[name] = {"name": name, "shape": list(ft.shape), "stored": "full", "bytes": nbytes, "full_bytes": nbytes}

    def add_masked(self, name: str, shape, dtype: str, ft: torch.Tensor, mask: torch.Tensor, scale: torch.Tensor, rep):
        nbytes = lambda *ts: sum(t.numel() * t.element_size() for t in ts)
        self._declare(name, shape, dtype)
        self._stored[f"{name}.mask"], self._stored[f"{name}.scale"] = mask.cpu(), scale.cpu()
        self._records[name] = {"name": name, "shape": list(ft.shape), "stored": "masked", "rows": rep.rows, "cols": rep.cols,
                               "c": rep.c, "nonzero": rep.nonzero, "A": rep.A, "B": rep.B, "D2": rep.D2, "X": rep.X, "U2": rep.U2,
                               "lambda": rep.lam, "delta_sq": rep.delta_sq, "resid_sq": rep.resid_sq,
                               "bytes": nbytes(mask, scale), "full_bytes": nbytes(ft)}

    def finish(self, order: Sequence[str]) -> dict:
        """the records in `order` (MODEL's layer order: the fp64 sums of --scale model depend on it), the model's
        rescaler, the config and the report; writes the pack and returns the report"""
        stored = self._stored
        declared = {n: self._declared[n] for n in order if n in self._declared}
        tensors = [self._records[n] for n in order if n in self._records]
        unchanged = [n for n in order if n in self._unchanged]
        if not stored:
            raise ValueError(f"emr-task: no tensor of {self.model} differs from {self.base}; nothing to write")
        masked = [t for t in tensors if t["stored"] == "masked"]
        model_lambda = None
        if self.scale == "model" and masked:
            A = B = 0.0
            for t in masked:                                        # MODEL's layer order, fp64 from 0.0
                A, B = A + t["A"], B + t["B"]
            model_lambda = float(torch.tensor(A / B, dtype=torch.float64).to(torch.float32)) if B != 0.0 else 0.0
            one = torch.tensor([model_lambda], dtype=torch.float32)
            for t in masked:
                stored[f"{t['name']}.scale"] = one.clone()
                t["lambda"] = model_lambda
                t["resid_sq"] = resid_of(t["D2"], t["X"], t["U2"], model_lambda)
        for t in masked:
            t["relative_residual"] = math.sqrt(t["resid_sq"] / t["delta_sq"]) if t["delta_sq"] > 0 else 0.0
            logger.info(f"Masked {t['name']}: {t['c']} of {t['rows'] * t['cols']} bits, lambda {t['lambda']:.6g}, "
                        f"relative residual {t['relative_residual']:.4f}")
        config = {"format": FORMAT, "version": VERSION, "base_model_name_or_path": self.base,
                  "unified_model_name_or_path": self.unified, "scale": self.scale, "tensors": declared}
        dsq, rsq = math.fsum(t["delta_sq"] for t in masked), math.fsum(t["resid_sq"] for t in masked)
        report = {"model": self.model, "base": self.base, "unified": self.unified, "scale": self.scale, "full": self.full,
                  "lambda": model_lambda, "tensors": tensors, "unchanged": unchanged,
                  "totals": {"masked": len(masked), "full": len(tensors) - len(masked), "unchanged": len(unchanged),
                             "bytes": sum(t["bytes"] for t in tensors), "full_bytes": sum(t["full_bytes"] for t in tensors),
                             "c": sum(t["c"] for t in masked), "nonzero": sum(t["nonzero"] for t in masked),
                             "elements": sum(t["rows"] * t["cols"] for t in masked),
                             "relative_residual": math.sqrt(rsq / dsq) if dsq > 0 else 0.0}}
        self.write(stored, config, report)
        return report

    def write(self, stored: Dict[str, torch.Tensor], config: dict, report: dict):
        from safetensors.torch import save_file
        self.out_dir.mkdir(parents=True, exist_ok=True)
        save_file({k: stored[k].contiguous() for k in sorted(stored)}, str(self.out_dir / EMR_WEIGHTS), metadata={"format": "pt"})
        (self.out_dir / EMR_CONFIG).write_text(json.dumps(config, indent=2))
        (self.out_dir / REPORT).write_text(json.dumps(report, indent=1))


def format_table(report: dict) -> str:
    tot = report["totals"]
    how = f"one rescaler for the model ({report['lambda']:.6g})" if report["scale"] == "model" and report["lambda"] is not None \
        else "a rescaler per tensor"
    lines = [f"{tot['masked']} tensor(s) masked on {report['unified']}, {how}; {tot['full']} stored whole, {tot['unchanged']} unchanged",
             f"{'tensor':56s} {'shape':>14s} {'mask bits':>12s} {'lambda':>10s} {'residual':>9s} {'bytes':>12s}"]
    for t in report["tensors"]:
        shape = "x".join(map(str, t["shape"]))
        if t["stored"] == "full":
            lines.append(f"{t['name'][-56:]:56s} {shape:>14s} {'whole':>12s} {'':>10s} {'':>9s} {t['bytes']:12d}")
        else:
            lines.append(f"{t['name'][-56:]:56s} {shape:>14s} {t['c']:12d} {t['lambda']:10.6f} {t['relative_residual']:9.4f} {t['bytes']:12d}")
    ratio = tot["full_bytes"] / tot["bytes"] if tot["bytes"] else 0.0
    lines.append(f"total: {tot['bytes']} bytes for {tot['full_bytes']} ({ratio:.1f} x smaller), relative residual {tot['relative_residual']:.4f}")
    return "\n".join(lines)


async def run_emr_task(model: str, base: str, unified: str, out_dir: Path, storage_dir: Path, scale: str = "model", full=None,
                       device: str = "cuda") -> dict:
    return await EmrTask(model, base, unified, out_dir, storage_dir, scale, full).run(device)
