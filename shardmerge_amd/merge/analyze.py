"""DeltaAnalysis: the driver of `python -m shard analyze CONFIG` - per-tensor task-vector statistics before a merge.

It walks a config exactly as ``merge`` would, with FourierMerge's routing - the ``finetune_merge`` layer windows, each
entry against its own base, adapter entries through ``finetune_tensor``, the prefetching loader through
``_layer_requests`` - and for every block tensor calls ``Engine.delta_stats`` (``smhip_delta_stats``; the function is
stated in include/shardmerge_hip.h) on the finetunes that cover it.  Embeddings, final norm and head pass through in a
merge: they are listed and not analysed.  No tensor is written and no ModelWriter exists: the only file the command
creates is its report, so a later ``merge`` of the same config neither resumes from an analysis nor trips over it.
``merge_options`` are validated by ``MergeConfig.from_yaml`` as always and not otherwise used; the alphas are, in the
election alone."""
from __future__ import annotations

import asyncio
import json
import logging
import math
import os
from pathlib import Path
from typing import Dict, List, Sequence

from ..config import MergeConfig
from ..constants import INPUT_LAYER, OUTPUT_LAYER
from ..writer import ShardLayer
from .base import MergeTensorsBase

logger = logging.getLogger(__name__)

DEFAULT_DENSITIES = (0.05, 0.1, 0.2, 0.5)
MAX_DENSITIES = 4                                   # SMHIP_STATS_MAX_DENSITIES
COUNT_FIELDS = ("kept", "opposed", "alone")         # [q][i] integer fields of a tensor's record


def parse_densities(text: str) -> List[float]:
    """'0.05,0.1' -> [0.05, 0.1]; ValueError on anything but 1..4 numbers in (0, 1]"""
    try:
        dens = [float(piece) for piece in text.split(",")]
    except ValueError:
        raise ValueError(f"{text!r} is not a comma-separated list of numbers") from None
    if not (1 <= len(dens) <= MAX_DENSITIES):
        raise ValueError(f"{len(dens)} densities given, one call takes 1..{MAX_DENSITIES}")
    for rho in dens:
        if not (0.0 < rho <= 1.0):
            raise ValueError(f"density {rho} is not in (0, 1]")
    return dens


def cosine(gij: float, gii: float, gjj: float) -> float:
    """step 3 of smhip_geo_merge: clamp(G_ij / (n_i n_j), -1, 1), 0 when the product of the norms is 0 or not finite"""
    p = math.sqrt(gii) * math.sqrt(gjj)
    if p == 0.0 or not math.isfinite(p):
        return 0.0
    return max(-1.0, min(1.0, gij / p))


class DeltaAnalysis(MergeTensorsBase):
    def __init__(self, config: MergeConfig, densities: Sequence[float] = DEFAULT_DENSITIES, index_manager=None, engine=None, **kwargs):
        super().__init__(config, index_manager)
        self.densities = [float(x) for x in densities]
        self._engine = engine

    def get_readme(self) -> str:
        return ""

    async def _merge_layer(self, shard_layer: ShardLayer, device: str):
        raise NotImplementedError("analyze writes no tensor")

    def _loader_device(self, device: str) -> str:
        return str(self.engine(device).device)

    def _entries(self, number: int) -> List[int]:
        return [i for i, m in enumerate(self.config.finetune_merge) if m.use_layer_index(number)]

    def _layer_requests(self, shard_layer: ShardLayer):
        """what analyze() below fetches: nothing for a passthrough tensor, else FourierMerge's reads but output_base_model's"""
        number, name = shard_layer.layer_number, shard_layer.layer_name
        if number in (INPUT_LAYER, OUTPUT_LAYER):
            return []
        models = [self.config.finetune_merge[i] for i in self._entries(number)]
        reqs = [r for m in models for r in self._finetune_requests(m, name)] + [(m.base, name) for m in models]
        return list(dict.fromkeys(reqs))

    def shard_layers(self) -> List[ShardLayer]:
        """the tensors in the order ``merge`` takes them (ModelWriter.shard_layers: shards by file name, a shard's tensors
        in layer order), read from output_base_model's index alone"""
        order = self.index_manager.get_layer_order(self.config.output_base_model)
        rank = {name: i for i, name in enumerate(order)}
        out = []
        for name, shard in sorted(self.index_doc["weight_map"].items(), key=lambda kv: (kv[1], rank[kv[0]])):
            sl = ShardLayer(rank[name], shard, name, False)
            sl.layer_number                    # raises on unknown names, as merge does
            out.append(sl)
        return out

    async def analyze(self, device: str) -> dict:
        await self.initialize()
        cfg = self.config
        todo = self.shard_layers()
        schedule = [self._layer_requests(sl) for sl in todo]
        if os.environ.get("SHARDMERGE_PREFETCH", "1") != "0" and any(schedule):
            from ..loader import PrefetchLoader
            self._loader = PrefetchLoader(self.index_manager, self._loader_device(device))
            self._loader.start(schedule)
        tensors, passthrough = [], []
        try:
            for pos, sl in enumerate(todo):
                if self._loader is not None:
                    self._loader.begin_layer(pos)
                number, name = sl.layer_number, sl.layer_name
                if number in (INPUT_LAYER, OUTPUT_LAYER):
                    flag = "is_input" if number == INPUT_LAYER else "is_output"
                    src = next((m for m in cfg.finetune_merge if getattr(m, flag)), None)
                    passthrough.append({"name": name, "source": src.model if src is not None else cfg.output_base_model})
                    continue
                tensors.append(await self._analyze_block(name, number, device))
        finally:
            if self._loader is not None:
                self._loader.close()
                self._loader = None
        return {"output_base_model": cfg.output_base_model,
                "models": [{"model": m.model, "base": m.base, "alpha": m.alpha, "start_layer": m.start_layer, "end_layer": m.end_layer}
                           for m in cfg.finetune_merge],
                "densities": self.densities, "tensors": tensors, "passthrough": passthrough,
                "model": model_record(tensors, len(cfg.finetune_merge), len(self.densities))}

    async def _analyze_block(self, name: str, number: int, device: str) -> dict:
        eng = self.engine(device)
        dev = str(eng.device)
        entries = self._entries(number)
        if not entries:
            raise ValueError(f"No finetune covers layer {number} ({name})")
        models = [self.config.finetune_merge[i] for i in entries]
        await asyncio.gather(*(self.index_manager.preload_tensor(u, t) for m in models for u, t in self._finetune_requests(m, name)))
        loaded = {}

        async def fetch(uri, tname=name):
            if (uri, tname) not in loaded:
                loaded[(uri, tname)] = await self._fetch(uri, tname, dev)
            return loaded[(uri, tname)]

        fts = [await self.finetune_tensor(m, name, dev, fetch) for m in models]
        bases = [await fetch(m.base) for m in models]
        rep = eng.delta_stats(fts, bases, [m.alpha for m in models], self.densities, layer_name=name)
        logger.info(f"Analysed {name}: {len(models)} model(s), kept {rep.kept} of {rep.k_keep} asked, conflict {rep.conflict}")
        return {"name": name, "shape": list(fts[0].shape), "n": rep.n, "entries": entries, "nonzero": rep.nonzero, "gram": rep.gram,
                "k_keep": rep.k_keep, "thresholds": rep.thresholds, "kept": rep.kept, "energy": rep.energy, "opposed": rep.opposed,
                "alone": rep.alone, "cover": rep.cover, "conflict": rep.conflict}


def model_record(tensors: List[dict], K: int, m: int) -> dict:
    """the tensors' records summed, indexed by the config's entries: integers exactly, Gram and energies added in tensor
    order in fp64.  covered[i]: the elements of the tensors entry i covers (the denominator of its shares)."""
    rec: Dict[str, object] = {
        "n": 0, "covered": [0] * K, "nonzero": [0] * K, "gram": [[0.0] * K for _ in range(K)],
        "k_keep": [[0] * K for _ in range(m)], "energy": [[0.0] * K for _ in range(m)],
        "cover": [[0] * (K + 1) for _ in range(m)], "conflict": [0] * m}
    for f in COUNT_FIELDS:
        rec[f] = [[0] * K for _ in range(m)]
    for t in tensors:
        ent = t["entries"]
        rec["n"] += t["n"]
        for a, i in enumerate(ent):
            rec["covered"][i] += t["n"]
            rec["nonzero"][i] += t["nonzero"][a]
            for b, j in enumerate(ent):
                rec["gram"][i][j] = rec["gram"][i][j] + t["gram"][a][b]
        for q in range(m):
            rec["conflict"][q] += t["conflict"][q]
            for c, v in enumerate(t["cover"][q]):
                rec["cover"][q][c] += v
            for a, i in enumerate(ent):
                rec["k_keep"][q][i] += t["k_keep"][q]
                rec["energy"][q][i] = rec["energy"][q][i] + t["energy"][q][a]
                for f in COUNT_FIELDS:
                    rec[f][q][i] += t[f][q][a]
    return rec


def format_tables(report: dict) -> str:
    """one table per finetune and the per-density lines, from the ``model`` record, in Python floats"""
    rec, dens, models = report["model"], report["densities"], report["models"]
    share = lambda a, b: a / b if b else 0.0
    lines = [f"{len(report['tensors'])} block tensor(s), {rec['n']} elements analysed; {len(report['passthrough'])} passthrough tensor(s) not analysed"]
    for i, mm in enumerate(models):
        gii = rec["gram"][i][i]
        lines.append("")
        lines.append(f"[{i}] {mm['model']} (vs {mm['base']}, weight {mm['alpha']:g}): norm {math.sqrt(gii):.6g}, "
                     f"nonzero {share(rec['nonzero'][i], rec['covered'][i]):.4f} of {rec['covered'][i]}")
        others = ", ".join(f"[{j}] {cosine(rec['gram'][i][j], gii, rec['gram'][j][j]):+.4f}" for j in range(len(models)) if j != i)
        lines.append(f"    cosine: {others or '-'}")
        lines.append("    density    kept  energy  opposed/kept  alone/kept")
        for q, rho in enumerate(dens):
            kept = rec["kept"][q][i]
            lines.append(f"    {rho:7.4g}  {share(kept, rec['covered'][i]):6.4f}  {share(rec['energy'][q][i], gii):6.4f}  "
                         f"{share(rec['opposed'][q][i], kept):12.4f}  {share(rec['alone'][q][i], kept):10.4f}")
    lines.append("")
    for q, rho in enumerate(dens):
        cover = ", ".join(f"{c}: {share(v, rec['n']):.4f}" for c, v in enumerate(rec["cover"][q]))
        lines.append(f"density {rho:g}: conflict {share(rec['conflict'][q], rec['n']):.4f} of the elements; kept by c finetunes - {cover}")
    return "\n".join(lines)


async def run_analysis(config: MergeConfig, device: str, densities: Sequence[float], report_path: Path) -> dict:
    from ..index import LocalModelIndex
    index_manager = LocalModelIndex(storage_path=config.storage_path, cache_path=config.cache_path)
    report = await DeltaAnalysis(config=config, densities=densities, index_manager=index_manager).analyze(device=device)
    report_path = Path(report_path)
    report_path.parent.mkdir(parents=True, exist_ok=True)
    with open(report_path, "w") as fh:
        json.dump(report, fh, indent=1)
    return report
