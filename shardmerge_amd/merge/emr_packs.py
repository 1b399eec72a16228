"""EmrPackMerge: `python -m shard merge CONFIG --emr-packs DIR --emr-unified NAME` - the `operator: emr` merge that also
writes every entry's EMR pack (emrpack.py), the directory `emr-task MODEL --base BASE --unified NAME` would write
afterwards from three more walks over full models: the same safetensors keys and bytes, the same emr_config.json and
emr_task.json.

Every tensor `emr-task` reads for a block tensor is on the device during the merge - the finetunes and their bases are
its inputs, the unified tensor its output - so a block tensor goes through ``Engine.emr_merge_masks``
(``smhip_emr_merge_masks``, one fused pass) instead of one ``emr_merge`` and K ``emr_mask`` calls, and nothing more is
read for it.  A passthrough tensor (embeddings, final norm, head) is the one kind for which this run reads more than a
plain merge: every entry's finetune and base tensor come in as well and go through ``Engine.emr_mask`` against the tensor
the merge passes through.  Per tensor and entry the decision is ``EmrTask.decide``'s, the records, the model's rescaler,
the config, the report and the files are ``EmrTask``'s own (merge/emr_task.py); the planes stay in host memory until the
walk has ended and the packs are written after the output's last shard.

EmrMerge itself stays what it is - the operator of a merge without these options, byte for byte - and this subclass is
chosen by ``run_merge`` when the options are given."""
from __future__ import annotations

import logging
import os
from dataclasses import dataclass, field
from pathlib import Path
from typing import Dict, List, Optional

import torch

from ..adapter import base_tensor_meta, is_adapter_dir, is_bin_only_adapter_dir
from ..constants import INPUT_LAYER, OUTPUT_LAYER
from ..deltapack import is_pack_dir
from ..emrpack import EMR_CONFIG, EMR_WEIGHTS, SCALES, is_emr_dir
from ..writer import ShardLayer
from .emr import EmrMerge
from .emr_task import EmrTask, parse_suffixes

logger = logging.getLogger(__name__)

_ST_NAME = {torch.bfloat16: "BF16", torch.float16: "F16", torch.float32: "F32"}


@dataclass
class EmrPackOptions:
    """--emr-packs DIR, --emr-unified NAME, --emr-scale model|tensor, --emr-full SUFFIXES of `merge`"""
    packs: Optional[Path] = None
    unified: Optional[str] = None
    scale: Optional[str] = None
    full: Optional[str] = None
    suffixes: List[str] = field(default_factory=list)

    @property
    def asked(self) -> bool:
        return self.packs is not None

    def pack_dir(self, model: str) -> Path:
        return Path(self.packs) / f"{model}-emr"

    def check(self, config):
        """what the options and the config alone show, before an index is built: ValueError naming the option and the cause"""
        from .. import distributed
        if not self.asked:
            for opt, value in (("--emr-unified", self.unified), ("--emr-scale", self.scale), ("--emr-full", self.full)):
                if value is not None:
                    raise ValueError(f"{opt} is accepted only with --emr-packs")
            return
        if config.operator != "emr":
            raise ValueError(f"--emr-packs requires operator: emr (operator '{config.operator}' elects no unified model)")
        if not self.unified:
            raise ValueError("--emr-packs requires --emr-unified NAME: the name under storage_dir at which the merged model will be found")
        if self.scale is not None and self.scale not in SCALES:
            raise ValueError(f"--emr-scale {self.scale!r} is not 'model' or 'tensor'")
        try:
            self.suffixes = parse_suffixes(self.full) or []
        except ValueError as exc:
            raise ValueError(str(exc).replace("emr-task: --full", "--emr-full")) from exc
        if distributed.world_size() > 1:
            raise ValueError("--emr-packs runs in a single process: packing on more than one rank is not supported (run it without torchrun, "
                             "or run emr-task afterwards)")
        for var in ("SHARDMERGE_FORCE_DIST", "SHARDMERGE_INPLACE"):
            if os.environ.get(var) == "1":
                raise ValueError(f"--emr-packs does not run on the partitioned path: unset {var}, or run emr-task afterwards")
        storage = Path(config.storage_path)
        seen = set()
        for m in config.finetune_merge:
            if m.start_layer != 0 or m.end_layer != -1:
                raise ValueError(f"--emr-packs: entry {m.model} has a layer window ({m.start_layer}..{m.end_layer}); a pack stands for the "
                                 f"whole model")
            if m.model in seen:
                raise ValueError(f"--emr-packs: two entries are {m.model}; their packs would be one directory")
            seen.add(m.model)
            for role, uri in (("entry", m.model), ("base", m.base)):
                path = storage / uri
                kinds = (("an adapter", is_adapter_dir(path) or is_bin_only_adapter_dir(path)), ("a delta pack", is_pack_dir(path)),
                         ("an EMR pack", is_emr_dir(path)))
                kind = next((k for k, hit in kinds if hit), None)
                if kind is not None:
                    raise ValueError(f"--emr-packs: {role} {uri} is {kind} directory; a full model is expected")
        for what, uri in [(f"entry {m.model}", m.model) for m in config.finetune_merge] + \
                         [(f"base {m.base}", m.base) for m in config.finetune_merge] + [("output_base_model", config.output_base_model)]:
            if self.unified == uri:
                raise ValueError(f"--emr-unified {self.unified} is {what}; the merged model needs a name of its own")
        for m in config.finetune_merge:
            d = self.pack_dir(m.model)
            if (d / EMR_WEIGHTS).exists() or (d / EMR_CONFIG).exists():
                raise ValueError(f"--emr-packs: {d} already holds an EMR pack; it is not overwritten")


class EmrPackMerge(EmrMerge):
    def __init__(self, config, index_manager=None, engine=None, emr_pack_options: Optional[EmrPackOptions] = None, **kwargs):
        super().__init__(config, index_manager=index_manager, engine=engine, **kwargs)
        self.pack_options = emr_pack_options
        self._tasks: List[EmrTask] = []
        self._meta: List[Dict[str, tuple]] = []

    # ---- what only the shard headers and the output directory show: still before anything is read or written ----------
    async def initialize(self):
        await super().initialize()
        cfg, opt = self.config, self.pack_options
        opt.check(cfg)
        want = _ST_NAME.get(cfg.output_astype)
        for uri in dict.fromkeys([cfg.output_base_model] + [u for m in cfg.finetune_merge for u in (m.model, m.base)]):
            for name, (_, dtype) in base_tensor_meta(self.index_manager, uri).items():
                if dtype != want:
                    raise ValueError(f"--emr-packs: output_dtype {cfg.output_dtype} differs from the dtype of {uri} ({name} is {dtype}); "
                                     f"emr-task rejects a unified model of another dtype, and so does this path")
        for shard in sorted(set(self.index_doc["weight_map"].values())):
            if (cfg.output_path / shard).exists():
                raise ValueError(f"--emr-packs: {cfg.output_path} holds the finished shard {shard}; a resumed run has not seen its tensors - "
                                 f"delete the output, or run emr-task afterwards")
        self._meta = [base_tensor_meta(self.index_manager, m.model) for m in cfg.finetune_merge]
        self._tasks = [EmrTask(m.model, m.base, opt.unified, opt.pack_dir(m.model), cfg.storage_path, opt.scale or "model",
                               opt.suffixes, index_manager=self.index_manager) for m in cfg.finetune_merge]
        for task in self._tasks:
            task.begin()

    def get_readme(self) -> str:
        packs = "\n".join(f"- {t.model}: {t.out_dir}" for t in self._tasks)
        return super().get_readme() + (f"EMR packs written by this merge (on the unified model {self.pack_options.unified}, "
                                       f"--emr-scale {self.pack_options.scale or 'model'}):\n{packs}\n")

    # ---- the walk --------------------------------------------------------------------------------------------------
    def _layer_requests(self, shard_layer: ShardLayer):
        """what _merge_layer fetches: a block tensor's reads are the plain merge's; a passthrough tensor's are its
        provider's and, on top, every entry's finetune and base tensor"""
        reqs = super()._layer_requests(shard_layer)
        if shard_layer.layer_number in (INPUT_LAYER, OUTPUT_LAYER):
            name = shard_layer.layer_name
            reqs = reqs + [(u, name) for m in self.config.finetune_merge for u in (m.model, m.base)]
        return list(dict.fromkeys(reqs))

    def _record(self, i: int, name: str, ft, bs, un, masked):
        """entry i's record of one tensor, decided as EmrTask.run decides; masked() -> (mask, scale, EmrMaskReport)"""
        task = self._tasks[i]
        shape, dtype = self._meta[i][name]
        kind = task.decide(name, dtype, ft, bs, un)
        if kind == "unchanged":
            task.add_unchanged(name)
        elif kind == "full":
            task.add_full(name, shape, dtype, ft)
        else:
            mask, scale, rep = masked()
            task.add_masked(name, shape, dtype, ft, mask, scale, rep)

    def merge_block(self, eng, fts, bases, alphas, base_out, name: str):
        if any(t.dtype not in _ST_NAME for t in list(fts) + list(bases) + [base_out]):
            out, report = super().merge_block(eng, fts, bases, alphas, base_out, name)      # (no mask for such a dtype: stored whole)
            masks = scales = mreps = None
        else:
            out, report, masks, scales, mreps = eng.emr_merge_masks(fts, bases, base_out, lam=self.emr_lambda, layer_name=name)
        for i in range(len(fts)):
            self._record(i, name, fts[i], bases[i], out, lambda: (masks[i], scales[i], mreps[i]))
        return out, report

    async def _merge_layer(self, shard_layer: ShardLayer, device: str) -> torch.Tensor:
        number, name = shard_layer.layer_number, shard_layer.layer_name
        if number not in (INPUT_LAYER, OUTPUT_LAYER):
            return await super()._merge_layer(shard_layer, device)
        eng = self.engine(device)
        dev = str(eng.device)
        loaded = {}

        async def fetch(uri):
            if uri not in loaded:
                loaded[uri] = await self._fetch(uri, name, dev)
            return loaded[uri]

        flag = "is_input" if number == INPUT_LAYER else "is_output"
        src = next((m for m in self.config.finetune_merge if getattr(m, flag)), None)
        uri = src.model if src is not None else self.config.output_base_model
        logger.info(f"Passthrough - {name} comes from {uri}")
        out = await fetch(uri)
        for i, m in enumerate(self.config.finetune_merge):
            ft, bs = await fetch(m.model), await fetch(m.base)
            self._record(i, name, ft, bs, out, lambda: eng.emr_mask(ft, bs, out, name=name))
        return out

    async def merge(self, device: str):
        await super().merge(device)                      # (ends after writer.finalize() and the README)
        for m, task in zip(self.config.finetune_merge, self._tasks):
            report = task.finish(list(self.index_manager.get_layer_order(m.model)))
            logger.info(f"EMR pack of {m.model}: {report['totals']['masked']} tensor(s) masked, {report['totals']['full']} stored whole, "
                        f"{report['totals']['unchanged']} unchanged -> {task.out_dir}")
