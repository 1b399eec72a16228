"""Merge-operator base class: the drop-in boundary of the path
(reference shard/merge/base.py:96-223).  Subclasses implement
``async _merge_layer(shard_layer, device) -> Tensor`` and ``get_readme()``;
``merge(device)`` drives initialize -> per-shard loop -> finalize -> README."""
from __future__ import annotations

import logging
import os
from abc import ABC, abstractmethod
from typing import List, Optional, Tuple

import torch

from ..config import MergeConfig, MergeModel
from ..index import LocalModelIndex
from ..writer import ModelWriter, ShardLayer

logger = logging.getLogger(__name__)


class MergeTensorsBase(ABC):
    def __init__(self, config: MergeConfig, index_manager: Optional[LocalModelIndex] = None):
        self.config = config
        self.index_manager = index_manager or LocalModelIndex(config.storage_path, config.cache_path)
        self._loader = None             # PrefetchLoader while merge() runs (loader.py)
        self._layer_pos = {}

    @abstractmethod
    def get_readme(self) -> str:
        return "No readme defined"

    @abstractmethod
    async def _merge_layer(self, shard_layer: ShardLayer, device: str) -> torch.Tensor:
        raise NotImplementedError

    def _layer_requests(self, shard_layer: ShardLayer) -> List[Tuple[str, str]]:
        """(model uri, tensor name) pairs `_merge_layer` will fetch for this layer, in any order;
        operators that list them get their inputs prefetched (loader.py), others load on demand."""
        return []

    def engine(self, device):
        if getattr(self, "_engine", None) is None:
            from ..engine import get_engine
            self._engine = get_engine(device)
        return self._engine

    def _finetune_requests(self, m: MergeModel, layer_name: str) -> List[Tuple[str, str]]:
        """the (uri, tensor) reads `finetune_tensor` makes for entry m: the model's tensor; for a LoRA adapter entry its
        base's tensor and, when the adapter targets it, the two factors; for a delta pack entry its base's tensor and
        the planes and scale, the tensor the pack stores whole, or the base's tensor alone; for an EMR pack entry its
        base's and the unified model's tensor, the mask and the rescaler, the whole tensor, or the base's tensor alone"""
        pack = self.index_manager.pack(m.model)
        if pack is not None:
            t = pack.tensors.get(layer_name)
            if t is None:
                return [(m.base, layer_name)]
            if t.kind == "full":
                return [(m.model, t.full_key)]
            return [(m.base, layer_name), (m.model, t.sign_key), (m.model, t.scale_key)] + \
                ([(m.model, t.mask_key)] if t.mask_key is not None else [])
        emr = self.index_manager.emr(m.model)
        if emr is not None:
            t = emr.tensors.get(layer_name)
            if t is None:
                return [(m.base, layer_name)]
            if t.kind == "full":
                return [(m.model, t.full_key)]
            return [(m.base, layer_name), (emr.unified, layer_name), (m.model, t.mask_key), (m.model, t.scale_key)]
        adapter = self.index_manager.adapter(m.model)
        if adapter is None:
            return [(m.model, layer_name)]
        pair = adapter.pairs.get(layer_name)
        if pair is None:
            return [(m.base, layer_name)]
        return [(m.base, layer_name), (m.model, pair.a_key), (m.model, pair.b_key)] + \
            ([(m.model, pair.m_key)] if pair.m_key is not None else [])

    async def finetune_tensor(self, m: MergeModel, layer_name: str, device: str, fetch=None) -> torch.Tensor:
        """THE finetune tensor of entry m - every operator and the partitioned path resolve finetunes here.  A full
        model's own tensor; for a LoRA adapter entry (adapter.py) base + s * B @ A rounded once into the base's dtype
        on the engine (embedding factors transposed; DoRA rows scaled to their magnitudes, where a zero or non-finite
        row norm raises AdapterError), or the base tensor itself where the adapter does not target it.  For a delta
        pack entry (deltapack.py) `Engine.delta_apply` on the base tensor and the planes, the tensor the pack stores
        whole, or the base tensor itself where the pack holds nothing for it.  For an EMR pack entry (emrpack.py)
        `Engine.emr_apply` on the base tensor, the unified model's tensor, the mask and the rescaler, likewise.
        fetch: async (uri, tensor name) -> tensor, the caller's (caching) reader; default: `_fetch` on `device`."""
        if fetch is None:
            async def fetch(uri, tname):
                return await self._fetch(uri, tname, device)
        pack = self.index_manager.pack(m.model)
        if pack is not None:
            t = pack.tensors.get(layer_name)
            if t is not None and t.kind == "full":
                return await fetch(m.model, t.full_key)
            base = await fetch(m.base, layer_name)
            if t is None:
                return base
            sign = await fetch(m.model, t.sign_key)
            scale = await fetch(m.model, t.scale_key)
            mask = await fetch(m.model, t.mask_key) if t.mask_key is not None else None
            return self.engine(device).delta_apply(base, sign, mask, scale)
        emr = self.index_manager.emr(m.model)
        if emr is not None:
            t = emr.tensors.get(layer_name)
            if t is not None and t.kind == "full":
                return await fetch(m.model, t.full_key)
            base = await fetch(m.base, layer_name)
            if t is None:
                return base
            unified = await fetch(emr.unified, layer_name)
            mask = await fetch(m.model, t.mask_key)
            scale = await fetch(m.model, t.scale_key)
            return self.engine(device).emr_apply(base, unified, mask, scale)
        adapter = self.index_manager.adapter(m.model)
        if adapter is None:
            return await fetch(m.model, layer_name)
        base = await fetch(m.base, layer_name)
        pair = adapter.pairs.get(layer_name)
        if pair is None:
            return base
        a = await fetch(m.model, pair.a_key)
        b = await fetch(m.model, pair.b_key)
        mag = await fetch(m.model, pair.m_key) if pair.m_key is not None else None
        from .._lib import ERR_ROW_NORM, SmhipError
        try:
            return self.engine(device).lora_apply(base, a, b, pair.scale, magnitude=mag,
                                                  embedding=pair.kind == "embedding")
        except SmhipError as e:
            if e.code != ERR_ROW_NORM:
                raise
            from ..adapter import AdapterError
            raise AdapterError(f"LoRA adapter {m.model}: tensor {layer_name} (DoRA): {e.message}") from e

    async def _fetch(self, model_uri: str, layer_name: str, device: str) -> torch.Tensor:
        if self._loader is not None:
            t = self._loader.take(model_uri, layer_name)
            if t is not None:
                return t
        return await self.index_manager.get_tensor(model_uri, layer_name, device=device).get()

    async def get_base_output_tensor(self, shard_layer: ShardLayer, device: str) -> torch.Tensor:
        """fp32 tensor of output_base_model (reference base.py:117-119)."""
        return (await self._fetch(self.config.output_base_model, shard_layer.layer_name, device)).to(torch.float32)

    async def get_delta_for_models(self, models: List[MergeModel], shard_layer: ShardLayer, device: str,
                                   apply_alpha: bool = True) -> List[torch.Tensor]:
        """fp32 (finetune - base) per model, times alpha on request (reference base.py:121-137).
        Kept for API compatibility; the HIP operator forms its deltas on the device instead."""
        bases, out = {}, []
        for m in models:
            if m.base not in bases:
                bases[m.base] = (await self._fetch(m.base, shard_layer.layer_name, device)).to(torch.float32)
            ft = (await self.finetune_tensor(m, shard_layer.layer_name, device)).to(torch.float32)
            out.append((ft - bases[m.base]).detach() * (m.alpha if apply_alpha else 1))
        return out

    async def initialize(self):
        cfg = self.config
        await self.index_manager.add_model(cfg.output_base_model)
        self.index_doc = self.index_manager.model_indexes[cfg.output_base_model]
        for m in cfg.finetune_merge:
            await self.index_manager.add_model(m.base)
            await self.index_manager.add_model(m.model)
        base_keys = self.index_manager.get_model_keys(cfg.output_base_model)
        for m in cfg.finetune_merge:
            adapter = self.index_manager.adapter(m.model)
            if adapter is not None:
                # an adapter's finetune has its base's tensors: check the pairs against the base's shard headers
                if self.index_manager.adapter(m.base) is not None:
                    raise ValueError(f"{m.model}: the base of a LoRA adapter entry must be a full model, {m.base} is an adapter")
                from ..adapter import base_tensor_meta
                adapter.check_against(m.base, base_tensor_meta(self.index_manager, m.base))
            pack = self.index_manager.pack(m.model)
            if pack is not None:
                # a pack's finetune has its base's tensors too: check what it stores against the base's shard headers
                if self.index_manager.pack(m.base) is not None or self.index_manager.adapter(m.base) is not None:
                    kind = "a delta pack" if self.index_manager.pack(m.base) is not None else "an adapter"
                    raise ValueError(f"{m.model}: the base of a delta pack entry must be a full model, {m.base} is {kind}")
                from ..adapter import base_tensor_meta
                pack.check_against(m.base, base_tensor_meta(self.index_manager, m.base))
            emr = self.index_manager.emr(m.model)
            if emr is not None:
                # an EMR pack's finetune has its base's tensors as well: check it against the base's and the unified model's headers
                await self.index_manager.add_model(emr.unified)
                for role, uri in (("base", m.base), ("unified model", emr.unified)):
                    kinds = (("an EMR pack", self.index_manager.emr), ("a delta pack", self.index_manager.pack), ("an adapter", self.index_manager.adapter))
                    kind = next((k for k, get in kinds if get(uri) is not None), None)
                    if kind is not None:
                        raise ValueError(f"{m.model}: the {role} of an EMR pack entry must be a full model, {uri} is {kind}")
                from ..adapter import base_tensor_meta
                emr.check_against(m.base, base_tensor_meta(self.index_manager, m.base))
                emr.check_against(emr.unified, base_tensor_meta(self.index_manager, emr.unified), what="unified model")
            keys = self.index_manager.get_model_keys(m.base if adapter is not None or pack is not None or emr is not None else m.model)
            if keys != base_keys:
                # (the reference means to raise this ValueError too but trips over a missing
                # attribute first - SURVEY quirk Q9; the intended error is raised here)
                raise ValueError(
                    f"Model {m.model} architecture mismatch with base model {cfg.output_base_model}\n"
                    f"Missing keys: {base_keys - keys}\nExtra keys: {keys - base_keys}")

    def _loader_device(self, device: str) -> str:
        """device the prefetched tensors must land on (operators with an engine override this)"""
        return device

    def get_writer(self, layer_order: List[str]) -> ModelWriter:
        return ModelWriter(base_index=self.index_doc, output_path=self.config.output_path,
                           layer_order=layer_order, output_astype=self.config.output_astype)

    async def merge(self, device: str):
        await self.initialize()
        layer_order = self.index_manager.get_layer_order(self.config.output_base_model)
        writer = self.get_writer(layer_order)
        groups = [[sl for sl in group if not sl.written] for group in writer.shard_layers()]
        todo = [sl for group in groups for sl in group]
        schedule = [self._layer_requests(sl) for sl in todo]
        if os.environ.get("SHARDMERGE_PREFETCH", "1") != "0" and any(schedule):
            from ..loader import PrefetchLoader
            self._layer_pos = {sl.layer_name: i for i, sl in enumerate(todo)}
            self._loader = PrefetchLoader(self.index_manager, self._loader_device(device))
            self._loader.start(schedule)
        try:
            for group in groups:
                await self._process_layers(writer, group, device)
        finally:
            if self._loader is not None:
                self._loader.close()
                self._loader = None
        writer.finalize()
        readme = self.get_readme() or "No README defined"
        with open(self.config.output_path / "README.md", "w") as fh:
            fh.write(readme)
        logger.info(f"Merge complete. Output saved to {self.config.output_path}")

    async def _process_layers(self, writer: ModelWriter, shard_layers: List[ShardLayer], device: str):
        shard_layer = None
        try:
            for shard_layer in shard_layers:
                if self._loader is not None:
                    self._loader.begin_layer(self._layer_pos[shard_layer.layer_name])
                out = await self._merge_layer(shard_layer, device)
                writer.add_tensor(shard_layer.layer_name, out)
                del out
        except Exception as exc:
            logger.error(f"Error processing {shard_layer.layer_name if shard_layer else '?'}: {exc}")
            raise
