"""EMR packs as finetunes: one task of an EMR-Merging merge stored as a 1-bit mask and one rescaler per tensor on top of
its base and the unified model.

A ``finetune_merge`` entry ``{model: X, base: Y}`` whose ``storage_dir/X/`` holds ``emr_config.json`` and
``emr_model.safetensors`` and neither ``model.safetensors.index.json``, ``adapter_config.json`` nor ``delta_config.json``
is an EMR entry.  ``python -m shard emr-task`` writes one (merge/emr_task.py).  With U the model that the pack's
``unified_model_name_or_path`` names (a full model in the storage directory), its finetune tensor ``T`` is

  ``Engine.emr_apply(Y[T], U[T], mask, scale)``  when the pack has ``T.mask`` (U8 [R, ceil(C / 8)]) and ``T.scale`` (F32 [1]):
                                                 ``Y[T] + scale * (U[T] - Y[T])`` where the mask bit is set, ``Y[T]`` bit for
                                                 bit elsewhere (the function is stated in include/shardmerge_hip.h,
                                                 smhip_emr_apply);
  ``T.full``                                     when the pack stores the tensor whole, in the model's dtype;
  ``Y[T]`` itself                                otherwise.

``R = shape[0]``, ``C`` the product of the other dimensions; a 0-D or 1-D tensor is one row.  ``emr_config.json`` holds
``format: "shardmerge-emr"``, ``version: 1``, ``base_model_name_or_path``, ``unified_model_name_or_path``, ``scale`` and
under ``tensors`` every stored tensor's ``shape`` and ``dtype``.  Everything this module rejects is rejected before any
output is written, and the message names the pack and the key or field.
"""
from __future__ import annotations

import hashlib
import json
from dataclasses import dataclass
from pathlib import Path
from typing import Dict, List, Optional, Tuple

from .adapter import ADAPTER_CONFIG, FULL_INDEX, read_header
from .deltapack import PACK_CONFIG as DELTA_CONFIG
from .deltapack import plane_shape

EMR_CONFIG = "emr_config.json"
EMR_WEIGHTS = "emr_model.safetensors"
FORMAT = "shardmerge-emr"
VERSION = 1
SUFFIXES = ("mask", "scale", "full")
SCALES = ("model", "tensor")
_DTYPES = ("BF16", "F16", "F32")


class EmrPackError(ValueError):
    """an EMR pack this build cannot read; the message names the pack and the field or tensor key"""


def is_emr_dir(path: Path) -> bool:
    path = Path(path)
    return (path / EMR_CONFIG).exists() and (path / EMR_WEIGHTS).exists() and not (path / FULL_INDEX).exists() \
        and not (path / ADAPTER_CONFIG).exists() and not (path / DELTA_CONFIG).exists()


def emr_identity(path: Path) -> Dict[str, str]:
    """what decides a pack's content for a resumed run: its config bytes and its tensors' header"""
    path = Path(path)
    return {"emr_config": hashlib.sha256((path / EMR_CONFIG).read_bytes()).hexdigest(),
            "emr_header": hashlib.sha256(read_header(path / EMR_WEIGHTS)[0]).hexdigest()}


@dataclass
class EmrTensor:
    kind: str                           # "masked" | "full"
    shape: List[int]
    dtype: str
    mask_key: Optional[str] = None
    scale_key: Optional[str] = None
    full_key: Optional[str] = None


class EmrPack:
    def __init__(self, uri: str, path: Path):
        self.uri = uri
        self.path = Path(path)
        try:
            self.config = json.loads((self.path / EMR_CONFIG).read_bytes())
        except ValueError as exc:
            self._fail(f"{EMR_CONFIG} is not JSON ({exc})")
        self._validate_config()
        _, self.header = read_header(self.path / EMR_WEIGHTS)
        self.identity = emr_identity(self.path)
        self.tensors: Dict[str, EmrTensor] = self._map_keys()       # model tensor name -> what the pack stores for it

    def _fail(self, what: str):
        raise EmrPackError(f"EMR pack {self.uri}: {what}")

    def _validate_config(self):
        c = self.config
        if not isinstance(c, dict) or c.get("format") != FORMAT:
            self._fail(f"format {c.get('format') if isinstance(c, dict) else c!r} is not {FORMAT!r}")
        if c.get("version") != VERSION:
            self._fail(f"version {c.get('version')!r} is not supported (only {VERSION})")
        if c.get("scale") not in SCALES:
            self._fail(f"scale {c.get('scale')!r} is not 'model' or 'tensor'")
        for field in ("base_model_name_or_path", "unified_model_name_or_path"):
            if not isinstance(c.get(field), str):
                self._fail(f"{field} {c.get(field)!r} is not a string")
        if not isinstance(c.get("tensors"), dict):
            self._fail("tensors is not a mapping of tensor names to their shape and dtype")

    @property
    def unified(self) -> str:
        return self.config["unified_model_name_or_path"]

    def _map_keys(self) -> Dict[str, EmrTensor]:
        found: Dict[str, Dict[str, str]] = {}
        for key in self.header:
            name, dot, suffix = key.rpartition(".")
            if not dot or suffix not in SUFFIXES or not name:
                self._fail(f"tensor {key} has an unknown suffix (expected .mask, .scale or .full)")
            found.setdefault(name, {})[suffix] = key
        declared = self.config["tensors"]
        out = {}
        for name, keys in found.items():
            rec = declared.get(name)
            if not isinstance(rec, dict) or not isinstance(rec.get("shape"), list) or not isinstance(rec.get("dtype"), str):
                self._fail(f"tensor {next(iter(keys.values()))}: {EMR_CONFIG} does not give the shape and dtype of {name}")
            shape, dtype = [int(s) for s in rec["shape"]], rec["dtype"]
            if "full" in keys:
                if len(keys) > 1:
                    other = next(k for s, k in keys.items() if s != "full")
                    self._fail(f"tensor {keys['full']} is stored whole, but {other} masks the same tensor")
                f = self.header[keys["full"]]
                if list(f["shape"]) != shape or f["dtype"] != dtype:
                    self._fail(f"tensor {keys['full']} is {f['dtype']} {f['shape']}, {EMR_CONFIG} says {dtype} {shape}")
                out[name] = EmrTensor("full", shape, dtype, full_key=keys["full"])
                continue
            if "mask" not in keys:
                self._fail(f"tensor {next(iter(keys.values()))} has no {name}.mask plane")
            if "scale" not in keys:
                self._fail(f"tensor {keys['mask']} has no {name}.scale")
            if dtype not in _DTYPES:
                self._fail(f"tensor {keys['mask']}: {name} is {dtype} (BF16, F16 or F32 tensors can be masked)")
            rows, pb = plane_shape(shape)
            p = self.header[keys["mask"]]
            if p["dtype"] != "U8" or list(p["shape"]) != [rows, pb]:
                self._fail(f"tensor {keys['mask']} is {p['dtype']} {p['shape']}, U8 [{rows}, {pb}] expected for {name} {shape}")
            sc = self.header[keys["scale"]]
            if sc["dtype"] != "F32" or list(sc["shape"]) != [1]:
                self._fail(f"tensor {keys['scale']} is {sc['dtype']} {sc['shape']}, F32 [1] expected for {name} {shape}")
            out[name] = EmrTensor("masked", shape, dtype, keys["mask"], keys["scale"])
        for name in declared:
            if name not in out:
                self._fail(f"{EMR_CONFIG} lists {name}, but {EMR_WEIGHTS} holds no {name}.mask or {name}.full")
        return out

    def weight_map(self) -> Dict[str, str]:
        return {k: EMR_WEIGHTS for k in self.header}

    def check_against(self, model_uri: str, meta: Dict[str, Tuple[List[int], str]], what: str = "base"):
        """pre-flight of every stored tensor against the shard headers of the base or of the unified model:
        name -> (shape, dtype)"""
        for name, t in self.tensors.items():
            key = t.full_key or t.mask_key
            if name not in meta:
                self._fail(f"tensor {key}: the {what} {model_uri} has no tensor {name}")
            shape, dtype = meta[name]
            if [int(s) for s in shape] != t.shape or dtype != t.dtype:
                self._fail(f"tensor {key} stands for {name} {t.dtype} {t.shape}, the {what} {model_uri} holds it as {dtype} {list(shape)}")
