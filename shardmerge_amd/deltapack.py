"""Delta packs as finetunes: a full finetune stored as one or two bits per weight on top of its base.

A ``finetune_merge`` entry ``{model: X, base: Y}`` whose ``storage_dir/X/`` holds ``delta_config.json`` and
``delta_model.safetensors`` and neither ``model.safetensors.index.json`` nor ``adapter_config.json`` is a pack entry.
``python -m shard compress-delta`` writes one (merge/compress.py).  Its finetune tensor ``T`` is

  ``Engine.delta_apply(Y[T], sign, mask, scale)``  when the pack has ``T.sign`` (U8 [R, ceil(C / 8)]), ``T.scale`` (F32 [R]
                                                   or [1]) and, for a 2-bit pack, ``T.mask``: ``Y[T] +- scale`` where an
                                                   element is kept, ``Y[T]`` bit for bit elsewhere (the function is stated
                                                   in include/shardmerge_hip.h, smhip_dpack_apply);
  ``T.full``                                       when the pack stores the tensor whole, in the model's dtype;
  ``Y[T]`` itself                                  otherwise.

``R = shape[0]``, ``C`` the product of the other dimensions; a 0-D or 1-D tensor is one row.  ``delta_config.json`` holds
``format: "shardmerge-delta"``, ``version: 1``, ``base_model_name_or_path``, ``bits``, ``density``, ``scale`` and under
``tensors`` every stored tensor's ``shape`` and ``dtype``.  Everything this module rejects is rejected before any output
is written, and the message names the pack and the key or field.
"""
from __future__ import annotations

import hashlib
import json
import math
from dataclasses import dataclass
from pathlib import Path
from typing import Dict, List, Optional, Tuple

from .adapter import ADAPTER_CONFIG, FULL_INDEX, read_header

PACK_CONFIG = "delta_config.json"
PACK_WEIGHTS = "delta_model.safetensors"
FORMAT = "shardmerge-delta"
VERSION = 1
SUFFIXES = ("sign", "mask", "scale", "full")
SCALES = ("row", "tensor")
_DTYPES = ("BF16", "F16", "F32")


class DeltaPackError(ValueError):
    """a delta pack this build cannot read; the message names the pack and the field or tensor key"""


def is_pack_dir(path: Path) -> bool:
    path = Path(path)
    return (path / PACK_CONFIG).exists() and (path / PACK_WEIGHTS).exists() and not (path / FULL_INDEX).exists() \
        and not (path / ADAPTER_CONFIG).exists()


def plane_shape(shape) -> Tuple[int, int]:
    """[R, ceil(C / 8)] of a tensor's planes"""
    shape = [int(s) for s in shape]
    rows, cols = (1, math.prod(shape)) if len(shape) <= 1 else (shape[0], math.prod(shape[1:]))
    return rows, (cols + 7) // 8


def pack_identity(path: Path) -> Dict[str, str]:
    """what decides a pack's content for a resumed run: its config bytes and its tensors' header"""
    path = Path(path)
    return {"delta_config": hashlib.sha256((path / PACK_CONFIG).read_bytes()).hexdigest(),
            "delta_header": hashlib.sha256(read_header(path / PACK_WEIGHTS)[0]).hexdigest()}


@dataclass
class PackedTensor:
    kind: str                           # "packed" | "full"
    shape: List[int]
    dtype: str
    sign_key: Optional[str] = None
    mask_key: Optional[str] = None
    scale_key: Optional[str] = None
    full_key: Optional[str] = None


class DeltaPack:
    def __init__(self, uri: str, path: Path):
        self.uri = uri
        self.path = Path(path)
        try:
            self.config = json.loads((self.path / PACK_CONFIG).read_bytes())
        except ValueError as exc:
            self._fail(f"{PACK_CONFIG} is not JSON ({exc})")
        self._validate_config()
        _, self.header = read_header(self.path / PACK_WEIGHTS)
        self.identity = pack_identity(self.path)
        self.tensors: Dict[str, PackedTensor] = self._map_keys()     # model tensor name -> what the pack stores for it

    def _fail(self, what: str):
        raise DeltaPackError(f"delta pack {self.uri}: {what}")

    def _validate_config(self):
        c = self.config
        if not isinstance(c, dict) or c.get("format") != FORMAT:
            self._fail(f"format {c.get('format') if isinstance(c, dict) else c!r} is not {FORMAT!r}")
        if c.get("version") != VERSION:
            self._fail(f"version {c.get('version')!r} is not supported (only {VERSION})")
        if isinstance(c.get("bits"), bool) or c.get("bits") not in (1, 2):
            self._fail(f"bits {c.get('bits')!r} is not 1 or 2")
        d = c.get("density")
        if isinstance(d, bool) or not isinstance(d, (int, float)) or not (0.0 < float(d) <= 1.0):
            self._fail(f"density {d!r} is not in (0, 1]")
        if c["bits"] == 1 and float(d) != 1.0:
            self._fail(f"density {d!r} with bits 1 (a 1-bit pack keeps every sign: density 1)")
        if c.get("scale") not in SCALES:
            self._fail(f"scale {c.get('scale')!r} is not 'row' or 'tensor'")
        if not isinstance(c.get("base_model_name_or_path"), str):
            self._fail(f"base_model_name_or_path {c.get('base_model_name_or_path')!r} is not a string")
        if not isinstance(c.get("tensors"), dict):
            self._fail("tensors is not a mapping of tensor names to their shape and dtype")

    @property
    def bits(self) -> int:
        return int(self.config["bits"])

    def _map_keys(self) -> Dict[str, PackedTensor]:
        found: Dict[str, Dict[str, str]] = {}
        for key in self.header:
            name, dot, suffix = key.rpartition(".")
            if not dot or suffix not in SUFFIXES or not name:
                self._fail(f"tensor {key} has an unknown suffix (expected .sign, .mask, .scale or .full)")
            found.setdefault(name, {})[suffix] = key
        declared = self.config["tensors"]
        out = {}
        for name, keys in found.items():
            rec = declared.get(name)
            if not isinstance(rec, dict) or not isinstance(rec.get("shape"), list) or not isinstance(rec.get("dtype"), str):
                self._fail(f"tensor {next(iter(keys.values()))}: {PACK_CONFIG} does not give the shape and dtype of {name}")
            shape, dtype = [int(s) for s in rec["shape"]], rec["dtype"]
            if "full" in keys:
                if len(keys) > 1:
                    other = next(k for s, k in keys.items() if s != "full")
                    self._fail(f"tensor {keys['full']} is stored whole, but {other} packs the same tensor")
                f = self.header[keys["full"]]
                if list(f["shape"]) != shape or f["dtype"] != dtype:
                    self._fail(f"tensor {keys['full']} is {f['dtype']} {f['shape']}, {PACK_CONFIG} says {dtype} {shape}")
                out[name] = PackedTensor("full", shape, dtype, full_key=keys["full"])
                continue
            if "sign" not in keys:
                self._fail(f"tensor {next(iter(keys.values()))} has no {name}.sign plane")
            if "scale" not in keys:
                self._fail(f"tensor {keys['sign']} has no {name}.scale")
            if self.bits == 2 and "mask" not in keys:
                self._fail(f"tensor {keys['sign']} has no {name}.mask plane, and bits is 2")
            if self.bits == 1 and "mask" in keys:
                self._fail(f"tensor {keys['mask']}: a mask plane, but bits is 1")
            if dtype not in _DTYPES:
                self._fail(f"tensor {keys['sign']}: {name} is {dtype} (BF16, F16 or F32 tensors can be packed)")
            rows, pb = plane_shape(shape)
            for s in ("sign", "mask"):
                if s in keys:
                    p = self.header[keys[s]]
                    if p["dtype"] != "U8" or list(p["shape"]) != [rows, pb]:
                        self._fail(f"tensor {keys[s]} is {p['dtype']} {p['shape']}, U8 [{rows}, {pb}] expected for {name} {shape}")
            sc = self.header[keys["scale"]]
            want = [rows] if self.config["scale"] == "row" else [1]
            if sc["dtype"] != "F32" or list(sc["shape"]) != want:
                self._fail(f"tensor {keys['scale']} is {sc['dtype']} {sc['shape']}, F32 {want} expected for {name} {shape} "
                           f"(scale: {self.config['scale']})")
            out[name] = PackedTensor("packed", shape, dtype, keys["sign"], keys.get("mask"), keys["scale"])
        for name in declared:
            if name not in out:
                self._fail(f"{PACK_CONFIG} lists {name}, but {PACK_WEIGHTS} holds no {name}.sign or {name}.full")
        return out

    def weight_map(self) -> Dict[str, str]:
        return {k: PACK_WEIGHTS for k in self.header}

    def check_against(self, base_uri: str, base_meta: Dict[str, Tuple[List[int], str]]):
        """pre-flight of every stored tensor against the base's shard headers: name -> (shape, dtype)"""
        for name, t in self.tensors.items():
            key = t.full_key or t.sign_key
            if name not in base_meta:
                self._fail(f"tensor {key}: the base {base_uri} has no tensor {name}")
            shape, dtype = base_meta[name]
            if [int(s) for s in shape] != t.shape or dtype != t.dtype:
                self._fail(f"tensor {key} stands for {name} {t.dtype} {t.shape}, the base {base_uri} holds it as {dtype} {list(shape)}")
