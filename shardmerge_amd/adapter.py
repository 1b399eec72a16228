"""LoRA adapters as finetunes.

A ``finetune_merge`` entry ``{model: X, base: Y}`` whose ``storage_dir/X/`` holds ``adapter_config.json`` and
``adapter_model.safetensors`` and no ``model.safetensors.index.json`` is an adapter entry.  Its finetune tensor ``T``
is ``Y[T] + s * B @ A`` when the adapter has the pair ``base_model.model.<module>.lora_{A,B}.weight`` for
``T == "<module>.weight"``, rounded once into ``Y[T]``'s dtype (``Engine.lora_apply``), and ``Y[T]`` itself otherwise.
``s`` is ``lora_alpha / r`` (``lora_alpha / sqrt(r)`` with ``use_rslora``); ``rank_pattern`` / ``alpha_pattern``
keys match a module as PEFT matches them.  Everything this module rejects is rejected before any output is written.
"""
from __future__ import annotations

import hashlib
import json
import math
import re
from dataclasses import dataclass
from pathlib import Path
from typing import Dict, List, Optional, Tuple

ADAPTER_CONFIG = "adapter_config.json"
ADAPTER_WEIGHTS = "adapter_model.safetensors"
ADAPTER_BIN = "adapter_model.bin"
FULL_INDEX = "model.safetensors.index.json"
KEY_PREFIX = "base_model.model."
MAX_RANK = 512                          # smhip_lora_apply
_FACTOR_DTYPES = ("BF16", "F16", "F32")
_KEY = re.compile(r"^base_model\.model\.(?P<module>.+)\.lora_(?P<ab>[AB])\.weight$")


class AdapterError(ValueError):
    """an adapter this build cannot apply; the message names the adapter and the field or tensor key"""


def is_adapter_dir(path: Path) -> bool:
    path = Path(path)
    return (path / ADAPTER_CONFIG).exists() and (path / ADAPTER_WEIGHTS).exists() and not (path / FULL_INDEX).exists()


def is_bin_only_adapter_dir(path: Path) -> bool:
    path = Path(path)
    return ((path / ADAPTER_CONFIG).exists() and (path / ADAPTER_BIN).exists() and not (path / ADAPTER_WEIGHTS).exists()
            and not (path / FULL_INDEX).exists())


def read_header(path: Path) -> Tuple[bytes, Dict]:
    """(raw header bytes, parsed header without __metadata__) of a safetensors file"""
    with open(path, "rb") as fh:
        n = int.from_bytes(fh.read(8), "little")
        raw = fh.read(n)
    doc = json.loads(raw)
    doc.pop("__metadata__", None)
    return raw, doc


def pattern_key(patterns: Dict, module: str) -> Optional[str]:
    """the first key (file order) that names `module` as PEFT matches it: the key, read as a regex, equals the module
    name or a dotted suffix of it"""
    for key in patterns:
        if re.fullmatch(rf"(.*\.)?(?:{key})", module):
            return key
    return None


@dataclass
class LoraPair:
    a_key: str
    b_key: str
    rank: int
    scale: float


class LoraAdapter:
    def __init__(self, uri: str, path: Path):
        self.uri = uri
        self.path = Path(path)
        cfg_bytes = (self.path / ADAPTER_CONFIG).read_bytes()
        self.config = json.loads(cfg_bytes)
        self._validate_config()
        header_bytes, self.header = read_header(self.path / ADAPTER_WEIGHTS)
        self.identity = {"adapter_config": hashlib.sha256(cfg_bytes).hexdigest(),
                         "adapter_header": hashlib.sha256(header_bytes).hexdigest()}
        self.pairs: Dict[str, LoraPair] = self._map_keys()       # base tensor name -> its factors

    def _fail(self, what: str):
        raise AdapterError(f"LoRA adapter {self.uri}: {what}")

    def _validate_config(self):
        c = self.config
        if c.get("peft_type") != "LORA":
            self._fail(f"peft_type {c.get('peft_type')!r} is not supported (only LORA)")
        if c.get("use_dora"):
            self._fail("use_dora (DoRA) is not supported")
        if c.get("fan_in_fan_out"):
            self._fail("fan_in_fan_out is not supported")
        if (c.get("bias") or "none") != "none":
            self._fail(f"bias {c.get('bias')!r} is not supported (only 'none')")
        if c.get("modules_to_save"):
            self._fail(f"modules_to_save {c.get('modules_to_save')!r} is not supported")
        if c.get("layer_replication"):
            self._fail("layer_replication is not supported")
        if not isinstance(c.get("r"), int) or c["r"] < 1:
            self._fail(f"r {c.get('r')!r} is not a positive integer")
        if not isinstance(c.get("lora_alpha", 8), (int, float)):
            self._fail(f"lora_alpha {c.get('lora_alpha')!r} is not a number")

    def module_scale(self, module: str, rank: int) -> float:
        c = self.config
        rank_pattern = c.get("rank_pattern") or {}
        alpha_pattern = c.get("alpha_pattern") or {}
        rk = pattern_key(rank_pattern, module)
        want = rank_pattern[rk] if rk is not None else c["r"]
        if rank != want:
            field = f"rank_pattern[{rk!r}]" if rk is not None else "r"
            self._fail(f"{KEY_PREFIX}{module}.lora_A.weight has rank {rank}, {field} says {want}")
        ak = pattern_key(alpha_pattern, module)
        alpha = float(alpha_pattern[ak] if ak is not None else c.get("lora_alpha", 8))
        return alpha / math.sqrt(rank) if c.get("use_rslora") else alpha / rank

    def _map_keys(self) -> Dict[str, LoraPair]:
        found: Dict[str, Dict[str, str]] = {}
        for key in self.header:
            m = _KEY.match(key)
            if m is None:
                self._fail(f"tensor {key} is not a lora_A / lora_B weight (embedding LoRA, DoRA magnitudes, biases and "
                           "full tensors are not supported)")
            found.setdefault(m.group("module"), {})[m.group("ab")] = key
        pairs = {}
        for module, ab in found.items():
            if set(ab) != {"A", "B"}:
                self._fail(f"tensor {next(iter(ab.values()))} has no lora_{'B' if 'A' in ab else 'A'} partner")
            a, b = self.header[ab["A"]], self.header[ab["B"]]
            for key, rec in ((ab["A"], a), (ab["B"], b)):
                if len(rec["shape"]) != 2:
                    self._fail(f"tensor {key} has shape {rec['shape']}, a 2-D factor expected")
                if rec["dtype"] not in _FACTOR_DTYPES:
                    self._fail(f"tensor {key} is {rec['dtype']} (BF16, F16 or F32 factors only)")
            rank = int(a["shape"][0])
            if int(b["shape"][1]) != rank:
                self._fail(f"tensor {ab['B']} has shape {b['shape']}, its lora_A {a['shape']}: the ranks differ")
            if not 1 <= rank <= MAX_RANK:
                self._fail(f"tensor {ab['A']} has rank {rank} (1..{MAX_RANK} supported)")
            pairs[f"{module}.weight"] = LoraPair(ab["A"], ab["B"], rank, self.module_scale(module, rank))
        return pairs

    def weight_map(self) -> Dict[str, str]:
        return {k: ADAPTER_WEIGHTS for k in self.header}

    def check_against(self, base_uri: str, base_meta: Dict[str, Tuple[List[int], str]]):
        """pre-flight of every pair against the base's shard headers: name -> (shape, dtype)"""
        for name, pair in self.pairs.items():
            if name not in base_meta:
                self._fail(f"tensor {pair.a_key}: the base {base_uri} has no tensor {name}")
            shape, dtype = base_meta[name]
            if len(shape) != 2:
                self._fail(f"tensor {pair.a_key}: the base tensor {name} has shape {list(shape)}, 2-D expected")
            if dtype not in _FACTOR_DTYPES:
                self._fail(f"tensor {pair.a_key}: the base tensor {name} is {dtype} (BF16, F16 or F32 supported)")
            out_f, in_f = int(shape[0]), int(shape[1])
            a, b = self.header[pair.a_key]["shape"], self.header[pair.b_key]["shape"]
            if int(a[1]) != in_f or int(b[0]) != out_f:
                self._fail(f"tensors {pair.a_key} {a} / {pair.b_key} {b} do not fit the base tensor {name} {list(shape)}")
            if self.header[pair.a_key]["dtype"] != self.header[pair.b_key]["dtype"]:
                self._fail(f"tensors {pair.a_key} and {pair.b_key} have different dtypes")


def base_tensor_meta(index, uri: str) -> Dict[str, Tuple[List[int], str]]:
    """name -> (shape, dtype) of every tensor of a full model, from its shard headers (no payload read)"""
    weight_map = index.model_indexes[uri]["weight_map"]
    out = {}
    for shard in sorted(set(weight_map.values())):
        _, header = read_header(index.storage_path / uri / shard)
        for name, rec in header.items():
            out[name] = (rec["shape"], rec["dtype"])
    return out
