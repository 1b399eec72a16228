"""LoRA adapters as finetunes.

A ``finetune_merge`` entry ``{model: X, base: Y}`` whose ``storage_dir/X/`` holds ``adapter_config.json`` and
``adapter_model.safetensors`` and no ``model.safetensors.index.json`` is an adapter entry.  Its finetune tensor ``T``
is ``Y[T] + s * B @ A`` when the adapter has the pair ``base_model.model.<module>.lora_{A,B}.weight`` for
``T == "<module>.weight"``, rounded once into ``Y[T]``'s dtype (``Engine.lora_apply``), and ``Y[T]`` itself otherwise.
``s`` is ``lora_alpha / r`` (``lora_alpha / sqrt(r)`` with ``use_rslora``); ``rank_pattern`` / ``alpha_pattern``
keys match a module as PEFT matches them.  Everything this module rejects is rejected before any output is written.

DoRA (``use_dora``): every targeted Linear also has ``base_model.model.<module>.lora_magnitude_vector`` m [out], and
its finetune tensor is PEFT's merged weight ``V * (m / ||V||)[:, None]``, V = ``Y[T] + s * B @ A``, row norms over
``in``, rounded once.  A row with a zero or non-finite norm (or magnitude) fails the merge when that tensor is
reached, naming the row.  Embedding LoRA: ``base_model.model.<module>.lora_embedding_{A,B}`` (A [r, num_embeddings],
B [dim, r]) gives ``Y[T] + s * (B @ A).T``; DoRA on an embedding module is rejected.
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
_KEY = re.compile(r"^base_model\.model\.(?P<module>.+)\.(?:lora_(?P<ab>[AB])\.weight|lora_embedding_(?P<eab>[AB])"
                  r"|(?P<mag>lora_magnitude_vector))$")


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
    a_key: str                          # lora_A.weight, or lora_embedding_A for an embedding module
    b_key: str
    rank: int
    scale: float
    kind: str = "linear"                # "linear" | "embedding"
    m_key: Optional[str] = None         # DoRA: the module's lora_magnitude_vector


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

    def module_scale(self, module: str, rank: int, a_key: Optional[str] = None) -> float:
        c = self.config
        rank_pattern = c.get("rank_pattern") or {}
        alpha_pattern = c.get("alpha_pattern") or {}
        rk = pattern_key(rank_pattern, module)
        want = rank_pattern[rk] if rk is not None else c["r"]
        if rank != want:
            field = f"rank_pattern[{rk!r}]" if rk is not None else "r"
            self._fail(f"{a_key or KEY_PREFIX + module + '.lora_A.weight'} has rank {rank}, {field} says {want}")
        ak = pattern_key(alpha_pattern, module)
        alpha = float(alpha_pattern[ak] if ak is not None else c.get("lora_alpha", 8))
        return alpha / math.sqrt(rank) if c.get("use_rslora") else alpha / rank

    def _map_keys(self) -> Dict[str, LoraPair]:
        found: Dict[str, Dict[str, str]] = {}
        for key in self.header:
            m = _KEY.match(key)
            if m is None:
                self._fail(f"tensor {key} is not a lora_A / lora_B weight, a lora_embedding_A / lora_embedding_B factor "
                           "or a DoRA lora_magnitude_vector (biases and full tensors are not supported)")
            role = m.group("ab") or ("E" + m.group("eab") if m.group("eab") else "M")
            found.setdefault(m.group("module"), {})[role] = key
        dora = bool(self.config.get("use_dora"))
        pairs = {}
        for module, keys in found.items():
            linear, emb = {"A", "B"} & set(keys), {"EA", "EB"} & set(keys)
            if "M" in keys and not dora:
                self._fail(f"tensor {keys['M']}: a DoRA lora_magnitude_vector, but use_dora is not set")
            if linear and emb:
                self._fail(f"tensors {keys[min(linear)]} and {keys[min(emb)]}: a module has either lora_A / lora_B or "
                           "lora_embedding_A / lora_embedding_B factors")
            if emb:
                if "M" in keys:
                    self._fail(f"tensor {keys['M']}: DoRA on the embedding module {module} is not supported")
                pairs[f"{module}.weight"] = self._pair(module, keys, "EA", "EB", "embedding")
            elif linear:
                if dora and "M" not in keys:
                    self._fail(f"use_dora is set but tensor {keys[min(linear)]} has no {KEY_PREFIX}{module}."
                               "lora_magnitude_vector")
                pairs[f"{module}.weight"] = self._pair(module, keys, "A", "B", "linear")
            else:
                self._fail(f"tensor {keys['M']} has no lora_A / lora_B factors")
        return pairs

    def _pair(self, module: str, keys: Dict[str, str], ra: str, rb: str, kind: str) -> LoraPair:
        """the factors of one module: linear lora_A [r, in] / lora_B [out, r]; embedding lora_embedding_A
        [r, num_embeddings] / lora_embedding_B [dim, r]; and a DoRA magnitude [out]"""
        if set(keys) & {ra, rb} != {ra, rb}:
            have = ra if ra in keys else rb
            partner = {"A": "lora_B", "B": "lora_A", "EA": "lora_embedding_B", "EB": "lora_embedding_A"}[have]
            self._fail(f"tensor {keys[have]} has no {partner} partner")
        ka, kb = keys[ra], keys[rb]
        a, b = self.header[ka], self.header[kb]
        for key, rec in ((ka, a), (kb, b)):
            if len(rec["shape"]) != 2:
                self._fail(f"tensor {key} has shape {rec['shape']}, a 2-D factor expected")
            if rec["dtype"] not in _FACTOR_DTYPES:
                self._fail(f"tensor {key} is {rec['dtype']} (BF16, F16 or F32 factors only)")
        rank = int(a["shape"][0])
        if int(b["shape"][1]) != rank:
            self._fail(f"tensor {kb} has shape {b['shape']}, its {'lora_embedding_A' if kind == 'embedding' else 'lora_A'} "
                       f"{a['shape']}: the ranks differ")
        if not 1 <= rank <= MAX_RANK:
            self._fail(f"tensor {ka} has rank {rank} (1..{MAX_RANK} supported)")
        km = keys.get("M")
        if km is not None:
            mrec = self.header[km]
            if len(mrec["shape"]) != 1 or int(mrec["shape"][0]) != int(b["shape"][0]):
                self._fail(f"tensor {km} has shape {mrec['shape']}, [{int(b['shape'][0])}] (the rows of {kb}) expected")
            if mrec["dtype"] not in _FACTOR_DTYPES:
                self._fail(f"tensor {km} is {mrec['dtype']} (BF16, F16 or F32 magnitudes only)")
        return LoraPair(ka, kb, rank, self.module_scale(module, rank, ka), kind, km)

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
            # linear: lora_A [r, in], lora_B [out, r]; embedding: lora_embedding_A [r, num_embeddings = out],
            # lora_embedding_B [dim = in, r]
            fits = (int(a[1]) == out_f and int(b[0]) == in_f) if pair.kind == "embedding" else \
                (int(a[1]) == in_f and int(b[0]) == out_f)
            if not fits:
                self._fail(f"tensors {pair.a_key} {a} / {pair.b_key} {b} do not fit the base tensor {name} {list(shape)}")
            if pair.m_key is not None and list(self.header[pair.m_key]["shape"]) != [out_f]:
                self._fail(f"tensor {pair.m_key} {self.header[pair.m_key]['shape']} does not fit the base tensor {name} "
                           f"{list(shape)}: [{out_f}] expected")
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
