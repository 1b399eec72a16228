"""Block-scaled FP8 checkpoints as finetunes: a full model whose 2-D weights are stored as OCP E4M3 codes with one fp32
scale per 128 x 128 block - the Hugging Face ``quant_method: "fp8"`` layout (as recalled: PAPERS.md).

A model directory is an FP8 checkpoint when a shard header holds an ``F8_E4M3`` tensor.  Every such tensor ``X`` must
come with an ``F32`` tensor ``X_scale_inv`` of shape ``[ceil(R / 128), ceil(C / 128)]``; ``config.json``, when it has a
``quantization_config``, must say ``quant_method: "fp8"``, ``fmt: "e4m3"`` and ``weight_block_size: [128, 128]``.  As a
``finetune_merge`` entry its tensor ``X`` is ``Engine.fp8_dequant(X, X_scale_inv, dtype of the base's X)`` (the function
is stated in include/shardmerge_hip.h, smhip_fp8_dequant); the tensors it keeps in 16 or 32 bits pass as they are.
``python -m shard quantize-fp8`` writes one and ``dequantize-fp8`` turns one back (merge/fp8.py).  Everything this
module rejects is rejected before any output is written, and the message names the model and the tensor or field.
"""
from __future__ import annotations

import hashlib
import json
from pathlib import Path
from typing import Dict, Optional

from .adapter import FULL_INDEX, read_header

FP8_DTYPE = "F8_E4M3"
SCALE_SUFFIX = "_scale_inv"
BLOCK = 128
QUANT_METHOD = "fp8"
FMT = "e4m3"


class Fp8ModelError(ValueError):
    """an FP8 checkpoint this build cannot read; the message names the model and the tensor or field"""


def quantization_config(not_converted) -> Dict:
    """the ``quantization_config`` block of a checkpoint `quantize-fp8` writes"""
    return {"quant_method": QUANT_METHOD, "fmt": FMT, "activation_scheme": "dynamic", "weight_block_size": [BLOCK, BLOCK],
            "modules_to_not_convert": sorted(not_converted)}


def scale_shape(shape):
    return [-(-int(shape[0]) // BLOCK), -(-int(shape[1]) // BLOCK)]


class Fp8Model:
    """the FP8 tensors of the full model at `path` and their scales; `scale_keys`: tensor name -> its scale's key"""

    def __init__(self, uri: str, path: Path, weight_map: Dict[str, str]):
        self.uri = uri
        self.path = Path(path)
        self.scale_keys: Dict[str, str] = {}
        sha = hashlib.sha256()
        header = {}
        for shard in sorted(set(weight_map.values())):
            raw, doc = read_header(self.path / shard)
            sha.update(shard.encode() + b"\0" + raw)
            header.update(doc)
        self.header = header
        self.identity = {"fp8_headers": sha.hexdigest()}       # offsets, shapes and metadata of every shard
        for name, rec in header.items():
            if rec["dtype"] != FP8_DTYPE:
                continue
            key = name + SCALE_SUFFIX
            if len(rec["shape"]) != 2:
                self._fail(f"tensor {name} is {FP8_DTYPE} {rec['shape']}; only 2-D tensors are block-scaled")
            sc = header.get(key)
            if sc is None:
                self._fail(f"tensor {name} is {FP8_DTYPE} but the checkpoint has no {key}")
            if sc["dtype"] != "F32" or list(sc["shape"]) != scale_shape(rec["shape"]):
                self._fail(f"tensor {key} is {sc['dtype']} {sc['shape']}, F32 {scale_shape(rec['shape'])} expected for "
                           f"{name} {rec['shape']} in blocks of {BLOCK} x {BLOCK}")
            self.scale_keys[name] = key
        if self.scale_keys:
            self._validate_config()

    def _fail(self, what: str):
        raise Fp8ModelError(f"FP8 checkpoint {self.uri}: {what}")

    def _validate_config(self):
        cfg_path = self.path / "config.json"
        if not cfg_path.exists():
            return
        try:
            qc = json.loads(cfg_path.read_bytes()).get("quantization_config")
        except ValueError as exc:
            self._fail(f"config.json is not JSON ({exc})")
        if qc is None:
            return
        if qc.get("quant_method") != QUANT_METHOD:
            self._fail(f"quantization_config.quant_method {qc.get('quant_method')!r} is not {QUANT_METHOD!r}")
        if qc.get("fmt", FMT) != FMT:
            self._fail(f"quantization_config.fmt {qc.get('fmt')!r} is not {FMT!r}")
        if list(qc.get("weight_block_size") or []) != [BLOCK, BLOCK]:
            self._fail(f"quantization_config.weight_block_size {qc.get('weight_block_size')!r} is not [{BLOCK}, {BLOCK}]")

    @property
    def scale_names(self):
        return set(self.scale_keys.values())


def fp8_model(uri: str, path: Path, weight_map: Dict[str, str]) -> Optional[Fp8Model]:
    """the Fp8Model of a full model directory, None when no shard holds an F8_E4M3 tensor - or when the directory is an
    NVFP4 checkpoint (nv4model.py), whose block scales are F8_E4M3 tensors"""
    from .nv4model import nv4_model
    if nv4_model(uri, path, weight_map) is not None:
        return None
    m = Fp8Model(uri, path, weight_map)
    return m if m.scale_keys else None


def fp8_identity(path: Path) -> Optional[Dict[str, str]]:
    """what decides an FP8 checkpoint's content for a resumed run: its shard headers; None for anything else"""
    path = Path(path)
    if not (path / FULL_INDEX).exists():
        return None
    try:
        weight_map = json.loads((path / FULL_INDEX).read_bytes())["weight_map"]
        m = fp8_model(str(path), path, weight_map)
    except (OSError, ValueError, KeyError):
        return None
    return m.identity if m is not None else None
