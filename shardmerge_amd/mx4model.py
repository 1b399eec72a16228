"""MXFP4 checkpoints as finetunes: a full model whose 2-D weights are stored as E2M1 codes, two to a byte, with one E8M0
power-of-two scale per block of 32 consecutive elements of a row - the OCP micro-scaling form (as recalled: PAPERS.md).

A model directory is an MXFP4 checkpoint when BOTH hold: its ``config.json`` has ``quantization_config.quant_method ==
"mxfp4"``, and a shard header holds a ``U8`` tensor ``X.weight`` of shape ``[R, C / 2]`` with a ``U8`` tensor
``X.weight_scale`` of shape ``[R, C / 32]``.  ``U8`` alone decides nothing.  The block must say ``weight_block_size:
[1, 32]`` and, when it names one, ``scale_format: "e8m0"``; every 2-D ``U8`` ``*.weight`` must come with its scale.  As a
``finetune_merge`` entry its tensor ``X.weight`` is ``Engine.mx4_dequant(X.weight, X.weight_scale, dtype of the base's
X.weight)`` (the function is stated in include/shardmerge_hip.h, smhip_mx4_dequant); the tensors it keeps in 16 or 32
bits pass as they are.  ``python -m shard quantize-mxfp4`` writes one and ``dequantize-mxfp4`` turns one back
(merge/mx4.py).  Everything this module rejects is rejected before any output is written, and the message names the
model and the tensor or field.
"""
from __future__ import annotations

import hashlib
import json
from pathlib import Path
from typing import Dict, Optional

from .adapter import FULL_INDEX, read_header

CODE_DTYPE = "U8"
SCALE_SUFFIX = "_scale"
BLOCK = 32
QUANT_METHOD = "mxfp4"
SCALE_FORMAT = "e8m0"


class Mx4ModelError(ValueError):
    """an MXFP4 checkpoint this build cannot read; the message names the model and the tensor or field"""


def quantization_config(not_converted) -> Dict:
    """the ``quantization_config`` block of a checkpoint `quantize-mxfp4` writes"""
    return {"quant_method": QUANT_METHOD, "weight_block_size": [1, BLOCK], "scale_format": SCALE_FORMAT,
            "modules_to_not_convert": sorted(not_converted)}


def scale_shape(code_shape):
    """the shape of the scales of codes [R, C / 2]: [R, C / 32]"""
    return [int(code_shape[0]), 2 * int(code_shape[1]) // BLOCK]


def quant_method(path: Path) -> Optional[str]:
    """``quantization_config.quant_method`` of the model directory's config.json, None where there is none"""
    try:
        qc = json.loads((Path(path) / "config.json").read_bytes()).get("quantization_config")
    except (OSError, ValueError, AttributeError):
        return None
    return qc.get("quant_method") if isinstance(qc, dict) else None


class Mx4Model:
    """the MXFP4 tensors of the full model at `path` and their scales; `scale_keys`: tensor name -> its scale's key"""

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
        self.identity = {"mx4_headers": sha.hexdigest()}       # offsets, shapes and metadata of every shard
        qc = json.loads((self.path / "config.json").read_bytes())["quantization_config"]
        if list(qc.get("weight_block_size") or []) != [1, BLOCK]:
            self._fail(f"quantization_config.weight_block_size {qc.get('weight_block_size')!r} is not [1, {BLOCK}]")
        if qc.get("scale_format", SCALE_FORMAT) != SCALE_FORMAT:
            self._fail(f"quantization_config.scale_format {qc.get('scale_format')!r} is not {SCALE_FORMAT!r}")
        for name, rec in header.items():
            if rec["dtype"] != CODE_DTYPE or not name.endswith(".weight"):
                continue
            key = name + SCALE_SUFFIX
            if len(rec["shape"]) != 2 or (2 * rec["shape"][1]) % BLOCK:
                self._fail(f"tensor {name} is {CODE_DTYPE} {rec['shape']}; MXFP4 codes are [R, C / 2] with C a multiple of {BLOCK}")
            sc = header.get(key)
            if sc is None:
                self._fail(f"tensor {name} is {CODE_DTYPE} but the checkpoint has no {key}")
            if sc["dtype"] != CODE_DTYPE or list(sc["shape"]) != scale_shape(rec["shape"]):
                self._fail(f"tensor {key} is {sc['dtype']} {sc['shape']}, {CODE_DTYPE} {scale_shape(rec['shape'])} expected for "
                           f"the codes {name} {rec['shape']} in blocks of {BLOCK}")
            self.scale_keys[name] = key

    def _fail(self, what: str):
        raise Mx4ModelError(f"MXFP4 checkpoint {self.uri}: {what}")

    @property
    def scale_names(self):
        return set(self.scale_keys.values())

    def shape(self, name: str):
        """the shape [R, C] of the tensor the codes `name` stand for"""
        r, half = self.header[name]["shape"]
        return [int(r), 2 * int(half)]


def mx4_model(uri: str, path: Path, weight_map: Dict[str, str]) -> Optional[Mx4Model]:
    """the Mx4Model of a full model directory; None unless its config.json says mxfp4 and a shard holds a coded weight"""
    if quant_method(path) != QUANT_METHOD:
        return None
    m = Mx4Model(uri, path, weight_map)
    return m if m.scale_keys else None


def mx4_identity(path: Path) -> Optional[Dict[str, str]]:
    """what decides an MXFP4 checkpoint's content for a resumed run: its shard headers; None for anything else"""
    path = Path(path)
    if not (path / FULL_INDEX).exists():
        return None
    try:
        weight_map = json.loads((path / FULL_INDEX).read_bytes())["weight_map"]
        m = mx4_model(str(path), path, weight_map)
    except (OSError, ValueError, KeyError):
        return None
    return m.identity if m is not None else None
