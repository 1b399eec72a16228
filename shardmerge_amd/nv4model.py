"""NVFP4 checkpoints as finetunes: a full model whose 2-D weights are stored as E2M1 codes, two to a byte, with one E4M3
scale per block of 16 consecutive elements of a row and one fp32 scale per tensor - the form ModelOpt writes (as
recalled: PAPERS.md).

A model directory is an NVFP4 checkpoint when BOTH hold: the ``quantization_config`` of its ``config.json``, or an
``hf_quant_config.json``, says ``quant_algo: "NVFP4"``, and a shard header holds a triple - a ``U8`` tensor ``X.weight``
of shape ``[R, C / 2]``, an ``F8_E4M3`` tensor ``X.weight_scale`` of shape ``[R, C / 16]`` and an ``F32`` tensor
``X.weight_scale_2`` of shape ``[]`` or ``[1]``.  The test runs BEFORE the FP8 one (fp8model.py), which would claim the
directory for its ``F8_E4M3`` scale tensors; a directory it does not claim is left to the FP8 test as before.  A
``group_size``, where one is named, must be 16; every 2-D ``U8`` ``*.weight`` must come with both scales; an ``F8_E4M3``
tensor that is no block scale (FP8 weights mixed in) and a ``U8`` scale (MXFP4 weights mixed in) are rejected; any
``X.input_scale`` is ignored.  As a ``finetune_merge`` entry its tensor ``X.weight`` is ``Engine.nv4_dequant(X.weight,
X.weight_scale, X.weight_scale_2, dtype of the base's X.weight)`` (the function is stated in include/shardmerge_hip.h,
smhip_nv4_dequant); the tensors it keeps in 16 or 32 bits pass as they are.  ``python -m shard quantize-nvfp4`` writes
one and ``dequantize-nvfp4`` turns one back (merge/nv4.py).  Everything this module rejects is rejected before any
output is written, and the message names the model and the tensor or field.
"""
from __future__ import annotations

import hashlib
import json
from pathlib import Path
from typing import Dict, Optional

from .adapter import FULL_INDEX, read_header

CODE_DTYPE = "U8"
SCALE_DTYPE = "F8_E4M3"
SCALE_SUFFIX = "_scale"
GLOBAL_SUFFIX = "_scale_2"
INPUT_SUFFIX = ".input_scale"
BLOCK = 16
QUANT_METHOD = "modelopt"
QUANT_ALGO = "NVFP4"
HF_QUANT_CONFIG = "hf_quant_config.json"


class Nv4ModelError(ValueError):
    """an NVFP4 checkpoint this build cannot read; the message names the model and the tensor or field"""


def quantization_config(not_converted) -> Dict:
    """the ``quantization_config`` block of a checkpoint `quantize-nvfp4` writes"""
    return {"quant_method": QUANT_METHOD, "quant_algo": QUANT_ALGO, "group_size": BLOCK, "ignore": sorted(not_converted)}


def scale_shape(code_shape):
    """the shape of the block scales of codes [R, C / 2]: [R, C / 16]"""
    return [int(code_shape[0]), 2 * int(code_shape[1]) // BLOCK]


def _read_json(path: Path):
    try:
        doc = json.loads(path.read_bytes())
    except (OSError, ValueError):
        return None
    return doc if isinstance(doc, dict) else None


def quant_fields(path: Path) -> Dict[str, Dict]:
    """the blocks that can name the algorithm, by the field path a message names them with"""
    path = Path(path)
    found = {}
    qc = (_read_json(path / "config.json") or {}).get("quantization_config")
    if isinstance(qc, dict):
        found["config.json quantization_config"] = qc
    hq = _read_json(path / HF_QUANT_CONFIG)
    if hq is not None:
        inner = hq.get("quantization")
        found[f"{HF_QUANT_CONFIG} quantization"] = inner if isinstance(inner, dict) else hq
    return found


def says_nvfp4(path: Path) -> bool:
    return any(block.get("quant_algo") == QUANT_ALGO for block in quant_fields(path).values())


def _is_triple(header: Dict, name: str) -> bool:
    rec, sc, g = header[name], header.get(name + SCALE_SUFFIX), header.get(name + GLOBAL_SUFFIX)
    return (rec["dtype"] == CODE_DTYPE and name.endswith(".weight") and len(rec["shape"]) == 2 and sc is not None
            and sc["dtype"] == SCALE_DTYPE and g is not None and g["dtype"] == "F32")


class Nv4Model:
    """the NVFP4 tensors of the full model at `path` and their scales; `scale_keys`: tensor name -> its block scales'
    key, `global_keys`: tensor name -> its tensor scale's key"""

    def __init__(self, uri: str, path: Path, weight_map: Dict[str, str]):
        self.uri = uri
        self.path = Path(path)
        self.scale_keys: Dict[str, str] = {}
        self.global_keys: Dict[str, str] = {}
        sha = hashlib.sha256()
        header = {}
        for shard in sorted(set(weight_map.values())):
            raw, doc = read_header(self.path / shard)
            sha.update(shard.encode() + b"\0" + raw)
            header.update(doc)
        header.pop("__metadata__", None)
        self.header = header
        self.identity = {"nv4_headers": sha.hexdigest()}       # offsets, shapes and metadata of every shard
        self.claimed = says_nvfp4(self.path) and any(_is_triple(header, n) for n in header)
        if not self.claimed:
            return
        for field, block in quant_fields(self.path).items():
            if block.get("quant_algo", QUANT_ALGO) != QUANT_ALGO:
                self._fail(f"{field}.quant_algo {block.get('quant_algo')!r} is not {QUANT_ALGO!r}")
            if block.get("group_size", BLOCK) != BLOCK:
                self._fail(f"{field}.group_size {block.get('group_size')!r} is not {BLOCK}")
        for name, rec in header.items():
            if rec["dtype"] != CODE_DTYPE or not name.endswith(".weight"):
                continue
            if len(rec["shape"]) != 2 or (2 * rec["shape"][1]) % BLOCK:
                self._fail(f"tensor {name} is {CODE_DTYPE} {rec['shape']}; NVFP4 codes are [R, C / 2] with C a multiple of {BLOCK}")
            key, gkey = name + SCALE_SUFFIX, name + GLOBAL_SUFFIX
            sc, g = header.get(key), header.get(gkey)
            if sc is None or g is None:
                self._fail(f"tensor {name} is {CODE_DTYPE} but the checkpoint has no {key if sc is None else gkey}")
            if sc["dtype"] != SCALE_DTYPE or list(sc["shape"]) != scale_shape(rec["shape"]):
                mix = " (MXFP4 and NVFP4 weights are mixed)" if sc["dtype"] == CODE_DTYPE else ""
                self._fail(f"tensor {key} is {sc['dtype']} {sc['shape']}, {SCALE_DTYPE} {scale_shape(rec['shape'])} expected for "
                           f"the codes {name} {rec['shape']} in blocks of {BLOCK}{mix}")
            if g["dtype"] != "F32" or list(g["shape"]) not in ([], [1]):
                self._fail(f"tensor {gkey} is {g['dtype']} {g['shape']}, one F32 value expected")
            self.scale_keys[name] = key
            self.global_keys[name] = gkey
        scales = set(self.scale_keys.values())
        for name, rec in header.items():
            if rec["dtype"] == SCALE_DTYPE and name not in scales:
                self._fail(f"tensor {name} is {SCALE_DTYPE} but no block scale of an NVFP4 weight (FP8 and NVFP4 weights are mixed)")
        self.ignored = {n for n in header if n.endswith(INPUT_SUFFIX)}

    def _fail(self, what: str):
        raise Nv4ModelError(f"NVFP4 checkpoint {self.uri}: {what}")

    @property
    def scale_names(self):
        """every tensor that belongs to a weight and is no tensor of the model: both scales, and the ignored input scales"""
        return set(self.scale_keys.values()) | set(self.global_keys.values()) | self.ignored

    def shape(self, name: str):
        """the shape [R, C] of the tensor the codes `name` stand for"""
        r, half = self.header[name]["shape"]
        return [int(r), 2 * int(half)]


def nv4_model(uri: str, path: Path, weight_map: Dict[str, str]) -> Optional[Nv4Model]:
    """the Nv4Model of a full model directory; None unless a config says NVFP4 and a shard holds a triple"""
    if not says_nvfp4(path):
        return None
    m = Nv4Model(uri, path, weight_map)
    return m if m.claimed else None


def nv4_identity(path: Path) -> Optional[Dict[str, str]]:
    """what decides an NVFP4 checkpoint's content for a resumed run: its shard headers; None for anything else"""
    path = Path(path)
    if not (path / FULL_INDEX).exists():
        return None
    try:
        weight_map = json.loads((path / FULL_INDEX).read_bytes())["weight_map"]
        m = nv4_model(str(path), path, weight_map)
    except (OSError, ValueError, KeyError):
        return None
    return m.identity if m is not None else None
