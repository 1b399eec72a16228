"""GPTQ-layout INT4 checkpoints as finetunes: a full model whose Linear weights ``W [R = out, C = in]`` are stored as
group-quantised 4-bit integers in the tensor layout GPTQ checkpoints ship in (as recalled: PAPERS.md) - ``X.qweight``
(``I32`` ``[C / 8, R]``, eight codes of consecutive input columns to a word), ``X.qzeros`` (``I32`` ``[C / g, R / 8]``,
eight zero-points of consecutive output rows to a word, stored minus one), ``X.scales`` (``F16`` ``[C / g, R]``) and
``X.g_idx`` (``I32`` ``[C]``).  There is no ``X.weight``; ``X.bias`` and every other tensor are plain.

A model directory is a GPTQ checkpoint when BOTH hold: the ``quantization_config`` of its ``config.json`` says
``quant_method: "gptq"``, and a shard header holds an ``I32`` tensor ``X.qweight`` together with ``X.qzeros``,
``X.scales`` and ``X.g_idx``.  A directory that is claimed must then be one this build reads: ``bits`` 4, ``desc_act``
false, a ``checkpoint_format`` - where one is named - of ``gptq``, a ``group_size`` of 32, 64 or 128, and every
``X.qweight`` with its three companions in the dtypes and shapes above.  As a ``finetune_merge`` entry its tensor
``X.weight`` is ``Engine.gptq_dequant(X.qweight, X.qzeros, X.scales, X.g_idx, dtype of the base's X.weight)`` (the
function is stated in include/shardmerge_hip.h, smhip_gptq_dequant).  ``python -m shard quantize-gptq`` writes one - by
round to nearest, not by the GPTQ solver - and ``dequantize-gptq`` turns one back (merge/gptq.py).  Everything this
module rejects is rejected before any output is written, and the message names the model and the tensor or field.
"""
from __future__ import annotations

import hashlib
import json
from pathlib import Path
from typing import Dict, Optional, Tuple

from .adapter import FULL_INDEX, read_header

QUANT_METHOD = "gptq"
GROUPS = (32, 64, 128)
WEIGHT_SUFFIX = ".weight"
QWEIGHT, QZEROS, SCALES, G_IDX = ".qweight", ".qzeros", ".scales", ".g_idx"
COMPANIONS = (QZEROS, SCALES, G_IDX)


class GptqModelError(ValueError):
    """a GPTQ checkpoint this build cannot read; the message names the model and the tensor or field"""


def quantization_config(not_converted, group_size: int = 128) -> Dict:
    """the ``quantization_config`` block of a checkpoint `quantize-gptq` writes"""
    return {"quant_method": QUANT_METHOD, "bits": 4, "group_size": group_size, "desc_act": False, "sym": False,
            "checkpoint_format": "gptq", "modules_to_not_convert": sorted(not_converted)}


def quant_block(path: Path) -> Optional[Dict]:
    try:
        doc = json.loads((Path(path) / "config.json").read_bytes())
    except (OSError, ValueError):
        return None
    qc = doc.get("quantization_config") if isinstance(doc, dict) else None
    return qc if isinstance(qc, dict) else None


def says_gptq(path: Path) -> bool:
    qc = quant_block(path)
    return qc is not None and qc.get("quant_method") == QUANT_METHOD


def _is_quad(header: Dict, name: str) -> bool:
    return (name.endswith(QWEIGHT) and header[name]["dtype"] == "I32"
            and all(name[: -len(QWEIGHT)] + c in header for c in COMPANIONS))


class GptqModel:
    """the GPTQ tensors of the full model at `path`; `keys`: the name ``X.weight`` of the tensor they stand for -> the
    names of (qweight, qzeros, scales, g_idx)"""

    def __init__(self, uri: str, path: Path, weight_map: Dict[str, str]):
        self.uri = uri
        self.path = Path(path)
        self.keys: Dict[str, Tuple[str, str, str, str]] = {}
        self.group_size = 0
        sha = hashlib.sha256()
        header = {}
        for shard in sorted(set(weight_map.values())):
            raw, doc = read_header(self.path / shard)
            sha.update(shard.encode() + b"\0" + raw)
            header.update(doc)
        header.pop("__metadata__", None)
        self.header = header
        self.identity = {"gptq_headers": sha.hexdigest()}      # offsets, shapes and metadata of every shard
        self.claimed = says_gptq(self.path) and any(_is_quad(header, n) for n in header)
        if not self.claimed:
            return
        qc = quant_block(self.path)
        field = "config.json quantization_config"
        if qc.get("bits") != 4:
            self._fail(f"{field}.bits {qc.get('bits')!r} is not 4")
        if qc.get("desc_act", False):
            self._fail(f"{field}.desc_act is true: act-order is not supported")
        if qc.get("checkpoint_format", "gptq") != "gptq":
            self._fail(f"{field}.checkpoint_format {qc.get('checkpoint_format')!r} is not 'gptq'")
        g = qc.get("group_size")
        if g not in GROUPS:
            self._fail(f"{field}.group_size {g!r} is not one of {list(GROUPS)}")
        self.group_size = g
        for name, rec in header.items():
            if not name.endswith(QWEIGHT):
                continue
            stem = name[: -len(QWEIGHT)]
            if rec["dtype"] != "I32" or len(rec["shape"]) != 2 or rec["shape"][1] % 8 or (8 * rec["shape"][0]) % g:
                self._fail(f"tensor {name} is {rec['dtype']} {rec['shape']}; I32 [C / 8, R] with R a multiple of 8 and C a "
                           f"multiple of the group size {g} expected")
            cols, rows = 8 * rec["shape"][0], rec["shape"][1]
            want = {QZEROS: ("I32", [cols // g, rows // 8]), SCALES: ("F16", [cols // g, rows]), G_IDX: ("I32", [cols])}
            for suffix, (dtype, shape) in want.items():
                c = header.get(stem + suffix)
                if c is None:
                    self._fail(f"tensor {name} is a GPTQ weight but the checkpoint has no {stem + suffix}")
                if c["dtype"] != dtype or list(c["shape"]) != shape:
                    self._fail(f"tensor {stem + suffix} is {c['dtype']} {c['shape']}, {dtype} {shape} expected for "
                               f"{name} {rec['shape']} in groups of {g}")
            if stem + WEIGHT_SUFFIX in header:
                self._fail(f"tensor {stem + WEIGHT_SUFFIX} stands next to {name}")
            self.keys[stem + WEIGHT_SUFFIX] = (name,) + tuple(stem + c for c in COMPANIONS)

    def _fail(self, what: str):
        raise GptqModelError(f"GPTQ checkpoint {self.uri}: {what}")

    @property
    def stored_names(self):
        """every stored tensor that belongs to a weight and is no tensor of the model"""
        return {n for quad in self.keys.values() for n in quad}

    def model_keys(self, keys):
        """the tensor list of the model the checkpoint stands for: the four names of a weight are its ``X.weight``"""
        return (set(keys) - self.stored_names) | set(self.keys)

    def shape(self, name: str):
        """the shape [R, C] of the tensor ``X.weight`` that `name` stands for"""
        eighth, r = self.header[self.keys[name][0]]["shape"]
        return [int(r), 8 * int(eighth)]


def gptq_model(uri: str, path: Path, weight_map: Dict[str, str]) -> Optional[GptqModel]:
    """the GptqModel of a full model directory; None unless config.json says gptq and a shard holds the four tensors"""
    if not says_gptq(path):
        return None
    m = GptqModel(uri, path, weight_map)
    return m if m.claimed else None


def gptq_identity(path: Path) -> Optional[Dict[str, str]]:
    """what decides a GPTQ checkpoint's content for a resumed run: its shard headers; None for anything else"""
    path = Path(path)
    if not (path / FULL_INDEX).exists():
        return None
    try:
        weight_map = json.loads((path / FULL_INDEX).read_bytes())["weight_map"]
        m = gptq_model(str(path), path, weight_map)
    except (OSError, ValueError, KeyError):
        return None
    return m.identity if m is not None else None
