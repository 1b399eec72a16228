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
round to nearest, not by the GPTQ solver; the four tensors take the place of a named module's ``X.weight`` with ``R % 8
== 0`` and ``C % group_size == 0``, any other is copied - and ``dequantize-gptq`` turns one back (merge/quantize.py).
Everything this module rejects is rejected before any output is written, and the message names the model and the
tensor or field.
"""
from __future__ import annotations

from typing import Dict

from .quantformat import CONFIG_BLOCK, QuantModel, quant_blocks

QUANT_METHOD = "gptq"
GROUPS = (32, 64, 128)
WEIGHT_SUFFIX = ".weight"
QWEIGHT, QZEROS, SCALES, G_IDX = ".qweight", ".qzeros", ".scales", ".g_idx"
COMPANIONS = (QZEROS, SCALES, G_IDX)


class GptqModelError(ValueError):
    """a GPTQ checkpoint this build cannot read; the message names the model and the tensor or field"""


def _is_quad(header: Dict, name: str) -> bool:
    return (name.endswith(QWEIGHT) and header[name]["dtype"] == "I32"
            and all(name[: -len(QWEIGHT)] + c in header for c in COMPANIONS))


class GptqModel(QuantModel):
    """`keys`: the name ``X.weight`` of the tensor they stand for -> the names of (qweight, qzeros, scales, g_idx);
    `group_size`: the checkpoint's"""
    NAME, A_NAME, A_LABEL, KEY, SUFFIX, Error = "GPTQ", "a GPTQ", "a GPTQ", "gptq", "gptq", GptqModelError
    EXPECTED = ("is no GPTQ checkpoint (quant_method 'gptq' in config.json and I32 qweight tensors with their qzeros, scales "
                "and g_idx are expected)")
    OPTIONS = {"group_size": (GROUPS, 128, "Input columns that share a scale and a zero-point")}
    QUANTIZE_HELP = """MODEL as a GPTQ-layout INT4 checkpoint, quantised by ROUND TO NEAREST (asymmetric) - not by the GPTQ solver.

    DIR receives the shards (X.qweight as I32 [C / 8, R], X.qzeros as I32 [C / g, R / 8], X.scales as F16 [C / g, R] and
    X.g_idx as I32 [C] in place of X.weight), model.safetensors.index.json and a config.json with the
    quantization_config block; it can be named as a finetune_merge entry of `merge` in place of MODEL.  A weight whose
    rows are no multiple of 8 or whose columns are no multiple of the group size is copied as it is.
    """
    DEQUANTIZE_HELP = """The GPTQ checkpoint MODEL written out in 16 or 32 bits: X.weight = (code - zero-point) times its group's scale.

    DIR can be named wherever `merge` takes a full model: as base, output_base_model or a finetune_merge entry.
    """

    @classmethod
    def says(cls, path, header) -> bool:
        return (quant_blocks(path).get(CONFIG_BLOCK, {}).get("quant_method") == QUANT_METHOD
                and any(_is_quad(header, n) for n in header))

    def validate(self):
        header, field = self.header, CONFIG_BLOCK
        qc = quant_blocks(self.path)[field]
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

    def shape(self, name):
        eighth, r = self.header[self.keys[name][0]]["shape"]
        return [int(r), 8 * int(eighth)]

    def dequant(self, engine, tensors, dtype, layer_name):
        return engine.gptq_dequant(*tensors, dtype, layer_name=layer_name)

    def summary(self) -> str:
        return f"GPTQ checkpoint, {len(self.keys)} INT4 tensors in groups of {self.group_size}"

    @classmethod
    def check_options(cls, command, group_size=128):
        if group_size not in GROUPS:
            raise ValueError(f"{command}: --group-size {group_size} is not one of {list(GROUPS)}")

    @classmethod
    def fits(cls, shape, group_size=128) -> bool:
        return shape[0] % 8 == 0 and shape[1] % group_size == 0

    @classmethod
    def unfit(cls, shape, group_size=128) -> str:
        return f"{list(shape)} is not rows a multiple of 8 by columns a multiple of {group_size}"

    @classmethod
    def quant(cls, engine, tensor, layer_name, group_size=128):
        stem = layer_name[: -len(WEIGHT_SUFFIX)]
        *four, rep = engine.gptq_quant(tensor, group_size, layer_name=layer_name)
        return ({stem + suffix: v.cpu() for suffix, v in zip((QWEIGHT,) + COMPANIONS, four)},
                {"groups": rep.groups, "zero_groups": rep.zero_groups, "scale_clamped": rep.scale_clamped, "clipped": rep.clipped},
                f"{rep.groups} groups of {group_size} ({rep.zero_groups} of zeros, {rep.scale_clamped} with a clamped scale), "
                f"{rep.clipped} clipped, {rep.nonfinite} non-finite")

    @classmethod
    def quantization_config(cls, not_converted, group_size=128):
        return {"quant_method": QUANT_METHOD, "bits": 4, "group_size": group_size, "desc_act": False, "sym": False,
                "checkpoint_format": "gptq", "modules_to_not_convert": sorted(not_converted)}
