"""MXFP4 checkpoints as finetunes: a full model whose 2-D weights are stored as E2M1 codes, two to a byte, with one E8M0
power-of-two scale per block of 32 consecutive elements of a row - the OCP micro-scaling form (as recalled: PAPERS.md).

A model directory is an MXFP4 checkpoint when BOTH hold: its ``config.json`` has ``quantization_config.quant_method ==
"mxfp4"``, and a shard header holds a ``U8`` tensor ``X.weight`` of shape ``[R, C / 2]`` with a ``U8`` tensor
``X.weight_scale`` of shape ``[R, C / 32]``.  ``U8`` alone decides nothing.  The block must say ``weight_block_size:
[1, 32]`` and, when it names one, ``scale_format: "e8m0"``; every 2-D ``U8`` ``*.weight`` must come with its scale.  As a
``finetune_merge`` entry its tensor ``X.weight`` is ``Engine.mx4_dequant(X.weight, X.weight_scale, dtype of the base's
X.weight)`` (the function is stated in include/shardmerge_hip.h, smhip_mx4_dequant); the tensors it keeps in 16 or 32
bits pass as they are.  ``python -m shard quantize-mxfp4`` writes one - a named module's weight with ``C % 32 != 0`` is
copied and listed under ``modules_to_not_convert`` with the rest - and ``dequantize-mxfp4`` turns one back
(merge/quantize.py).  Everything this module rejects is rejected before any output is written, and the message names
the model and the tensor or field.
"""
from __future__ import annotations

from .quantformat import CONFIG_BLOCK, QuantModel, quant_blocks

CODE_DTYPE = "U8"
SCALE_SUFFIX = "_scale"
BLOCK = 32
QUANT_METHOD = "mxfp4"
SCALE_FORMAT = "e8m0"


class Mx4ModelError(ValueError):
    """an MXFP4 checkpoint this build cannot read; the message names the model and the tensor or field"""


def scale_shape(code_shape, block: int = BLOCK):
    """the shape of the block scales of codes [R, C / 2]: [R, C / block]"""
    return [int(code_shape[0]), 2 * int(code_shape[1]) // block]


class E2m1Model(QuantModel):
    """what MXFP4 and NVFP4 (nv4model.py) share: a weight [R, C], C a multiple of the format's BLOCK, as codes [R, C / 2]"""
    BLOCK = 0

    def shape(self, name):
        r, half = self.header[name]["shape"]
        return [int(r), 2 * int(half)]

    @classmethod
    def fits(cls, shape) -> bool:
        return shape[1] % cls.BLOCK == 0

    @classmethod
    def unfit(cls, shape) -> str:
        return f"its {shape[1]} columns are no multiple of {cls.BLOCK}"

    @staticmethod
    def columns(record) -> str:
        return f" {record['blocks']:8d} blocks  {record['saturated']:8d} saturated"


class Mx4Model(E2m1Model):
    """`keys`: tensor name -> (its own name: the codes, its scale's key)"""
    NAME, A_NAME, A_LABEL, KEY, SUFFIX, Error = "MXFP4", "an MXFP4", "an MXFP4", "mx4", "mxfp4", Mx4ModelError
    EXPECTED = ("is no MXFP4 checkpoint (quantization_config.quant_method 'mxfp4' and U8 weights with their U8 scales are "
                "expected)")
    QUANTIZE_HELP = """MODEL as an MXFP4 checkpoint: E2M1 weights, two to a byte, with one E8M0 scale per 32 elements of a row.

    DIR receives the shards (X.weight as U8 [R, C / 2], X.weight_scale as U8 [R, C / 32]), model.safetensors.index.json
    and a config.json with the quantization_config block; it can be named as a finetune_merge entry of `merge` in place
    of MODEL.  A weight whose row length is no multiple of 32 is copied as it is.
    """
    DEQUANTIZE_HELP = """The MXFP4 checkpoint MODEL written out in 16 or 32 bits: code times its block's power-of-two scale.

    DIR can be named wherever `merge` takes a full model: as base, output_base_model or a finetune_merge entry.
    """
    BLOCK = BLOCK

    @classmethod
    def says(cls, path, header) -> bool:
        return quant_blocks(path).get(CONFIG_BLOCK, {}).get("quant_method") == QUANT_METHOD

    def validate(self):
        qc = quant_blocks(self.path)[CONFIG_BLOCK]
        if list(qc.get("weight_block_size") or []) != [1, BLOCK]:
            self._fail(f"quantization_config.weight_block_size {qc.get('weight_block_size')!r} is not [1, {BLOCK}]")
        if qc.get("scale_format", SCALE_FORMAT) != SCALE_FORMAT:
            self._fail(f"quantization_config.scale_format {qc.get('scale_format')!r} is not {SCALE_FORMAT!r}")
        for name, rec in self.header.items():
            if rec["dtype"] != CODE_DTYPE or not name.endswith(".weight"):
                continue
            key = name + SCALE_SUFFIX
            if len(rec["shape"]) != 2 or (2 * rec["shape"][1]) % BLOCK:
                self._fail(f"tensor {name} is {CODE_DTYPE} {rec['shape']}; MXFP4 codes are [R, C / 2] with C a multiple of {BLOCK}")
            sc = self.header.get(key)
            if sc is None:
                self._fail(f"tensor {name} is {CODE_DTYPE} but the checkpoint has no {key}")
            if sc["dtype"] != CODE_DTYPE or list(sc["shape"]) != scale_shape(rec["shape"]):
                self._fail(f"tensor {key} is {sc['dtype']} {sc['shape']}, {CODE_DTYPE} {scale_shape(rec['shape'])} expected for "
                           f"the codes {name} {rec['shape']} in blocks of {BLOCK}")
            self.keys[name] = (name, key)

    @property
    def scale_keys(self):
        """tensor name -> its scale's key"""
        return {name: stored[1] for name, stored in self.keys.items()}

    def dequant(self, engine, tensors, dtype, layer_name):
        return engine.mx4_dequant(*tensors, dtype, layer_name=layer_name)

    def summary(self) -> str:
        return f"MXFP4 checkpoint, {len(self.keys)} micro-scaled E2M1 tensors"

    @classmethod
    def quant(cls, engine, tensor, layer_name):
        codes, scale, rep = engine.mx4_quant(tensor, layer_name=layer_name)
        return ({layer_name: codes.cpu(), layer_name + SCALE_SUFFIX: scale.cpu()},
                {"blocks": rep.blocks, "zero_blocks": rep.zero_blocks, "saturated": rep.saturated},
                f"{rep.blocks} blocks ({rep.zero_blocks} of zeros), {rep.saturated} saturated, {rep.nonfinite} non-finite")

    @classmethod
    def quantization_config(cls, not_converted):
        return {"quant_method": QUANT_METHOD, "weight_block_size": [1, BLOCK], "scale_format": SCALE_FORMAT,
                "modules_to_not_convert": sorted(not_converted)}
