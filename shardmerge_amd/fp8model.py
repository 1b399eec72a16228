"""Block-scaled FP8 checkpoints as finetunes: a full model whose 2-D weights are stored as OCP E4M3 codes with one fp32
scale per 128 x 128 block - the Hugging Face ``quant_method: "fp8"`` layout (as recalled: PAPERS.md).

A model directory is an FP8 checkpoint when a shard header holds an ``F8_E4M3`` tensor - unless it is an NVFP4 one
(nv4model.py), whose block scales are such tensors.  Every such tensor ``X`` must come with an ``F32`` tensor
``X_scale_inv`` of shape ``[ceil(R / 128), ceil(C / 128)]``; ``config.json``, when it has a ``quantization_config``,
must say ``quant_method: "fp8"``, ``fmt: "e4m3"`` and ``weight_block_size: [128, 128]``.  As a ``finetune_merge`` entry
its tensor ``X`` is ``Engine.fp8_dequant(X, X_scale_inv, dtype of the base's X)`` (the function is stated in
include/shardmerge_hip.h, smhip_fp8_dequant); the tensors it keeps in 16 or 32 bits pass as they are.  ``python -m shard
quantize-fp8`` writes one, every named 2-D weight whatever its shape, and ``dequantize-fp8`` turns one back
(merge/quantize.py).  Everything this module rejects is rejected before any output is written, and the message names
the model and the tensor or field.
"""
from __future__ import annotations

from .quantformat import CONFIG_BLOCK, QuantModel, quant_blocks

FP8_DTYPE = "F8_E4M3"
SCALE_SUFFIX = "_scale_inv"
BLOCK = 128
QUANT_METHOD = "fp8"
FMT = "e4m3"


class Fp8ModelError(ValueError):
    """an FP8 checkpoint this build cannot read; the message names the model and the tensor or field"""


def scale_shape(shape):
    return [-(-int(shape[0]) // BLOCK), -(-int(shape[1]) // BLOCK)]


class Fp8Model(QuantModel):
    """`keys`: tensor name -> (its own name: the codes, its scale's key)"""
    NAME, A_NAME, A_LABEL, KEY, SUFFIX, Error = "FP8", "an FP8", "a block-scaled FP8", "fp8", "fp8", Fp8ModelError
    EXPECTED = f"holds no {FP8_DTYPE} tensor; an FP8 checkpoint is expected"
    QUANTIZE_HELP = """MODEL as a block-scaled FP8 checkpoint: E4M3 weights with one fp32 scale per 128 x 128 block.

    DIR receives the shards (X.weight as F8_E4M3, X.weight_scale_inv as F32), model.safetensors.index.json and a
    config.json with the quantization_config block; it can be named as a finetune_merge entry of `merge` in place of MODEL.
    """
    DEQUANTIZE_HELP = """The block-scaled FP8 checkpoint MODEL written out in 16 or 32 bits: code times its block's scale, rounded once.

    DIR can be named wherever `merge` takes a full model: as base, output_base_model or a finetune_merge entry.
    """

    @classmethod
    def says(cls, path, header) -> bool:
        return any(rec["dtype"] == FP8_DTYPE for rec in header.values())

    def validate(self):
        for name, rec in self.header.items():
            if rec["dtype"] != FP8_DTYPE:
                continue
            key = name + SCALE_SUFFIX
            if len(rec["shape"]) != 2:
                self._fail(f"tensor {name} is {FP8_DTYPE} {rec['shape']}; only 2-D tensors are block-scaled")
            sc = self.header.get(key)
            if sc is None:
                self._fail(f"tensor {name} is {FP8_DTYPE} but the checkpoint has no {key}")
            if sc["dtype"] != "F32" or list(sc["shape"]) != scale_shape(rec["shape"]):
                self._fail(f"tensor {key} is {sc['dtype']} {sc['shape']}, F32 {scale_shape(rec['shape'])} expected for "
                           f"{name} {rec['shape']} in blocks of {BLOCK} x {BLOCK}")
            self.keys[name] = (name, key)
        try:
            qc = quant_blocks(self.path, strict=True).get(CONFIG_BLOCK)
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

    def shape(self, name):
        return list(self.header[name]["shape"])

    def dequant(self, engine, tensors, dtype, layer_name):
        return engine.fp8_dequant(*tensors, dtype, name=layer_name)

    def summary(self) -> str:
        return f"FP8 checkpoint, {len(self.keys)} block-scaled E4M3 tensors"

    @classmethod
    def quant(cls, engine, tensor, layer_name):
        codes, scale, rep = engine.fp8_quant(tensor, name=layer_name)
        return ({layer_name: codes.cpu(), layer_name + SCALE_SUFFIX: scale.cpu()},
                {"blocks": rep.blocks, "zero_blocks": rep.zero_blocks, "amax": rep.amax},
                f"{rep.blocks} blocks ({rep.zero_blocks} of zeros), amax {rep.amax:.6g}")

    @classmethod
    def quantization_config(cls, not_converted):
        return {"quant_method": QUANT_METHOD, "fmt": FMT, "activation_scheme": "dynamic", "weight_block_size": [BLOCK, BLOCK],
                "modules_to_not_convert": sorted(not_converted)}

    @staticmethod
    def columns(record) -> str:
        return f" {record['blocks']:8d} blocks  amax {record['amax']:.6g}"
