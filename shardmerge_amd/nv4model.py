"""NVFP4 checkpoints as finetunes: a full model whose 2-D weights are stored as E2M1 codes, two to a byte, with one E4M3
scale per block of 16 consecutive elements of a row and one fp32 scale per tensor - the form ModelOpt writes (as
recalled: PAPERS.md).

A model directory is an NVFP4 checkpoint when BOTH hold: the ``quantization_config`` of its ``config.json``, or an
``hf_quant_config.json``, says ``quant_algo: "NVFP4"``, and a shard header holds a triple - a ``U8`` tensor ``X.weight``
of shape ``[R, C / 2]``, an ``F8_E4M3`` tensor ``X.weight_scale`` of shape ``[R, C / 16]`` and an ``F32`` tensor
``X.weight_scale_2`` of shape ``[]`` or ``[1]``.  The test runs BEFORE the FP8 one (fp8model.py), which would claim the
directory for its ``F8_E4M3`` scale tensors (``SHADOWS``); a directory it does not claim is left to the FP8 test.  A
``group_size``, where one is named, must be 16; every 2-D ``U8`` ``*.weight`` must come with both scales; an ``F8_E4M3``
tensor that is no block scale (FP8 weights mixed in) and a ``U8`` scale (MXFP4 weights mixed in) are rejected; any
``X.input_scale`` is ignored, and `dequantize-nvfp4` drops it.  As a ``finetune_merge`` entry its tensor ``X.weight`` is
``Engine.nv4_dequant(X.weight, X.weight_scale, X.weight_scale_2, dtype of the base's X.weight)`` (the function is stated
in include/shardmerge_hip.h, smhip_nv4_dequant); the tensors it keeps in 16 or 32 bits pass as they are.  ``python -m
shard quantize-nvfp4`` writes one - a named module's weight with ``C % 16 != 0`` is copied and listed under ``ignore``
with the rest - and ``dequantize-nvfp4`` turns one back (merge/quantize.py).  Everything this module rejects is rejected
before any output is written, and the message names the model and the tensor or field.
"""
from __future__ import annotations

from typing import Dict

from .mx4model import E2m1Model, scale_shape
from .quantformat import quant_blocks

CODE_DTYPE = "U8"
SCALE_DTYPE = "F8_E4M3"
SCALE_SUFFIX = "_scale"
GLOBAL_SUFFIX = "_scale_2"
INPUT_SUFFIX = ".input_scale"
BLOCK = 16
QUANT_METHOD = "modelopt"
QUANT_ALGO = "NVFP4"


class Nv4ModelError(ValueError):
    """an NVFP4 checkpoint this build cannot read; the message names the model and the tensor or field"""


def _is_triple(header: Dict, name: str) -> bool:
    rec, sc, g = header[name], header.get(name + SCALE_SUFFIX), header.get(name + GLOBAL_SUFFIX)
    return (rec["dtype"] == CODE_DTYPE and name.endswith(".weight") and len(rec["shape"]) == 2 and sc is not None
            and sc["dtype"] == SCALE_DTYPE and g is not None and g["dtype"] == "F32")


class Nv4Model(E2m1Model):
    """`keys`: tensor name -> (its own name: the codes, its block scales' key, its tensor scale's key)"""
    NAME, A_NAME, A_LABEL, KEY, SUFFIX, Error = "NVFP4", "an NVFP4", "an NVFP4", "nv4", "nvfp4", Nv4ModelError
    SHADOWS = ("fp8",)
    EXPECTED = ("is no NVFP4 checkpoint (quant_algo 'NVFP4' in config.json or hf_quant_config.json and U8 weights with "
                "their F8_E4M3 and F32 scales are expected)")
    QUANTIZE_HELP = """MODEL as an NVFP4 checkpoint: E2M1 weights, two to a byte, one E4M3 scale per 16 elements of a row, one fp32 scale per tensor.

    DIR receives the shards (X.weight as U8 [R, C / 2], X.weight_scale as F8_E4M3 [R, C / 16], X.weight_scale_2 as one
    F32), model.safetensors.index.json and a config.json with the quantization_config block; it can be named as a
    finetune_merge entry of `merge` in place of MODEL.  A weight whose row length is no multiple of 16 is copied as it is.
    """
    DEQUANTIZE_HELP = """The NVFP4 checkpoint MODEL written out in 16 or 32 bits: code times its block's scale times the tensor's scale.

    DIR can be named wherever `merge` takes a full model: as base, output_base_model or a finetune_merge entry.
    """
    BLOCK = BLOCK

    @classmethod
    def says(cls, path, header) -> bool:
        return (any(block.get("quant_algo") == QUANT_ALGO for block in quant_blocks(path).values())
                and any(_is_triple(header, n) for n in header))

    def validate(self):
        header = self.header
        for field, block in quant_blocks(self.path).items():
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
            want = scale_shape(rec["shape"], BLOCK)
            if sc["dtype"] != SCALE_DTYPE or list(sc["shape"]) != want:
                mix = " (MXFP4 and NVFP4 weights are mixed)" if sc["dtype"] == CODE_DTYPE else ""
                self._fail(f"tensor {key} is {sc['dtype']} {sc['shape']}, {SCALE_DTYPE} {want} expected for "
                           f"the codes {name} {rec['shape']} in blocks of {BLOCK}{mix}")
            if g["dtype"] != "F32" or list(g["shape"]) not in ([], [1]):
                self._fail(f"tensor {gkey} is {g['dtype']} {g['shape']}, one F32 value expected")
            self.keys[name] = (name, key, gkey)
        scales = {stored[1] for stored in self.keys.values()}
        for name, rec in header.items():
            if rec["dtype"] == SCALE_DTYPE and name not in scales:
                self._fail(f"tensor {name} is {SCALE_DTYPE} but no block scale of an NVFP4 weight (FP8 and NVFP4 weights are mixed)")
        self.ignored = {n for n in header if n.endswith(INPUT_SUFFIX)}

    @property
    def extra_names(self):
        """both scales of every weight, and the ignored input scales"""
        return super().extra_names | self.ignored

    def dequant(self, engine, tensors, dtype, layer_name):
        return engine.nv4_dequant(*tensors, dtype, layer_name=layer_name)

    def summary(self) -> str:
        return f"NVFP4 checkpoint, {len(self.keys)} two-level-scaled E2M1 tensors"

    @classmethod
    def quant(cls, engine, tensor, layer_name):
        codes, scale, g, rep = engine.nv4_quant(tensor, layer_name=layer_name)
        return ({layer_name: codes.cpu(), layer_name + SCALE_SUFFIX: scale.cpu(), layer_name + GLOBAL_SUFFIX: g},
                {"blocks": rep.blocks, "zero_blocks": rep.zero_blocks, "zero_scale_blocks": rep.zero_scale_blocks,
                 "saturated": rep.saturated},
                f"{rep.blocks} blocks ({rep.zero_blocks} of zeros, {rep.zero_scale_blocks} below their scale), {rep.saturated} "
                f"saturated, {rep.nonfinite} non-finite")

    @classmethod
    def quantization_config(cls, not_converted):
        return {"quant_method": QUANT_METHOD, "quant_algo": QUANT_ALGO, "group_size": BLOCK, "ignore": sorted(not_converted)}
