"""Quantised checkpoint formats as finetunes: what block-scaled FP8 (fp8model.py), MXFP4 (mx4model.py), NVFP4
(nv4model.py) and GPTQ-layout INT4 (gptqmodel.py) checkpoints share, and the one place that tells them apart.

A format is a subclass of `QuantModel`.  The class describes the format - its names, how a directory says it is one,
what its quantiser takes and writes; an instance is the quantised tensors of one full model, validated against the
shard headers and the config files alone.  `claim` reads a model directory's shard headers once and asks every format of
`formats()` in turn; `identity_of` is what a resumed run compares (distributed.config_stamp).  The index
(`LocalModelIndex.quant`), the merge (merge/base.py) and the commands (merge/quantize.py, __main__.py) know a checkpoint
through this interface only: a further format is one module and one entry of `formats()`.
"""
from __future__ import annotations

import hashlib
import json
from pathlib import Path
from typing import Dict, List, Optional, Tuple

from .adapter import FULL_INDEX, read_header

CONFIG_BLOCK = "config.json quantization_config"
HF_QUANT_CONFIG = "hf_quant_config.json"
HF_BLOCK = f"{HF_QUANT_CONFIG} quantization"


def read_headers(path: Path, weight_map: Dict[str, str]) -> Tuple[Dict, str]:
    """(the merged header of the shards `weight_map` names, the sha256 over every shard's name and raw header in sorted
    shard order: offsets, shapes and metadata of every shard) of the model directory `path`"""
    sha = hashlib.sha256()
    header = {}
    for shard in sorted(set(weight_map.values())):
        raw, doc = read_header(Path(path) / shard)
        sha.update(shard.encode() + b"\0" + raw)
        header.update(doc)
    return header, sha.hexdigest()


def _read_json(path: Path, strict: bool) -> Optional[Dict]:
    try:
        doc = json.loads(path.read_bytes())
    except OSError:
        return None
    except ValueError:
        if strict:
            raise
        return None
    return doc if isinstance(doc, dict) else None


def quant_blocks(path: Path, strict: bool = False) -> Dict[str, Dict]:
    """the blocks of a model directory that can name its quantisation, by the field path a message names them with:
    config.json's ``quantization_config`` and the ``quantization`` block (or the whole) of hf_quant_config.json.  A file
    that is missing, unreadable or no JSON object has no block; strict: a config.json that is not JSON raises ValueError"""
    path = Path(path)
    found = {}
    qc = (_read_json(path / "config.json", strict) or {}).get("quantization_config")
    if isinstance(qc, dict):
        found[CONFIG_BLOCK] = qc
    hq = _read_json(path / HF_QUANT_CONFIG, False)
    if hq is not None:
        inner = hq.get("quantization")
        found[HF_BLOCK] = inner if isinstance(inner, dict) else hq
    return found


class QuantModel:
    """the quantised tensors of the full model at `path`.  `keys`: the name of a tensor of the model -> the names of the
    stored tensors `dequant` takes, in its order; `identity`: what decides the checkpoint's content for a resumed run"""
    NAME = ""           # "FP8": how messages, logs and help strings name the format
    A_NAME = ""         # "an FP8": the same with its article
    A_LABEL = ""        # "a block-scaled FP8": what a rejection of the checkpoint calls it
    KEY = ""            # "fp8": LocalModelIndex's accessor, the stamp's "fp8_models" and "fp8_headers"
    SUFFIX = ""         # "fp8": the commands quantize-fp8 and dequantize-fp8
    Error = ValueError  # what `_fail` raises
    SHADOWS: Tuple[str, ...] = ()   # the KEYs of the formats that would claim this one's directories for its scale tensors
    EXPECTED = ""       # what `dequantize-SUFFIX MODEL` says of a MODEL that is no checkpoint of the format, after "MODEL "
    OPTIONS: Dict[str, tuple] = {}  # what `quantize-SUFFIX` takes beyond the common options: name -> (choices, default, help)
    QUANTIZE_HELP = DEQUANTIZE_HELP = ""     # the commands' --help texts

    def __init__(self, uri: str, path: Path, header: Dict, digest: str):
        self.uri, self.path, self.header = uri, Path(path), header
        self.identity = {f"{self.KEY}_headers": digest}
        self.keys: Dict[str, Tuple[str, ...]] = {}
        self.validate()

    # ---- what a format fills in: the checkpoint side -----------------------------------------------------------
    @classmethod
    def says(cls, path: Path, header: Dict) -> bool:
        """whether the directory says it is a checkpoint of this format (its config files, its tensors' dtypes and names)"""
        raise NotImplementedError

    def validate(self):
        """fills `keys` from a directory that `says` so; `_fail`s at what this build does not read.  A directory that
        leaves `keys` empty is none of this format after all"""
        raise NotImplementedError

    def shape(self, name: str) -> List[int]:
        """the shape [R, C] of the model's tensor `name` of `keys`"""
        raise NotImplementedError

    def dequant(self, engine, tensors, dtype, layer_name: str):
        """the model's tensor from the stored ones of a `keys` entry, in `dtype`: the format's `Engine.*_dequant`"""
        raise NotImplementedError

    def summary(self) -> str:
        """the index's log line"""
        raise NotImplementedError

    # ---- what a format fills in: the quantiser side (`options`: a value for each of OPTIONS) --------------------
    @classmethod
    def check_options(cls, command: str, **options):
        """raises ValueError for an option value the quantiser does not take"""

    @classmethod
    def fits(cls, shape, **options) -> bool:
        """whether the quantiser takes a 2-D weight of this shape; `unfit` says why not"""
        return True

    @classmethod
    def unfit(cls, shape, **options) -> str:
        raise NotImplementedError

    @classmethod
    def quant(cls, engine, tensor, layer_name: str, **options):
        """(stored tensors by name, the report record's fields beyond name and shape, the log line's tail) of the
        model's tensor `layer_name`: the format's `Engine.*_quant`"""
        raise NotImplementedError

    @classmethod
    def quantization_config(cls, not_converted, **options) -> Dict:
        """the ``quantization_config`` block of a checkpoint `quantize-SUFFIX` writes"""
        raise NotImplementedError

    @staticmethod
    def columns(record: Dict) -> str:
        """what the printed table shows of a quantised tensor's report record, after its name and shape"""
        return ""

    # ---- shared ------------------------------------------------------------------------------------------------
    def _fail(self, what: str):
        raise self.Error(f"{self.NAME} checkpoint {self.uri}: {what}")

    @property
    def extra_names(self):
        """every stored tensor that belongs to a weight and is no tensor of the model: scales, zero-points, and a weight's
        stored form where it goes by another name"""
        return {n for name, stored in self.keys.items() for n in stored if n != name}

    def model_keys(self, keys):
        """the tensor list of the model the checkpoint stands for, from the stored one"""
        return (set(keys) - self.extra_names) | set(self.keys)


def formats() -> Tuple[type, ...]:
    """the formats, in the order `claim` asks them: NVFP4 before FP8, which its F8_E4M3 block scales would otherwise claim"""
    from .fp8model import Fp8Model
    from .gptqmodel import GptqModel
    from .mx4model import Mx4Model
    from .nv4model import Nv4Model
    return (Nv4Model, Fp8Model, Mx4Model, GptqModel)


def claim(uri: str, path: Path, weight_map: Dict[str, str]) -> Optional[QuantModel]:
    """the QuantModel of a full model directory, None for a model no format claims.  The shard headers are read once;
    every format gets its say, so a directory one format claims and another rejects is rejected, except that a format
    the claiming one SHADOWS is not asked; two claims raise ValueError"""
    header, digest = read_headers(path, weight_map)
    found: List[QuantModel] = []
    for fmt in formats():
        if any(fmt.KEY in m.SHADOWS for m in found) or not fmt.says(path, header):
            continue
        m = fmt(uri, path, header, digest)
        if m.keys:
            found.append(m)
    if len(found) > 1:
        raise ValueError(f"{uri} is {found[0].A_LABEL} checkpoint and {found[1].A_LABEL} checkpoint at once: its config files and "
                         f"tensors say both")
    return found[0] if found else None


def identity_of(path: Path) -> Optional[Tuple[str, Dict[str, str]]]:
    """(the format's KEY, what decides the checkpoint's content for a resumed run: its shard headers) of the model
    directory `path`; None for anything else, an unreadable or a rejected directory included"""
    path = Path(path)
    if not (path / FULL_INDEX).exists():
        return None
    try:
        weight_map = json.loads((path / FULL_INDEX).read_bytes())["weight_map"]
        m = claim(str(path), path, weight_map)
    except (OSError, ValueError, KeyError):
        return None
    return (m.KEY, m.identity) if m is not None else None
