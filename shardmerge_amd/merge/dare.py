"""DareTiesMerge / DareLinearMerge: DARE (Yu et al., "Language Models are Super Mario", 2023) - drop each entry of a
finetune's delta at random with probability 1 - density, rescale the survivors by 1 / density, then merge the deltas
as TIES does (``dare_ties``: elect a sign, merge the agreeing entries) or add them (``dare_linear``), and add the
result onto output_base_model.  The reference has no such operator; the function is defined in
include/shardmerge_hip.h (``smhip_dare_merge``) and runs in ONE HIP kernel (csrc/sm_dare.hpp) behind
``Engine.dare_merge``.

The random mask is a function, not a stream: Philox4x32-10 keyed by (seed, tensor name), with the entry's position
in ``finetune_merge`` as the stream and the element's index as the counter.  The same config therefore gives the same
bytes in one process, in place, and on any number of ranks, and a model's mask does not change when another entry's
layer window does.

Tensor routing is FourierMerge's, as with TiesMerge: only the block-tensor merge (``merge_block``) differs."""
from __future__ import annotations

import hashlib
import logging

from ..config import DARE_OPTION_DEFAULTS
from ..writer import ShardLayer
from .ties import TiesMerge

logger = logging.getLogger(__name__)


def tensor_key(seed: int, tensor_name: str) -> int:
    """the generator's key of one tensor: the first 8 bytes, little-endian, of sha256(f"{seed}\\n{tensor_name}")"""
    return int.from_bytes(hashlib.sha256(f"{seed}\n{tensor_name}".encode()).digest()[:8], "little")


def effective_threshold(density: float) -> int:
    """T of smhip_dare_merge: an element is kept iff its 16-bit draw is below it; the density in effect is T / 65536"""
    return 65536 if density == 1 else int(float(density) * 65536.0)


class DareTiesMerge(TiesMerge):
    sign_election = True
    mode = "dare_ties"

    option_defaults = DARE_OPTION_DEFAULTS

    def __init__(self, config, index_manager=None, engine=None, **kwargs):
        super().__init__(config, index_manager=index_manager, engine=engine, **kwargs)
        self.seed = int((getattr(config, "merge_options", None) or {}).get("seed", DARE_OPTION_DEFAULTS["seed"]))   # exactly

    def get_readme(self) -> str:
        T = effective_threshold(self.density)
        how, norm = self._how_and_norm(self.dare_normalize)
        return self._readme("DARE", f"DARE ({self.mode}: drop at random, {'rescale' if self.dare_rescale else 'no rescale'}, {how}), "
                                    f"density {self.density:g} (effective {T}/65536 = {T / 65536.0:.6g}), lambda {self.dare_lambda:g}, "
                                    f"seed {self.seed}, {norm}")

    def stream_ids(self, name: str, k: int):
        """positions in config.finetune_merge of the entries that cover the tensor's layer: the mask's streams"""
        number = ShardLayer(0, "", name, False).layer_number
        ids = [i for i, m in enumerate(self.config.finetune_merge) if m.use_layer_index(number)]
        if len(ids) != k:
            raise ValueError(f"{name}: {k} finetune tensors for the {len(ids)} entries of finetune_merge that cover layer {number}")
        return ids

    def merge_block(self, eng, fts, bases, alphas, base_out, name: str):
        return eng.dare_merge(fts, bases, alphas, base_out, density=self.density, lam=self.dare_lambda,
                              normalize=bool(self.dare_normalize), rescale=bool(self.dare_rescale),
                              sign_election=self.sign_election, key=tensor_key(self.seed, name),
                              stream_ids=self.stream_ids(name, len(fts)), layer_name=name)

    def tensor_passes(self, k: int) -> int:
        return k + 2

    def _log_block(self, name: str, k: int, report):
        logger.info(f"Merged {name}: {k} model(s), DARE ({self.mode}) kept {report.kept} at effective density "
                    f"{report.threshold}/65536")


class DareLinearMerge(DareTiesMerge):
    sign_election = False
    mode = "dare_linear"
