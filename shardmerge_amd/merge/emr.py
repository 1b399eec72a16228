"""EmrMerge: the unified model of EMR-Merging (Huang et al., "EMR-Merging: Tuning-Free High-Performance Model Merging",
NeurIPS 2024) - per element the deltas are summed, the sign of the sum is elected, and the entry of that sign with the
largest magnitude is taken as it is (``emr_lambda`` times it goes onto output_base_model).  The method has no weights and
no tuning.  The per-task masks and rescalers that recover a model per task are computed afterwards from (finetune, base,
unified model) by ``python -m shard emr-task`` (merge/emr_task.py).  The reference has no such operator; the function is
defined in include/shardmerge_hip.h (``smhip_emr_merge``) and runs in one fused HIP kernel (csrc/sm_emr.hpp) behind
``Engine.emr_merge``.

Tensor routing is FourierMerge's, as with TiesMerge: only the block-tensor merge (``merge_block``) differs."""
from __future__ import annotations

import logging

from ..config import EMR_OPTION_DEFAULTS
from .ties import TiesMerge

logger = logging.getLogger(__name__)


class EmrMerge(TiesMerge):
    option_defaults = EMR_OPTION_DEFAULTS

    def get_readme(self) -> str:
        return self._readme("EMR", f"EMR-Merging, the unified model (elect the sign of the summed deltas, take the largest "
                                   f"agreeing entry; a zero sum elects plus), lambda {self.emr_lambda:g}, no weights")

    def merge_block(self, eng, fts, bases, alphas, base_out, name: str):
        return eng.emr_merge(fts, bases, base_out, lam=self.emr_lambda, layer_name=name)

    def tensor_passes(self, k: int) -> int:
        return k + 2

    def _log_block(self, name: str, k: int, report):
        logger.info(f"Merged {name}: {k} model(s), EMR elected +{report.elected_pos} / -{report.elected_neg} / 0 {report.zero} "
                    f"of {report.n}, contested {report.contested}, winner {report.winner}, agree {report.agree}")
