"""PcbMerge: PCB-Merging (Du et al., "Parameter Competition Balancing for Model Merging", NeurIPS 2024) - every entry
of every weighted delta gets a continuous weight of its own.  Its score is how large the entry is within its own
finetune (intra-balancing: the magnitude, clamped at the ``pcb_clip`` share of both ends and min-max normalised, through
``exp``) times how well it agrees with what all finetunes together do to that weight (inter-balancing: ``tanh`` of the
entry times the sum; an entry that opposes the sum scores 0).  Each finetune keeps its ``pcb_ratio`` highest scores of a
tensor, rescaled to [0, 1], and the clamped entries are averaged with those weights.  The reference has no such
operator; the function is defined in include/shardmerge_hip.h (``smhip_pcb_merge``) and runs in the HIP kernels of
csrc/sm_pcb.hpp (and the selection kernels of the task-vector statistics) behind ``Engine.pcb_merge``.

Tensor routing is FourierMerge's, as with TiesMerge: only the block-tensor merge (``merge_block``) differs."""
from __future__ import annotations

import logging

from ..config import PCB_OPTION_DEFAULTS
from .ties import TiesMerge

logger = logging.getLogger(__name__)


class PcbMerge(TiesMerge):
    option_defaults = PCB_OPTION_DEFAULTS

    def get_readme(self) -> str:
        return self._readme("PCB", f"PCB (parameter competition balancing: score every entry within its finetune and against "
                                   f"the sum, keep the highest scores, average by score), ratio {self.pcb_ratio:g}, "
                                   f"clip {self.pcb_clip:g}, lambda {self.pcb_lambda:g}")

    def merge_block(self, eng, fts, bases, alphas, base_out, name: str):
        return eng.pcb_merge(fts, bases, alphas, base_out, ratio=self.pcb_ratio, clip=self.pcb_clip, lam=self.pcb_lambda,
                             layer_name=name)

    def tensor_passes(self, k: int) -> int:
        # three levels of k + 1 for the clip's order statistics, three for the scores', the fused pass k + 2
        return 7 * k + 8

    def _log_block(self, name: str, k: int, report):
        logger.info(f"Merged {name}: {k} model(s), PCB covered {report.covered} of {report.n} ({report.contested} contested), "
                    f"selected {report.selected} of {report.q} asked, positive {report.positive}")
