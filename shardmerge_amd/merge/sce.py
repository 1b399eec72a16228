"""SceMerge: SCE (Wan et al., FuseChat, 2024; mergekit's ``merge_method: sce``) - SELECT the parameters whose deltas vary
most across the finetunes (the ``select_topk`` share of the nonzero variances), CALCULATE a weight per finetune from the
energy of what it kept, ERASE the entries whose sign disagrees with the majority, and add the weighted rest onto
output_base_model.  The reference has no such operator; the function is defined in include/shardmerge_hip.h
(``smhip_sce_merge``) and runs in the HIP kernels of csrc/sm_sce.hpp behind ``Engine.sce_merge``: the exact radix select
of TIES on ONE stream of variance scores, then the ordered fp64 sums of the geometric operators, then one fused pass.

Tensor routing is FourierMerge's, as with TiesMerge: only the block-tensor merge (``merge_block``) differs."""
from __future__ import annotations

import logging

from ..config import SCE_OPTION_DEFAULTS
from .ties import TiesMerge

logger = logging.getLogger(__name__)


class SceMerge(TiesMerge):
    option_defaults = SCE_OPTION_DEFAULTS

    def get_readme(self) -> str:
        return self._readme("SCE", f"SCE (sce: select the most variant parameters, calculate the weights from their energy, erase "
                                   f"the minority sign), select_topk {self.select_topk:g}, sce_lambda {self.sce_lambda:g}")

    def merge_block(self, eng, fts, bases, alphas, base_out, name: str):
        return eng.sce_merge(fts, bases, alphas, base_out, select_topk=self.select_topk, lam=self.sce_lambda, layer_name=name)

    def tensor_passes(self, k: int) -> int:
        # with selection: three levels of k + 1, the energy pass k + 1, the merge k + 2; without: the last two
        return 2 * k + 3 if self.select_topk == 1.0 else 5 * k + 6

    def _log_block(self, name: str, k: int, report):
        logger.info(f"Merged {name}: {k} model(s), SCE selected {report.selected} of {report.k_keep} asked ({report.nz} nonzero variances), "
                    f"threshold {report.threshold:.4g}, weights {[float(f'{w:.4g}') for w in report.weights]}")
