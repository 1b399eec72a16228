"""ConsensusTaMerge / ConsensusTiesMerge: Consensus Merging (Wang et al., "Localizing Task Information for Improved
Model Merging and Compression", ICML 2024) - per finetune a TALL mask marks where its own weighted delta outweighs what
the other tasks did to the same weight (``|tv_i| >= mask_lambda * |U - tv_i|``, U the multi-task vector); an element of
U is kept only where at least ``consensus_k`` masks agree, which drops the weights that serve one task only and those
that serve none.  U is the sum of the weighted deltas (``consensus_ta``, on top of task arithmetic) or the TIES merge of
them (``consensus_ties``).  The reference has no such operator; the function is defined in include/shardmerge_hip.h
(``smhip_consensus_merge``) and runs in one fused HIP kernel (csrc/sm_consensus.hpp), after the selection kernels of
TIES for ``consensus_ties``, behind ``Engine.consensus_merge``.

Tensor routing is FourierMerge's, as with TiesMerge: only the block-tensor merge (``merge_block``) differs."""
from __future__ import annotations

import logging

from ..config import CONSENSUS_OPTION_DEFAULTS
from .ties import TiesMerge

logger = logging.getLogger(__name__)


class ConsensusTaMerge(TiesMerge):
    ties = False
    mode = "consensus_ta"

    option_defaults = CONSENSUS_OPTION_DEFAULTS

    def get_readme(self) -> str:
        on = f"the TIES merge at density {self.density:g}" if self.ties else "the sum of the weighted deltas (task arithmetic)"
        norm = ("normalized by the agreeing weights" if self.ties else "normalized by the sum of the weights") \
            if self.consensus_normalize else "plain sum"
        return self._readme("Consensus", f"Consensus ({self.mode}: TALL masks on {on}, keep where the masks agree), "
                                         f"mask_lambda {self.mask_lambda:g}, consensus_k {int(self.consensus_k)}, "
                                         f"lambda {self.consensus_lambda:g}, {norm}")

    def merge_block(self, eng, fts, bases, alphas, base_out, name: str):
        return eng.consensus_merge(fts, bases, alphas, base_out, ties=self.ties, density=self.density,
                                   mask_lambda=self.mask_lambda, consensus_k=int(self.consensus_k),
                                   lam=self.consensus_lambda, normalize=bool(self.consensus_normalize), layer_name=name)

    def tensor_passes(self, k: int) -> int:
        # the one fused pass k + 2; consensus_ties: three selection levels of k + 1 before it
        return 4 * k + 5 if self.ties else k + 2

    def _log_block(self, name: str, k: int, report):
        logger.info(f"Merged {name}: {k} model(s), Consensus ({self.mode}) selected {report.selected} of {report.n}, "
                    f"agree {report.agree}, masked {report.masked}")


class ConsensusTiesMerge(ConsensusTaMerge):
    ties = True
    mode = "consensus_ties"
