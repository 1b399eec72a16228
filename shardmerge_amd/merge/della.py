"""DellaMerge / DellaLinearMerge: DELLA (Deep et al., "DELLA-Merging", 2024; mergekit's ``della`` and ``della_linear``) -
DARE whose keep probability rises with the rank of each entry's magnitude within its row, from ``density - epsilon``
for the smallest magnitude to ``density + epsilon`` for the largest; the survivors are rescaled by the inverse of their
own probability and the deltas merged as TIES does (``della``) or added (``della_linear``).  The reference has no such
operator; the function is defined in include/shardmerge_hip.h (``smhip_della_merge``) and runs in the HIP kernels of
csrc/sm_della.hpp behind ``Engine.della_merge``: an exact rank per row (a whole-row sort in LDS; equal magnitudes share
a rank), then the fused pass of DARE with a threshold per element.

The mask, its key and its streams are DARE's (dare.py): a function of (seed, tensor name, position of the entry in
``finetune_merge``, element index).  ``epsilon: 0`` is ``dare_ties`` / ``dare_linear`` bit for bit.  The row is the last
dimension of the tensor; a row longer than 32768 elements is an error raised when the tensor is reached.

Tensor routing is FourierMerge's, as with TiesMerge: only the block-tensor merge (``merge_block``) differs."""
from __future__ import annotations

import logging

from ..config import DELLA_OPTION_DEFAULTS, della_thresholds
from .dare import DareTiesMerge, tensor_key

logger = logging.getLogger(__name__)


class DellaMerge(DareTiesMerge):
    sign_election = True
    mode = "della"

    option_defaults = DELLA_OPTION_DEFAULTS

    def get_readme(self) -> str:
        t_lo, t_hi = della_thresholds(self.density, self.epsilon)
        how, norm = self._how_and_norm(self.della_normalize)
        return self._readme("DELLA", f"DELLA ({self.mode}: drop at random by magnitude rank within each row, "
                                     f"{'rescale' if self.della_rescale else 'no rescale'}, {how}), density {self.density:g}, "
                                     f"epsilon {self.epsilon:g} (effective {t_lo}/65536 = {t_lo / 65536.0:.6g} .. "
                                     f"{t_hi}/65536 = {t_hi / 65536.0:.6g}), lambda {self.della_lambda:g}, seed {self.seed}, {norm}")

    def merge_block(self, eng, fts, bases, alphas, base_out, name: str):
        return eng.della_merge(fts, bases, alphas, base_out, density=self.density, epsilon=self.epsilon, lam=self.della_lambda,
                               normalize=bool(self.della_normalize), rescale=bool(self.della_rescale),
                               sign_election=self.sign_election, key=tensor_key(self.seed, name),
                               stream_ids=self.stream_ids(name, len(fts)), layer_name=name)

    def tensor_passes(self, k: int) -> int:
        # the rank pass reads k + 1 tensors twice (the second time mostly from cache) and writes k half-size ones, the merge
        # reads them with its k + 2; without a window it is DARE's one pass
        return k + 2 if self.epsilon == 0 or self.density == 1 else 3 * k + 4

    def _log_block(self, name: str, k: int, report):
        logger.info(f"Merged {name}: {k} model(s), DELLA ({self.mode}) kept {report.kept} at thresholds "
                    f"{report.threshold_lo}/65536 .. {report.threshold_hi}/65536")


class DellaLinearMerge(DellaMerge):
    sign_election = False
    mode = "della_linear"
