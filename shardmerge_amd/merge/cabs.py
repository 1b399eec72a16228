"""CabsMerge: CABS (Yang et al., "CABS: Conflict-Aware and Balanced Sparsification for Enhancing Model Merging", ICML
2025, as recalled: PAPERS.md) - n:m sparsification of the task vectors.  BS, balanced: every group of ``cabs_m``
consecutive weights of a row (the last dimension) keeps the ``cabs_n`` largest magnitudes of a finetune's delta, so the
budget is spent evenly over the tensor, not where one row's entries are large.  CA, conflict-aware: the finetunes are
pruned one after another, IN THE ORDER OF ``finetune_merge``, and each may keep only positions that no earlier one kept,
so the kept sets are disjoint.  The sparse deltas are added with their alphas, without normalisation.  The reference
has no such operator; the function is defined in include/shardmerge_hip.h (``smhip_cabs_merge``) and runs in one fused
HIP kernel (csrc/sm_cabs.hpp) behind ``Engine.cabs_merge``.

Tensor routing is FourierMerge's, as with TiesMerge: only the block-tensor merge (``merge_block``) differs.  On a layer,
the order of the finetunes is the order of the covering entries in ``finetune_merge``."""
from __future__ import annotations

import logging

from ..config import CABS_OPTION_DEFAULTS
from .ties import TiesMerge

logger = logging.getLogger(__name__)


class CabsMerge(TiesMerge):
    option_defaults = CABS_OPTION_DEFAULTS

    def get_readme(self) -> str:
        ca = bool(self.cabs_conflict_aware)
        order = " > ".join(m.model for m in self.config.finetune_merge)
        how = ("conflict-aware: the finetunes are pruned in the order of the entries, each only where no earlier one kept "
               "a weight, so the order is part of the result") if ca else \
            "conflict-aware off: every finetune is pruned on its own"
        return self._readme("CABS", f"CABS (n:m sparsification of the deltas within groups of a row, ties at the cut kept), "
                                    f"{int(self.cabs_n)}:{int(self.cabs_m)}, {how}, lambda {self.cabs_lambda:g}, "
                                    f"plain sum; entry order: {order}")

    def merge_block(self, eng, fts, bases, alphas, base_out, name: str):
        return eng.cabs_merge(fts, bases, alphas, base_out, n_keep=int(self.cabs_n), group=int(self.cabs_m),
                              conflict_aware=bool(self.cabs_conflict_aware), lam=self.cabs_lambda, layer_name=name)

    def tensor_passes(self, k: int) -> int:
        return k + 2                    # the one fused pass: k finetunes, the shared base, the output

    def _log_block(self, name: str, k: int, report):
        share = lambda c: float(f"{c / max(report.n, 1):.4g}")
        parts = ", ".join(f"[{i}] kept {share(report.kept[i])} short {report.short_groups[i]} surplus {report.surplus[i]}"
                          for i in range(k))
        logger.info(f"Merged {name}: {k} model(s), CABS {report.n_keep}:{report.group} "
                    f"{'conflict-aware' if report.conflict_aware else 'independent'} over {report.groups} groups, {parts}, "
                    f"covered {share(report.covered)}, overlap {share(report.overlap)}")
