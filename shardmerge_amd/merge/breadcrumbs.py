"""BreadcrumbsMerge / BreadcrumbsTiesMerge: Model Breadcrumbs (Davari & Belilovsky, 2023) - trim each finetune's delta
at BOTH ends: drop its ``gamma`` share of largest magnitudes (the outliers that dominate a merge of several finetunes)
and keep the next ``density`` share, dropping the small rest as TIES does; then add the weighted masked deltas
(``breadcrumbs``) or elect a sign and merge the agreeing entries as TIES does (``breadcrumbs_ties``), and add the result
onto output_base_model.  The reference has no such operator; the function is defined in include/shardmerge_hip.h
(``smhip_breadcrumbs_merge``) and runs in three HIP kernels (csrc/sm_breadcrumbs.hpp) behind
``Engine.breadcrumbs_merge``: both thresholds of a finetune come out of the same three histogram passes TIES spends on
its one.

Tensor routing is FourierMerge's, as with TiesMerge: only the block-tensor merge (``merge_block``) differs."""
from __future__ import annotations

import logging

from ..config import BREADCRUMBS_OPTION_DEFAULTS
from .ties import TiesMerge

logger = logging.getLogger(__name__)


class BreadcrumbsMerge(TiesMerge):
    sign_election = False
    mode = "breadcrumbs"

    option_defaults = BREADCRUMBS_OPTION_DEFAULTS                # (density 0.9, not TIES's 0.2; TIES's passes over the tensor)

    def get_readme(self) -> str:
        how, norm = self._how_and_norm(self.breadcrumbs_normalize)
        return self._readme("Breadcrumbs", f"Model Breadcrumbs ({self.mode}: drop the largest and the smallest magnitudes, {how}), "
                                           f"density {self.density:g}, gamma {self.gamma:g}, lambda {self.breadcrumbs_lambda:g}, {norm}")

    def merge_block(self, eng, fts, bases, alphas, base_out, name: str):
        return eng.breadcrumbs_merge(fts, bases, alphas, base_out, density=self.density, gamma=self.gamma,
                                     lam=self.breadcrumbs_lambda, normalize=bool(self.breadcrumbs_normalize),
                                     sign_election=self.sign_election, layer_name=name)

    def _log_block(self, name: str, k: int, report):
        logger.info(f"Merged {name}: {k} model(s), Breadcrumbs ({self.mode}) kept {report.kept} of {report.k_keep} asked, "
                    f"dropped {report.dropped_top} of at most {report.n_top} at the top, thresholds "
                    f"{[(float(f'{lo:.4g}'), float(f'{hi:.4g}')) for lo, hi in zip(report.thresholds_lo, report.thresholds_hi)]}")


class BreadcrumbsTiesMerge(BreadcrumbsMerge):
    sign_election = True
    mode = "breadcrumbs_ties"
