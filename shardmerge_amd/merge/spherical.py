"""KarcherMerge / MultiSlerpMerge: slerp and nuslerp for any number of models - the weighted Karcher mean of the vectors'
DIRECTIONS on the unit sphere, their LENGTHS averaged linearly (nuslerp's rule; with two models of equal norm also
slerp's result).

``karcher`` works on the models' WEIGHTS, as ``slerp`` does (the bases and output_base_model do not enter a block
tensor); ``multislerp`` on the deltas ``finetune_i - base_i``, as ``nuslerp`` does, the result added onto
output_base_model.  The weights on the sphere are alpha_i / sum alpha.  ``sphere_row_wise: 1`` takes one mean per row of
each tensor; ``multislerp`` with two entries is then the row-wise NuSLERP.  The reference has no such operators; the
function is defined in include/shardmerge_hip.h (``smhip_sphere_merge``) and runs behind ``Engine.sphere_merge``: the
mean lies in the span of the vectors, so the log-map iteration runs on k coefficients against the fp64 Gram matrix of
csrc/sm_geo.hpp's Gram pass (csrc/sm_sphere.hpp; per row in the ``sphere_coef`` kernel) and never re-reads a tensor: two
streaming passes whatever the iteration count.

Tensor routing is FourierMerge's, as with TiesMerge: only the block-tensor merge (``merge_block``) differs."""
from __future__ import annotations

import logging

from ..config import SPHERE_OPTION_DEFAULTS
from .ties import TiesMerge

logger = logging.getLogger(__name__)


class MultiSlerpMerge(TiesMerge):
    mode = "multislerp"
    title = "MultiSLERP"
    space = "deltas"

    option_defaults = SPHERE_OPTION_DEFAULTS

    def _weights(self):
        alphas = [float(m.alpha) for m in self.config.finetune_merge]
        return [float(f"{a / sum(alphas):.6g}") for a in alphas]

    def get_readme(self) -> str:
        scope = "per row of each tensor" if self.sphere_row_wise else "per tensor"
        return self._readme(self.title, f"{self.title} ({self.mode}: the Karcher mean of the directions of the {self.space} on the sphere, "
                                        f"weights {self._weights()}, their lengths averaged linearly, {scope}; "
                                        f"max_iter {int(self.karcher_max_iter)}, tol {self.karcher_tol:g})")

    def merge_block(self, eng, fts, bases, alphas, base_out, name: str):
        return eng.sphere_merge(fts, bases, alphas, base_out, mode=self.mode, rowwise=bool(self.sphere_row_wise),
                                max_iter=int(self.karcher_max_iter), tol=float(self.karcher_tol), layer_name=name)

    def tensor_passes(self, k: int) -> int:
        return 2 * k + 3                      # the Gram pass reads k + 1, the combine pass reads k + 1 and writes 1

    def _log_block(self, name: str, k: int, report):
        if report.rowwise:
            logger.info(f"Merged {name}: {k} model(s), {self.title} per row, at most {report.iters_max} iteration(s), "
                        f"{report.rows_unconverged} row(s) not converged, {report.rows_linear} linear, sum of coefficients in "
                        f"[{report.csum_min:.4g}, {report.csum_max:.4g}], mean {report.csum_mean:.4g}")
        else:
            state = "linear" if report.linear else ("converged" if report.converged else "NOT converged")
            logger.info(f"Merged {name}: {k} model(s), {self.title}, {report.iterations} iteration(s), tau {report.tau:.3g} ({state}), "
                        f"coefficients {[float(f'{c:.4g}') for c in report.coefficients]}")


class KarcherMerge(MultiSlerpMerge):
    mode = "karcher"
    title = "Karcher"
    space = "weights"

    def tensor_passes(self, k: int) -> int:
        return 2 * k + 1                      # no base is read
