"""ModelStockMerge / NuSlerpMerge / SlerpMerge: the operators whose coefficients come from the GEOMETRY of the task
vectors - their norms and the angles between them - instead of a per-element decision.

``model_stock`` (Jang et al., 2024): the finetunes of one base are averaged (weighted by alpha) and the average is pulled
towards the base by the ratio t = k cos / (1 + (k - 1) cos), cos being the mean cosine between the deltas - per tensor, or
per row of the tensor with ``stock_filter_wise: 1``.  ``nuslerp``: two deltas, their directions interpolated on the
sphere at alpha_1 / (alpha_0 + alpha_1), their lengths linearly, added onto output_base_model.  ``slerp``: the classic
spherical interpolation of two models' WEIGHTS (the bases are not part of the result).  The reference has no such
operators; the function is defined in include/shardmerge_hip.h (``smhip_geo_merge``) and runs in the HIP kernels of
csrc/sm_geo.hpp behind ``Engine.geo_merge``: an fp64 Gram pass whose summation order depends on the element count only,
a few scalars, one streaming pass.

Tensor routing is FourierMerge's, as with TiesMerge: only the block-tensor merge (``merge_block``) differs."""
from __future__ import annotations

import logging

from ..config import GEO_OPTION_DEFAULTS
from .ties import TiesMerge

logger = logging.getLogger(__name__)


class ModelStockMerge(TiesMerge):
    mode = "model_stock"
    title = "Model Stock"

    option_defaults = GEO_OPTION_DEFAULTS

    def get_readme(self) -> str:
        scope = "per row of each tensor" if self.stock_filter_wise else "per tensor"
        return self._readme(self.title, f"Model Stock (model_stock: the weighted average of the deltas, pulled towards the base by the "
                                        f"ratio t of their mean cosine, {scope})")

    def merge_block(self, eng, fts, bases, alphas, base_out, name: str):
        return eng.geo_merge(fts, bases, alphas, base_out, mode=self.mode,
                             rowwise=bool(self.stock_filter_wise) and self.mode == "model_stock", layer_name=name)

    def tensor_passes(self, k: int) -> int:
        return 2 * k + 3                      # the Gram pass reads k + 1, the combine pass reads k + 1 and writes 1

    def _log_block(self, name: str, k: int, report):
        if report.rowwise:
            logger.info(f"Merged {name}: {k} model(s), Model Stock per row, t in [{report.t_min:.4g}, {report.t_max:.4g}], mean {report.t_mean:.4g}")
        else:
            logger.info(f"Merged {name}: {k} model(s), Model Stock, mean cosine {report.cos:.4g}, t {report.t:.4g}, "
                        f"coefficients {[float(f'{c:.4g}') for c in report.coefficients]}")


class NuSlerpMerge(ModelStockMerge):
    mode = "nuslerp"
    title = "NuSLERP"

    def get_readme(self) -> str:
        return self._readme(self.title, "NuSLERP (nuslerp: the two deltas' directions interpolated on the sphere at "
                                        "alpha_1 / (alpha_0 + alpha_1), their lengths linearly)")

    def _log_block(self, name: str, k: int, report):
        logger.info(f"Merged {name}: {k} model(s), {self.title}, cosine {report.cos:.4g}, angle {report.omega:.4g}"
                    f"{' (linear)' if report.linear else ''}, coefficients {[float(f'{c:.4g}') for c in report.coefficients]}")


class SlerpMerge(NuSlerpMerge):
    mode = "slerp"
    title = "SLERP"

    def get_readme(self) -> str:
        return self._readme(self.title, "SLERP (slerp: the two models' weights interpolated on the sphere at alpha_1 / (alpha_0 + alpha_1))")

    def tensor_passes(self, k: int) -> int:
        return 2 * k + 1                      # no base is read
