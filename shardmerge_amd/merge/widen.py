"""WidenMerge: WIDEN (Yu, Yu, Yu, Huang, Li, "Extend Model Merging from Fine-Tuned to Pre-Trained Large Language Models
via Weight Disentanglement", 2024) - the one operator that weighs a finetune per COLUMN of a weight matrix, and the one
built for finetunes whose deltas differ by orders of magnitude.  Every block tensor is viewed as ``[shape[0], rest]``;
per covering finetune and column, how far the column's magnitude and its direction moved from the base's is RANKED
within the finetune, the ranks become weights by a softmax across the finetunes, and a column ranked above
``widen_ratio`` times its finetune's mean rank takes ``widen_calibration`` instead.  A tensor whose first dimension is 1
(norm weights, 1-D tensors) ranks the magnitudes of its delta's entries.  The reference has no such operator; the
function is defined in include/shardmerge_hip.h (``smhip_widen_merge``) and runs in the HIP kernels of csrc/sm_widen.hpp
behind ``Engine.widen_merge``.

Tensor routing is FourierMerge's, as with TiesMerge: only the block-tensor merge (``merge_block``) differs.  The ranks
are counted over all pairs of columns, so a block tensor may have at most 65536 of them: ``initialize`` checks every
block tensor before anything is written."""
from __future__ import annotations

import json
import logging
import math

from ..config import WIDEN_MAX_COLS, WIDEN_OPTION_DEFAULTS
from .ties import TiesMerge

logger = logging.getLogger(__name__)


def widen_view(shape):
    """(R, C) of a tensor of this shape: [shape[0] x the rest], a 1-D tensor is one row"""
    shape = tuple(int(v) for v in shape)
    if len(shape) < 2:
        return 1, math.prod(shape)
    return shape[0], math.prod(shape[1:])


class WidenMerge(TiesMerge):
    option_defaults = WIDEN_OPTION_DEFAULTS

    async def initialize(self):
        await super().initialize()
        self.check_columns()

    def check_columns(self):
        """every block tensor has at most WIDEN_MAX_COLS columns, else ValueError naming the tensor"""
        uri = self.config.output_base_model
        weight_map = self.index_manager.model_indexes[uri]["weight_map"]
        for shard in sorted(set(weight_map.values())):
            with open(self.index_manager.storage_path / uri / shard, "rb") as fh:
                header = json.loads(fh.read(int.from_bytes(fh.read(8), "little")))
            for name, rec in sorted(header.items()):
                if not name.startswith("model.layers.") or "shape" not in rec:
                    continue
                rows, cols = widen_view(rec["shape"])
                if cols > WIDEN_MAX_COLS:
                    raise ValueError(f"operator widen: {name} {list(rec['shape'])} has {cols} columns ([shape[0] x the rest]), "
                                     f"at most {WIDEN_MAX_COLS} can be ranked.  Nothing was written")

    def get_readme(self) -> str:
        return self._readme("WIDEN", f"WIDEN (weight disentanglement: per column, the divergence of magnitude and direction "
                                     f"ranked within each finetune, a softmax across the finetunes, the columns above the cut "
                                     f"calibrated), ratio {self.widen_ratio:g}, calibration {self.widen_calibration:g}, "
                                     f"lambda {self.widen_lambda:g}")

    def merge_block(self, eng, fts, bases, alphas, base_out, name: str):
        return eng.widen_merge(fts, bases, alphas, base_out, ratio=self.widen_ratio, calibration=self.widen_calibration,
                               lam=self.widen_lambda, layer_name=name)

    def tensor_passes(self, k: int) -> int:
        # the column statistics read every finetune and its base (2 k), the combine pass k + 2
        return 3 * k + 2

    def _log_block(self, name: str, k: int, report):
        share = lambda c: float(f"{c / max(report.cols, 1):.4g}")
        stats = ("|delta|",) if report.vector_mode else ("magnitude", "direction")
        parts = ", ".join(f"{s} {[share(report.calibrated[i][j]) for i in range(k)]}" for j, s in enumerate(stats))
        logger.info(f"Merged {name}: {k} model(s), WIDEN {'vector' if report.vector_mode else 'matrix'} mode "
                    f"{report.rows} x {report.cols}, calibrated share per finetune: {parts}")
