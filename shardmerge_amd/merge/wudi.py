"""WudiMerge: WUDI-Merging (Cheng et al., "Whoever Started the Interference Should End It: Guiding Data-Free Model Merging
via Task Vectors", ICML 2025).  Every block tensor with at least two dimensions is viewed as ``[shape[0], rest] = R x C``;
the merged task vector ``X`` minimises the interference ``sum_i ||(X - d_i) d_i^T||_F^2 / ||d_i||_F^2`` between the covering
finetunes' deltas ``d_i``, whose rows stand in for the layer's inputs, by ``wudi_iters`` Adam steps at ``wudi_lr`` from
the sum of the deltas times their alphas; ``X`` is added, times ``wudi_lambda``, onto output_base_model.  The gradient is
``2 (X S - P)`` with ``S`` and ``P`` built once, so a step is one product on the fp32 MFMA GEMMs of csrc/sm_wudi.hpp with
Adam's update as its epilogue.  The reference has no such operator; the function is defined in
include/shardmerge_hip.h (``smhip_wudi_merge``) and runs behind ``Engine.wudi_merge``.

Tensor routing is FourierMerge's, as with TiesMerge: only the block-tensor merge (``merge_block``) differs.  A 0-D or 1-D
tensor, and a matrix that the layer windows leave with ONE covering entry, take the normalised weighted mean of their
deltas (``dare_linear`` at density 1) times ``wudi_lambda``: with one task the gradient is zero in exact arithmetic, and
Adam would turn its rounding noise into steps of size ``wudi_lr``.  ``initialize`` checks ``C <= 32768`` for every block
tensor before anything is written."""
from __future__ import annotations

import json
import logging
import math

from ..config import WUDI_MAX_C, WUDI_OPTION_DEFAULTS
from ..writer import ShardLayer
from .dare import tensor_key
from .ties import TiesMerge

logger = logging.getLogger(__name__)


class WudiMerge(TiesMerge):
    option_defaults = WUDI_OPTION_DEFAULTS

    def __init__(self, config, index_manager=None, engine=None, **kwargs):
        super().__init__(config, index_manager=index_manager, engine=engine, **kwargs)
        opts = getattr(config, "merge_options", None) or {}
        self.wudi_iters = int(opts.get("wudi_iters", WUDI_OPTION_DEFAULTS["wudi_iters"]))      # exactly

    async def initialize(self):
        await super().initialize()
        self.check_sizes()

    def check_sizes(self):
        """every block matrix that several entries cover fits the C x C buffers, else ValueError naming the tensor"""
        uri = self.config.output_base_model
        weight_map = self.index_manager.model_indexes[uri]["weight_map"]
        for shard in sorted(set(weight_map.values())):
            with open(self.index_manager.storage_path / uri / shard, "rb") as fh:
                header = json.loads(fh.read(int.from_bytes(fh.read(8), "little")))
            for name, rec in sorted(header.items()):
                if not name.startswith("model.layers."):
                    continue
                shape = tuple(int(v) for v in rec["shape"])
                if len(shape) < 2 or not all(shape):
                    continue
                try:
                    number = ShardLayer(0, shard, name, False).layer_number
                except ValueError:
                    continue                  # (the merge itself reports unknown names, as the reference does)
                cols = math.prod(shape[1:])
                if sum(1 for m in self.config.finetune_merge if m.use_layer_index(number)) > 1 and cols > WUDI_MAX_C:
                    raise ValueError(f"operator wudi: {name} {list(shape)} has {cols} columns; the iteration holds two "
                                     f"C x C matrices and takes at most {WUDI_MAX_C}.  Nothing was written")

    def get_readme(self) -> str:
        return self._readme("WUDI", f"WUDI (the merged task vector that minimises the interference between the tasks, the task "
                                    f"vectors standing in for the data: Adam on 2 (X S - P)), iterations {self.wudi_iters}, "
                                    f"lr {self.wudi_lr:g}, lambda {self.wudi_lambda:g}; 1-D tensors and tensors of one entry: the "
                                    f"normalised weighted mean of the deltas")

    def merge_block(self, eng, fts, bases, alphas, base_out, name: str):
        if base_out.ndim < 2 or len(fts) == 1:
            return eng.dare_merge(fts, bases, alphas, base_out, density=1.0, lam=self.wudi_lambda, normalize=True, rescale=True,
                                  sign_election=False, key=tensor_key(0, name), stream_ids=list(range(len(fts))),
                                  layer_name=name)
        return eng.wudi_merge(fts, bases, alphas, base_out, iters=self.wudi_iters, lr=self.wudi_lr, lam=self.wudi_lambda,
                              layer_name=name)

    def tensor_passes(self, k: int) -> int:
        # every finetune and base read for its norm and for the start; base_out read and out written; the matrix products
        # (which re-read the 16-bit inputs tile by tile) are not streaming passes and are not counted
        return 4 * k + 2

    def _log_block(self, name: str, k: int, report):
        if not hasattr(report, "grad_sq_first"):
            logger.info(f"Merged {name}: {k} model(s), WUDI took the weighted mean of the deltas (not a matrix, or one entry)")
            return
        if report.zero:
            logger.info(f"Merged {name}: {k} model(s), WUDI: no entry with a weight and a delta, the base is kept")
            return
        logger.info(f"Merged {name}: k {len(report.active)} of {k} model(s), WUDI lr {self.wudi_lr:g} lambda {self.wudi_lambda:g}: "
                    f"{report.R} x {report.C}, iterations {report.iterations}, grad_sq {report.grad_sq_first:.6g} -> "
                    f"{report.grad_sq_last:.6g}")
