"""TsvMerge: TSV-Merge (Gargiulo et al., "Task Singular Vectors: Reducing Task Interference in Model Merging", CVPR
2025) - the one operator that looks at a task vector as a matrix.  Every block tensor with at least two dimensions is
viewed as ``[shape[0], rest]``; each covering finetune's delta is cut to its ``tsv_rank`` leading singular triplets (a
randomized subspace iteration, ``tsv_power_iters`` power steps, one sketch per tensor keyed by ``seed`` and the tensor's
name), the singular vectors of all finetunes are whitened together so that overlapping subspaces count once, and the
delta is rebuilt with the singular values times ``alpha`` and added, times ``tsv_lambda``, onto output_base_model.  The
reference has no such operator; the function is defined in include/shardmerge_hip.h (``smhip_tsv_merge``) and runs on
the kernels of csrc/sm_extract.hpp and ``tsv_apply`` of csrc/sm_tsv.hpp behind ``Engine.tsv_merge``.

Tensor routing is FourierMerge's, as with TiesMerge: only the block-tensor merge (``merge_block``) differs.  A 1-D tensor
has no singular vectors and a tensor one entry covers has nothing to whiten: both take the normalised weighted mean of
their deltas (``dare_linear`` at density 1) times ``tsv_lambda`` - the paper's rule for non-matrices.  The whitened
panels hold at most 256 vectors: ``initialize`` checks ``k * min(tsv_rank, rows, cols) <= 256`` for every block tensor
before anything is written."""
from __future__ import annotations

import json
import logging
import math

from ..config import TSV_MAX_VECTORS, TSV_OPTION_DEFAULTS
from ..writer import ShardLayer
from .dare import tensor_key
from .ties import TiesMerge

logger = logging.getLogger(__name__)


class TsvMerge(TiesMerge):
    option_defaults = TSV_OPTION_DEFAULTS

    def __init__(self, config, index_manager=None, engine=None, **kwargs):
        super().__init__(config, index_manager=index_manager, engine=engine, **kwargs)
        opts = getattr(config, "merge_options", None) or {}
        for key in ("tsv_rank", "tsv_power_iters", "seed"):         # exactly
            setattr(self, key, int(opts.get(key, TSV_OPTION_DEFAULTS[key])))

    async def initialize(self):
        await super().initialize()
        self.check_ranks()

    def _active(self, number: int):
        return [m for m in self.config.finetune_merge if m.use_layer_index(number)]

    def check_ranks(self):
        """every block matrix that several entries cover fits the whitened panels, else ValueError naming the tensor"""
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
                k = sum(1 for m in self._active(number) if m.alpha != 0)
                r = min(self.tsv_rank, shape[0], math.prod(shape[1:]))
                if len(self._active(number)) > 1 and k * r > TSV_MAX_VECTORS:
                    raise ValueError(f"operator tsv: {name} {list(shape)} is covered by {k} finetune_merge entries with a weight: "
                                     f"{k} x min(tsv_rank, rows, cols) = {k} x {r} = {k * r} singular vectors, at most "
                                     f"{TSV_MAX_VECTORS} fit; lower merge_options.tsv_rank to {TSV_MAX_VECTORS // k} or "
                                     f"narrow the layer windows.  Nothing was written")

    def get_readme(self) -> str:
        return self._readme("TSV", f"TSV (task singular vectors: the leading singular triplets of every delta, whitened across "
                                   f"the finetunes, rebuilt), rank {self.tsv_rank}, power iterations {self.tsv_power_iters}, "
                                   f"lambda {self.tsv_lambda:g}, seed {self.seed}; 1-D tensors and tensors of one entry: the "
                                   f"normalised weighted mean of the deltas")

    def merge_block(self, eng, fts, bases, alphas, base_out, name: str):
        if base_out.ndim < 2 or len(fts) == 1:
            return eng.dare_merge(fts, bases, alphas, base_out, density=1.0, lam=self.tsv_lambda, normalize=True, rescale=True,
                                  sign_election=False, key=tensor_key(self.seed, name), stream_ids=list(range(len(fts))),
                                  layer_name=name)
        return eng.tsv_merge(fts, bases, alphas, base_out, rank=self.tsv_rank, power_iters=self.tsv_power_iters,
                             lam=self.tsv_lambda, key=tensor_key(self.seed, name), layer_name=name)

    def tensor_passes(self, k: int) -> int:
        # k (2 q + 2) delta products and k energies of two reads each, base_out read and out written
        return 2 * k * (2 * self.tsv_power_iters + 3) + 2

    def _log_block(self, name: str, k: int, report):
        if not hasattr(report, "kept_U"):
            logger.info(f"Merged {name}: {k} model(s), TSV took the weighted mean of the deltas (not a matrix, or one entry)")
            return
        logger.info(f"Merged {name}: {k} model(s), TSV rank {self.tsv_rank} q {self.tsv_power_iters} lambda {self.tsv_lambda:g} "
                    f"seed {self.seed}: R {report.R}, kept_U {report.kept_U} / kept_W {report.kept_W}, energy shares "
                    f"{[float(f'{s:.4g}') for s in report.share]}")
