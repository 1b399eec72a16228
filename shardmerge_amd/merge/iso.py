"""IsoMerge: Iso-C, isotropic merging (Marczak et al., "No Task Left Behind: Isotropic Model Merging with Common and
Task-Specific Subspaces", ICML 2025).  Every block tensor with at least two dimensions is viewed as ``[shape[0], rest]``;
the deltas of the covering finetunes are summed with their alphas into one task matrix ``T = U S V^T`` whose spectrum is
replaced by its mean: ``mean(S) U V^T`` is added, times ``iso_lambda``, onto output_base_model.  ``U V^T`` is the polar
factor of ``T`` and ``mean(S) = <U V^T, T> / min(rows, cols)``, so no SVD is taken: a Newton-Schulz iteration on the
fp32 MFMA GEMM of csrc/sm_iso.hpp stops at ``||X X^T - I||_F / sqrt(s) <= iso_tol`` or after ``iso_max_iter`` steps.  The
reference has no such operator; the function is defined in include/shardmerge_hip.h (``smhip_iso_merge``) and runs
behind ``Engine.iso_merge``.

Tensor routing is FourierMerge's, as with TiesMerge: only the block-tensor merge (``merge_block``) differs.  A 0-D or 1-D
tensor has no spectrum and takes the normalised weighted mean of its deltas (``dare_linear`` at density 1) times
``iso_lambda``, as with TsvMerge; a matrix one entry covers is the function at k = 1.  ``initialize`` checks
``min(rows, cols) <= 16384`` for every block tensor before anything is written."""
from __future__ import annotations

import json
import logging
import math

from ..config import ISO_MAX_S, ISO_OPTION_DEFAULTS
from ..writer import ShardLayer
from .dare import tensor_key
from .ties import TiesMerge

logger = logging.getLogger(__name__)


class IsoMerge(TiesMerge):
    option_defaults = ISO_OPTION_DEFAULTS

    def __init__(self, config, index_manager=None, engine=None, **kwargs):
        super().__init__(config, index_manager=index_manager, engine=engine, **kwargs)
        opts = getattr(config, "merge_options", None) or {}
        self.iso_max_iter = int(opts.get("iso_max_iter", ISO_OPTION_DEFAULTS["iso_max_iter"]))      # exactly

    async def initialize(self):
        await super().initialize()
        self.check_sizes()

    def check_sizes(self):
        """every block matrix fits the iteration's s x s buffers, else ValueError naming the tensor"""
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
                    ShardLayer(0, shard, name, False).layer_number
                except ValueError:
                    continue                  # (the merge itself reports unknown names, as the reference does)
                s = min(shape[0], math.prod(shape[1:]))
                if s > ISO_MAX_S:
                    raise ValueError(f"operator iso_c: {name} {list(shape)} has min(rows, cols) = {s}; the iteration holds two "
                                     f"s x s matrices and takes at most {ISO_MAX_S}.  Nothing was written")

    def get_readme(self) -> str:
        return self._readme("Iso-C", f"Iso-C (isotropic merging: the summed delta's singular values replaced by their mean, by a "
                                     f"Newton-Schulz polar iteration), lambda {self.iso_lambda:g}, tol {self.iso_tol:g}, "
                                     f"max_iter {self.iso_max_iter}; 1-D tensors: the normalised weighted mean of the deltas")

    def merge_block(self, eng, fts, bases, alphas, base_out, name: str):
        if base_out.ndim < 2:
            return eng.dare_merge(fts, bases, alphas, base_out, density=1.0, lam=self.iso_lambda, normalize=True, rescale=True,
                                  sign_election=False, key=tensor_key(0, name), stream_ids=list(range(len(fts))),
                                  layer_name=name)
        return eng.iso_merge(fts, bases, alphas, base_out, lam=self.iso_lambda, tol=self.iso_tol, max_iter=self.iso_max_iter,
                             layer_name=name)

    def tensor_passes(self, k: int) -> int:
        # the k finetunes and their bases read once; base_out read and out written; the iteration's matrix products are
        # not streaming passes and are not counted
        return 2 * k + 2

    def _log_block(self, name: str, k: int, report):
        if not hasattr(report, "sigma_bar"):
            logger.info(f"Merged {name}: {k} model(s), Iso-C took the weighted mean of the deltas (not a matrix)")
            return
        if report.zero:
            logger.info(f"Merged {name}: {k} model(s), Iso-C: the summed delta is zero, the base is kept")
            return
        logger.info(f"Merged {name}: {k} model(s), Iso-C lambda {self.iso_lambda:g} tol {self.iso_tol:g}: {report.s} x {report.L}"
                    f"{' (transposed)' if report.transposed else ''}, steps {report.steps or '-'}, residual {report.e[-1]:.3g} "
                    f"{'converged' if report.converged else f'NOT converged after iso_max_iter = {self.iso_max_iter} steps'}, "
                    f"mean singular value {report.sigma_bar:.6g}")
